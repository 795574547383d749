"""The launches of the fast K-quant decode step over a Q6_K BODY (enqueue_segment_k<Q6_K>: k_qkv<Q6_K>, attention, k_gemv_res_nq<Q6_K,
SPLIT, QIN> for wo, k_gateup_k_lds<.., Q6_K>, the same for ffn_down, the classifier) restated in float64 for the tap recorder.
tests/fused_step_ref.py's K forms already read Q6_K rows (weight_rows, k_pieces, _chunk_dots: the attn_v / ffn_down rows of a *_K_M
layer and the Q6_K classifier go through them), and nothing in check_layer_k depends on the body's format -- the Q8_K interval
check with its EXCUSED_CAP, the norm intervals, the attention and classifier checks -- so check_layer here IS R.check_layer_k.  The
rhs of a Q6_K row is the ELEMENT-order plane (`q`, which k_pieces takes for Q6_K), and R.shrink_residual knows Q6_K's d (byte 208).

  Q6_K block (buf_q6_k.rs:11-18): ql[128] | qh[64] | scales i8[16] | d f16 = 210 bytes.  Element 128 h + 32 j + l of a super-block
      (half h, quarter j < 4, l < 32) has the level (nibble j >> 1 of ql[64 h + 32 (j & 1) + l]) + 16 * (bits 2 j, 2 j + 1 of
      qh[32 h + l]) - 32 and the scale sc[8 h + 2 j + l / 16] (buf_q6_k.rs:21-48).
  Q6_K row dot (q6k_term, gemv_core.hpp): a lane's PIECE (h, a, p) is the 16 bytes ql[64 h + 32 a + 16 p .. + 16] with the two-bit
      fields 2 a (low nibbles) and 2 a + 4 (high) of qh[32 h + 16 p .. + 16]: the low nibbles are scale group g = 8 h + 2 a + p, the
      high ones group g + 4.  Exact integers lo = sum(q6 q8 | group g) - 32 bsums[g], hi likewise for g + 4 (|lo|, |hi| <= 16 * 63 *
      128 + 32 * 16 * 128 < 2^18), scaled by the signed byte scales (|sc lo| < 2^25: the conversions to f32 may round), and the f32
      term f32(d_w d8) * (f32(sc_lo lo) + f32(sc_hi hi)).  fused_step_ref's derivation (its module docstring) stands word for word:
      three roundings per piece on A = |d_w d8| (|sc_lo lo| + |sc_hi hi|), the 8 nsb terms of a row added in some order --
          |f32 - exact| <= (8 nsb + C_K) U sum A
      order-free, so it covers the prologue-first add order of wo, ffn_down and gate | up too.

What this module adds is the list of subtly WRONG kernels the Q6_K body loader could be (the checker's own tests: every one must
land outside the bound): k_pieces below restates R.k_pieces' Q6_K arm from the block's raw fields so that each can be named."""
import contextlib

import numpy as np

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests.fused_step_ref import C_K, EXCUSED_CAP, U, _u16, f16v  # noqa: F401

WRONG = ("qh_bits_dropped", "qh_twin_shift", "scales_swapped", "q6_scale_shift", "offset_dropped", "bsum_neighbour", "d_sign_lost")
_R_weight_rows, _R_chunk_dots = R.weight_rows, R._chunk_dots


def levels(lo4, qh, twin=False, drop=False):
    """the 6-bit levels 0 .. 63 in element order, [.., 256], from lo4 [.., 2, 4, 32] (the nibbles, element order) and qh [.., 64]: bits
    2 j, 2 j + 1 of qh[32 h + l] for element 128 h + 32 j + l.  twin: the field of the lane with the other `a` (j ^ 1); drop: none"""
    out = np.empty(lo4.shape, dtype=np.int64)
    for h in range(2):
        for j in range(4):
            hi2 = (qh[..., 32 * h:32 * h + 32] >> (2 * (j ^ 1 if twin else j))) & 3
            out[..., h, j, :] = lo4[..., h, j, :] + (0 if drop else 16 * hi2)
    return out.reshape(lo4.shape[:-3] + (256,))


def weight_rows(t, r0, r1):
    """fused_step_ref.weight_rows with the raw fields of Q6_K rows beside it: lo4 (the nibbles in element order) and qh"""
    w = _R_weight_rows(t, r0, r1)
    if t.typ != synth.Q6_K:
        return w
    rows, k = t.shape
    b = np.ascontiguousarray(t.data).view(np.uint8).reshape(rows, k // 256, 210)[r0:r1]
    ql = b[:, :, 0:128].astype(np.int64).reshape(b.shape[0], b.shape[1], 2, 2, 32)  # [half h, a, l]
    w["lo4"] = np.stack([ql[:, :, :, 0] & 0xF, ql[:, :, :, 1] & 0xF, ql[:, :, :, 0] >> 4, ql[:, :, :, 1] >> 4], axis=3)  # quarter j = a + 2 * (high nibble)
    w["qh"] = b[:, :, 128:192].astype(np.int64)
    assert np.array_equal(levels(w["lo4"], w["qh"]) - 32, w["q6"])
    return w


def k_pieces(w, act, wrong=None):
    """Q6_K weight rows against one row's Q8_K blocks, per piece (h, a, p) = index 4 h + 2 a + p of every row: the exact term and the
    magnitude A its roundings act on -> (terms, A), each [rows, nsb, 8].  wrong: a kernel that is subtly wrong in the named way"""
    assert w["typ"] == synth.Q6_K and (wrong is None or wrong in WRONG), wrong
    r, nsb = w["d"].shape
    d8, bs = act["d"], act["bsums"].astype(np.float64)
    assert d8.size == nsb and bs.shape == (nsb, 16), (d8.size, nsb, bs.shape)
    q = levels(w["lo4"], w["qh"], twin=wrong == "qh_twin_shift", drop=wrong == "qh_bits_dropped").astype(np.float64)
    x = act["q"].astype(np.float64).reshape(nsb, 16, 16)  # ELEMENT order: [scale group g, i]
    S = np.einsum("rsgi,sgi->rsg", q.reshape(r, nsb, 16, 16), x)
    off = bs
    if wrong == "bsum_neighbour":  # (the entry of group g + 1, as an off-by-one in the piece's index would take)
        off = np.roll(bs, -1, axis=1)
    G = S - (0.0 if wrong == "offset_dropped" else 32.0 * off[None])
    assert np.max(np.abs(G)) < 2 ** 18
    sc = w["sc"]
    if wrong == "q6_scale_shift":
        sc = sc.copy()
        sc[:, 0, 5] = w["sc"][:, 0, 6]
    if wrong == "scales_swapped":  # the low nibbles' group takes the high nibbles' scale and the other way round
        sc = sc.reshape(r, nsb, 2, 2, 4)[:, :, :, ::-1].reshape(r, nsb, 16)
    G = (sc * G).reshape(r, nsb, 2, 2, 4)  # group 8 h + 4 hi + (2 a + p); a piece: the low nibbles of group 8 h + 2 a + p, the high of + 4
    d = np.abs(w["d"]) if wrong == "d_sign_lost" else w["d"]
    dd = (d * d8[None])[:, :, None, None]
    return (dd * (G[:, :, :, 0] + G[:, :, :, 1])).reshape(r, nsb, 8), (np.abs(dd) * (np.abs(G[:, :, :, 0]) + np.abs(G[:, :, :, 1]))).reshape(r, nsb, 8)


def _chunk_dots(w, typ, act, k, drop_last_block, wrong=None):
    if typ != synth.Q6_K:
        return _R_chunk_dots(w, typ, act, k, drop_last_block, wrong)
    assert act["qt"] == o.Q8_K
    terms, A = k_pieces(w, act, wrong)
    if drop_last_block:
        terms = terms[:, :-1]
    return terms.sum(axis=(1, 2)), (A.shape[1] * 8 + C_K) * U * A.sum(axis=(1, 2))


@contextlib.contextmanager
def q6k_rows():
    """fused_step_ref's row dots go through this module's Q6_K pieces (and its wrong kernels) inside this block"""
    saved = R.weight_rows, R._chunk_dots
    R.weight_rows, R._chunk_dots = weight_rows, _chunk_dots
    try:
        yield
    finally:
        R.weight_rows, R._chunk_dots = saved


def row_dots(t, act, chunk=256, drop_last_block=False, wrong=None):
    with q6k_rows():
        return R.row_dots(t, act, chunk, drop_last_block, wrong)


def check_layer(tap, kc_raw, vc_raw, model, l, pos, form, ctx, twin=None, token=None):
    """every launch of the tapped layer (and the classifier) of a step over a Q6_K body -> {launch: Result}: fused_step_ref's own K
    checker, unwrapped (its row dots read Q6_K rows against the element-order plane as they are)"""
    assert model.wtype == synth.Q6_K and tap["plan"]["path"] == 2, (model.wtype, tap["plan"])
    return R.check_layer_k(tap, kc_raw, vc_raw, model, l, pos, form, ctx, twin, token)


def shrink_residual(model, log2=9):
    """fused_step_ref.shrink_residual (it knows Q6_K's d at byte 208; a Q4_K classifier is no residual writer) -- the embedding of a
    model with another output type is the body's"""
    return R.shrink_residual(model, log2)


def flip_signs(model, seed=5):
    """block scales of either sign: the sign bit of Q6_K's d (byte 209) on every Q6_K tensor"""
    rng = np.random.default_rng(seed)
    for t in model.tensors.values():
        if t.typ == synth.Q6_K:
            blk = t.data.reshape(-1, synth.BLOCK_BYTES[t.typ])
            blk[:, 209] ^= (rng.integers(0, 2, size=blk.shape[0], dtype=np.uint8) << 7)
    return model


failures = R.failures
