"""The launches of the fast K-quant decode step over a Q3_K BODY (enqueue_segment_k<Q3_K>: k_qkv<Q3_K>, attention, k_gemv_res_nq<F,
SPLIT, QIN> for wo with F the tensor's own format, k_gateup_k_lds<.., Q3_K>, the same for ffn_down, the classifier) restated in
float64 for the tap recorder.  The body is the Q3_K recipe family: attn_q, attn_k, ffn_gate and ffn_up are Q3_K, attn_v, attn_output
and ffn_down each Q3_K, Q4_K or Q5_K (the Q3_K_S / _M / _L recipes), the classifier any Q8_K-rhs format.  fused_step_ref's K forms
read Q4_K and Q6_K rows, q5k_step_ref's wrappers add Q5_K rows; this module adds Q3_K rows ON TOP of those wrappers (its weight_rows
/ _chunk_dots dispatch back to q5k_step_ref's for every other format, which dispatch back to fused_step_ref's), so a Q3_K_M layer's
Q5_K and Q4_K rows are read by the same check.  Nothing else in check_layer_k depends on the body's format.

  Q3_K block (buf_q3_k.rs:19-30): hmask[32] | qs[64] | scales[12] | d f16 = 110 bytes.  Element 128 half + 32 s + l of a super-block
      (half < 2, field s < 4, l < 32) has the level ((qs[32 half + l] >> 2 s) & 3 | bit (4 half + s) of hmask[l] as bit 2) - 4, i.e.
      -4 .. 3, and the scale group g = 8 half + 2 s + l / 16 (buf_q3_k.rs:62-83).  The 6-bit scale of group g (buf_q3_k.rs:44-56): low
      four bits = nibble g / 8 of scales[g % 8], high two bits = bits 2 (g / 4), 2 (g / 4) + 1 of scales[8 + g % 4]; minus 32.
  Q3_K row dot (q3k_term = PieceQ3_K::term, gemv_core.hpp): a lane's PIECE (half, h) is the 16 bytes qs[32 half + 16 h .. + 16] with
      hmask[16 h .. + 16]; its field s is group g = 8 half + 2 s + h.  Per group the exact integer G_g = sum((q2 | hbit << 2) q8) - 4
      bsums[g] (|G_g| <= 16 * 4 * 128 = 2^13), scaled: (sc_g - 32) G_g (|.| <= 2^18); the four pieces of a super-block add their four
      groups each across the quad: tot = sum_g (sc_g - 32) G_g, |tot| <= 2^22 < 2^24 -- an exact integer whose conversion to f32 is
      exact.  Then ONE f32 expression per SUPER-BLOCK, (f32(d_w) * d8) * (float)tot: f32(d_w) is exact (an f16), the product with d8
      rounds once, the product with tot once -- TWO roundings on |d_w d8 tot|: the term is off by at most 2 U |term| (1 + U).  The nsb
      terms of a row (quad lanes 1 .. 3 add +0.0, which changes no bit) are added in some order -- a lane's in ascending order, the
      lanes through a tree, the leading pieces of the prologue forms first --, nsb - 1 additions, each off by at most U times a
      partial sum of |terms|: the kernel alone would be held by (nsb + 2) U sum |term|.
  The reference's own order (buf_q3_k.rs:303-327) is another association, and a checker of the step has to admit it as well (its own
      tests hold an oracle-built tap to it): eight i32 lanes per super-block, aux_l = sum over the elements e with e % 8 = l of (sc - 32)
      lv q8 (sum_l aux_l = tot), `sums[l] += (f32(d_w) * d8) * (float)aux_l` super-block after super-block, the eight lanes added at
      the end.  Its roundings act on the LANES' magnitudes, which cancellation between lanes can leave far above |tot|: two per term,
      nsb - 1 additions per lane, seven additions of the lanes.  With
          A = |d_w d8| sum_l |aux_l|   (>= |term|: it covers the kernel's expression too)
          |f32 - exact| <= (n_terms + C_Q3K) U sum A,   n_terms = nsb,   C_Q3K = 9
      two for the term, minus one, seven for the lanes, plus one for every second-order term (nsb^2 U^2 < 2e-4 U for the longest row
      here, 56 super-blocks).  Order-free, so it covers the prologue-first add order of wo, ffn_down and gate | up too.  (Measured on
      the models of tests/test_q3k_step_ref.py: with A = |term| the reference's own step lands up to 277 bounds out on rows whose
      super-blocks nearly cancel; it is the reference that is off there, by its lanes' magnitudes, not the kernel.)

What this module also holds is the list of subtly WRONG kernels the Q3_K body loader could be (the checker's own tests: every one must
land outside the bound)."""
import contextlib

import numpy as np

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests import q5k_step_ref as Q5
from tests.fused_step_ref import EXCUSED_CAP, U, _u16, f16v  # noqa: F401

C_Q3K = 9
WRONG = ("hmask_dropped", "hmask_other_half", "hmask_twin_piece", "offset_dropped", "scale_high_neighbour", "scale_without_32", "bsum_neighbour")
FAMILY = (synth.Q3_K, synth.Q4_K, synth.Q5_K)  # what attn_v / attn_output / ffn_down of the family may be


def levels(q2, hmask, wrong=None):
    """the levels 0 .. 7 (before the -4) in element order, [.., 256], from q2 [.., 2, 4, 32] (the 2-bit fields: half, s, l) and hmask
    [.., 32]: bit 4 half + s of hmask[l].  wrong: hmask_dropped (no bit), hmask_other_half (the bit of the other half: off by 4),
    hmask_twin_piece (the byte of the lane with the other h: l ^ 16)"""
    out = np.empty(q2.shape, dtype=np.int64)
    hm = hmask[..., np.arange(32) ^ 16] if wrong == "hmask_twin_piece" else hmask
    for half in range(2):
        for s in range(4):
            bit = 4 * ((1 - half) if wrong == "hmask_other_half" else half) + s
            hb = 0 if wrong == "hmask_dropped" else (hm >> bit) & 1
            out[..., half, s, :] = q2[..., half, s, :] | (hb << 2)
    return out.reshape(q2.shape[:-3] + (256,))


def scales(s12, wrong=None):
    """the sixteen 6-bit scales of a super-block minus 32, [.., 16], from scales[12].  wrong: scale_high_neighbour (the high two bits
    from the neighbouring byte of scales[8 .. 11]), scale_without_32"""
    out = np.empty(s12.shape[:-1] + (16,), dtype=np.int64)
    for g in range(16):
        lo = (s12[..., g % 8] >> (4 * (g // 8))) & 0xF
        hi = (s12[..., 8 + ((g % 4) ^ (1 if wrong == "scale_high_neighbour" else 0))] >> (2 * (g // 4))) & 3
        out[..., g] = (lo | (hi << 4)) - (0 if wrong == "scale_without_32" else 32)
    return out


def weight_rows(t, r0, r1):
    """q5k_step_ref.weight_rows (Q5_K, and fused_step_ref's formats behind it) with Q3_K from the raw 110-byte block: d, the 2-bit
    fields q2 [.., half, s, l], hmask, scales[12] and what they make -- lv (levels - 4, element order) and sc (scales - 32)"""
    if t.typ != synth.Q3_K:
        return Q5.weight_rows(t, r0, r1)
    rows, k = t.shape
    b = np.ascontiguousarray(t.data).view(np.uint8).reshape(rows, k // 256, 110)[r0:r1]
    qs = b[:, :, 32:96].astype(np.int64).reshape(b.shape[0], b.shape[1], 2, 32)
    q2 = np.stack([(qs >> (2 * s)) & 3 for s in range(4)], axis=3)  # [half, s, l]
    hmask, s12 = b[:, :, 0:32].astype(np.int64), b[:, :, 96:108].astype(np.int64)
    return {"typ": t.typ, "d": f16v(_u16(b[:, :, 108:110])), "q2": q2, "hmask": hmask, "s12": s12,
            "lv": (levels(q2, hmask) - 4).astype(np.float64), "sc": scales(s12).astype(np.float64)}


def k_values(w):
    """the dequantized elements of Q3_K rows, f64 [rows, nsb * 256] (16 groups of 16 elements: element order IS group order)"""
    r, nsb = w["d"].shape
    return ((w["d"][:, :, None] * w["sc"])[:, :, :, None] * w["lv"].reshape(r, nsb, 16, 16)).reshape(r, -1)


def k_terms(w, act, wrong=None):
    """Q3_K weight rows against one row's Q8_K blocks: per SUPER-BLOCK of every row the exact term d_w d8 tot and the magnitude A its
    roundings act on -> (terms, A), each [rows, nsb].  wrong: a kernel that is subtly wrong in the named way"""
    assert w["typ"] == synth.Q3_K and (wrong is None or wrong in WRONG), wrong
    r, nsb = w["d"].shape
    d8, bs = act["d"], act["bsums"].astype(np.float64)
    assert d8.size == nsb and bs.shape == (nsb, 16), (d8.size, nsb, bs.shape)
    lv = levels(w["q2"], w["hmask"], wrong).astype(np.float64)  # 0 .. 7, as the kernel's v_dot4 takes them
    x = act["q"].astype(np.float64).reshape(nsb, 16, 16)        # ELEMENT order: [scale group g, i]
    S = np.einsum("rsgi,sgi->rsg", lv.reshape(r, nsb, 16, 16), x)
    off = np.roll(bs, -1, axis=1) if wrong == "bsum_neighbour" else bs  # (the entry of group g + 1, as an off-by-one in the index would take)
    G = S - (0.0 if wrong == "offset_dropped" else 4.0 * off[None])
    assert np.max(np.abs(G)) <= 2 ** 13 + (2 ** 13 if wrong else 0)
    sc = scales(w["s12"], wrong).astype(np.float64)
    tot = (sc * G).sum(axis=2)
    assert wrong or np.max(np.abs(tot)) < 2 ** 24
    # the reference's eight lanes (element e of a group feeds lane e % 8; the -4 is part of its levels)
    aux = np.einsum("rsg,rsghl,sghl->rsl", sc, (lv - 4.0).reshape(r, nsb, 16, 2, 8), x.reshape(nsb, 16, 2, 8))
    dd = w["d"] * d8[None]
    return dd * tot, np.abs(dd) * np.abs(aux).sum(axis=2)


def _chunk_dots(w, typ, act, k, drop_last_block, wrong=None):
    if typ != synth.Q3_K:
        return Q5._chunk_dots(w, typ, act, k, drop_last_block, wrong)
    assert act["qt"] == o.Q8_K
    terms, A = k_terms(w, act, wrong)
    if drop_last_block:
        terms = terms[:, :-1]
    return terms.sum(axis=1), (A.shape[1] + C_Q3K) * U * A.sum(axis=1)


@contextlib.contextmanager
def q3k_rows():
    """fused_step_ref's row dots read Q3_K rows (and, through q5k_step_ref's wrappers, Q5_K rows) inside this block"""
    saved = R.weight_rows, R._chunk_dots
    R.weight_rows, R._chunk_dots = weight_rows, _chunk_dots
    try:
        yield
    finally:
        R.weight_rows, R._chunk_dots = saved


def row_dots(t, act, chunk=256, drop_last_block=False, wrong=None):
    with q3k_rows():
        return R.row_dots(t, act, chunk, drop_last_block, wrong)


def check_layer(tap, kc_raw, vc_raw, model, l, pos, form, ctx, twin=None, token=None):
    """every launch of the tapped layer (and the classifier) of a step over a Q3_K body -> {launch: Result}"""
    assert model.wtype == synth.Q3_K and tap["plan"]["path"] == 2, (model.wtype, tap["plan"])
    for n in ("attn_q", "attn_k", "ffn_gate", "ffn_up"):
        assert model.tensors[f"blk.{l}.{n}.weight"].typ == synth.Q3_K, n
    for n in ("attn_v", "attn_output", "ffn_down"):
        assert model.tensors[f"blk.{l}.{n}.weight"].typ in FAMILY, n
    with q3k_rows():
        return R.check_layer_k(tap, kc_raw, vc_raw, model, l, pos, form, ctx, twin, token)


# byte offsets of the f16 block scales (d; d | dmin) of the formats a member of the family holds in the matrices that write the residual
_SCALES_AT = {synth.Q3_K: (108,), synth.Q4_K: (0, 2), synth.Q5_K: (172, 174), synth.Q6_K: (208,)}


def shrink_residual(model, log2=9):
    """fused_step_ref.shrink_residual for a member of the Q3_K family: every block scale of the matrices that write the residual stream
    (the embedding, attn_output, ffn_down) times 2^-log2 -- Q3_K's d sits at byte 108 of the block"""
    for name, t in model.tensors.items():
        if not (name == "token_embd.weight" or name.endswith("attn_output.weight") or name.endswith("ffn_down.weight")):
            continue
        assert t.typ in _SCALES_AT, name
        blk = t.data.reshape(-1, synth.BLOCK_BYTES[t.typ])
        for lo in _SCALES_AT[t.typ]:
            bits = np.ascontiguousarray(blk[:, lo:lo + 2]).view(np.uint16).reshape(-1)
            v = (f16v(bits) * 2.0 ** -log2).astype(np.float16)
            blk[:, lo:lo + 2] = v.view(np.uint8).reshape(-1, 2)
    return model


def flip_signs(model, seed=5):
    """block scales of either sign: the sign bit of every f16 block scale (Q3_K's d: byte 109) on every K-quant tensor"""
    rng = np.random.default_rng(seed)
    for t in model.tensors.values():
        at = _SCALES_AT.get(t.typ, ())
        blk = t.data.reshape(-1, synth.BLOCK_BYTES[t.typ]) if at else None
        for lo in at:
            blk[:, lo + 1] ^= (rng.integers(0, 2, size=blk.shape[0], dtype=np.uint8) << 7)
    return model


failures = R.failures
