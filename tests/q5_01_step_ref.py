"""The five launches of the fast fused decode step over Q5_0 / Q5_1 layers (enqueue_segment_t<Q5_0 / Q5_1>: k_qkv, attention,
k_gemv_res_nq for wo, k_gateup_q, k_gemv_res_nq for ffn_down, the classifier; Q5_1 in front of a classifier of another format:
enqueue_segment_k<Q5_1>) restated in float64 for the tap recorder.  Built on tests/fused_step_ref.py without editing it: nothing in
its launch checkers depends on the weight format beyond weight_rows (the unpack) and _chunk_dots (the term and its bound), and
those two are what this module supplies for the two formats, inside q5_rows().

  Q5_0 block (buf_q5_0.rs:13-19): d f16 | qh u32 | qs[16] = 22 bytes.  Element i < 16 has the level (qs[i] & 15) | bit i of qh << 4,
      element 16 + i the level (qs[i] >> 4) | bit 16 + i of qh << 4; its value is (level - 16) * d (buf_q5_0.rs:22-37).
  Q5_0 row dot (BlockFmt<Q5_0>::term, gemv_core.hpp; the reference: buf_q5_0.rs:158): sumi = sum (level - 16) * q8 is an exact
      integer, |sumi| <= 32 * 16 * 127 < 2^24, so (float)sumi is exact; the term is ((float)sumi * d_w) * d_x, TWO roundings, and the nb
      terms are added in some order: fused_step_ref's Q4_0 derivation stands word for word,
          |f32 - exact| <= (nb + C_DOT) U sum_b |t_b|.
      With w["q"] = level - 16 and w["d"] the f16 scale, R._chunk_dots' Q4_0 / Q8_0 arm computes exactly this.
  Q5_1 block (buf_q5_1.rs:10-17): d f16 | m f16 | qh u32 | qs[16] = 24 bytes, the same levels, value level * d + m.
  Q5_1 row dot (BlockFmt<Q5_1>::term; buf_q5_1.rs:156): f16(d_w d_x) * (float)sumi + f16(m s), sumi = sum level * q8 exact (|sumi| <=
      32 * 31 * 128 < 2^24), the two f16 products part of the expression and restated exactly (the exact product of two f16 values
      fits float64, rounded once to f16): Q4_1's bound, (nb + C_DOT) U sum_b (|f16(d_w d_x) sumi| + |f16(m s)|), never more than
      8 GEMV_REL sum_i |w_i x_i|.  R._chunk_dots' Q4_1 arm with w["q"] = level computes exactly this.

What this module adds beside the unpack is the list of subtly WRONG loaders the two formats could have (the checker's own tests: each
must land outside the bound)."""
import contextlib

import numpy as np

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests.fused_step_ref import C_DOT, EXCUSED_CAP, U, _u16, f16v  # noqa: F401

# a loader that ...: drops the fifth bits; takes the high half's bits for the low half and the other way round; takes bit i of qh for
# element i's NEIGHBOUR in the dword (the bits of a nibble group reversed); forgets the -16 (Q5_0) / the minimum (Q5_1); reads the
# scale of the next block (a third plane addressed one unit off); reads qh of the next block
WRONG = ("qh_bits_dropped", "qh_halves_swapped", "qh_bits_reversed_in_group", "offset_dropped", "scale_neighbour", "qh_neighbour")
_R_weight_rows, _R_chunk_dots, _R_shrink = R.weight_rows, R._chunk_dots, R.shrink_residual
Q5 = (synth.Q5_0, synth.Q5_1)


def levels(qs, qh, wrong=None):
    """the 32 levels 0 .. 31 of every block in element order, [.., 32], from qs [.., 16] and qh [..] (the u32)"""
    qs, qh = qs.astype(np.int64), qh.astype(np.int64)
    if wrong == "qh_neighbour":
        qh = np.roll(qh, -1, axis=-1)
    sh = np.arange(32)
    if wrong == "qh_halves_swapped":
        sh = (sh + 16) % 32
    if wrong == "qh_bits_reversed_in_group":
        sh = (sh & ~3) | (3 - (sh & 3))
    bits = (qh[..., None] >> sh) & 1
    if wrong == "qh_bits_dropped":
        bits = bits * 0
    return np.concatenate([qs & 15, qs >> 4], axis=-1) | (bits << 4)


def weight_rows(t, r0, r1, wrong=None):
    """fused_step_ref.weight_rows for Q5_0 / Q5_1 rows (every other format: its own): d [rows, nb], q [rows, nb, 32] -- level - 16
    (Q5_0) or level (Q5_1) -- and m (Q5_1), with the raw fields beside them"""
    if t.typ not in Q5:
        return _R_weight_rows(t, r0, r1)
    rows, k = t.shape
    bb = synth.BLOCK_BYTES[t.typ]
    b = np.ascontiguousarray(t.data).view(np.uint8).reshape(rows, k // 32, bb)[r0:r1]
    h = 2 if t.typ == synth.Q5_0 else 4
    qh = np.ascontiguousarray(b[:, :, h:h + 4]).view("<u4")[..., 0]
    lv = levels(b[:, :, h + 4:], qh, wrong).astype(np.float64)
    d = f16v(_u16(b[:, :, 0:2]))
    if wrong == "scale_neighbour":
        d = np.roll(d, -1, axis=1)
    w = {"typ": t.typ, "d": d, "qs": b[:, :, h + 4:], "qh": qh}
    if t.typ == synth.Q5_0:
        w["q"] = lv - (0.0 if wrong == "offset_dropped" else 16.0)
    else:
        w["q"] = lv
        m = f16v(_u16(b[:, :, 2:4]))
        w["m"] = m * 0.0 if wrong == "offset_dropped" else m
    return w


def _chunk_dots(w, typ, act, k, drop_last_block, wrong=None):
    """R._chunk_dots with Q5_0 rows through its Q4_0 / Q8_0 arm (the same two-rounding term on w["q"] = level - 16) and Q5_1 rows
    through its Q4_1 arm (the same f16 products on w["q"] = level): see the module docstring"""
    if typ == synth.Q5_0:
        assert act["qt"] == o.Q8_0 and np.abs(np.einsum("rbi,bi->rb", w["q"], act["q"].astype(np.float64))).max() <= 32 * 16 * 127
        return _R_chunk_dots(w, synth.Q4_0, act, k, drop_last_block, None)
    if typ == synth.Q5_1:
        return _R_chunk_dots(w, synth.Q4_1, act, k, drop_last_block, None)
    return _R_chunk_dots(w, typ, act, k, drop_last_block, wrong)


@contextlib.contextmanager
def q5_rows(wrong=None):
    """fused_step_ref's row dots go through this module's Q5_0 / Q5_1 rows (and its wrong loaders) inside this block"""
    saved = R.weight_rows, R._chunk_dots
    R.weight_rows = (lambda t, r0, r1: weight_rows(t, r0, r1, wrong)) if wrong else weight_rows
    R._chunk_dots = _chunk_dots
    try:
        yield
    finally:
        R.weight_rows, R._chunk_dots = saved


def row_dots(t, act, chunk=256, drop_last_block=False, wrong=None):
    with q5_rows(wrong):
        return R.row_dots(t, act, chunk, drop_last_block)


def check_layer(tap, kc_raw, vc_raw, model, l, pos, form, ctx, twin=None, token=None):
    """every launch of the tapped layer (and the classifier) of a step over Q5_0 / Q5_1 layers -> {launch: Result}"""
    assert model.wtype in Q5, model.wtype
    with q5_rows():
        return R.check_layer(tap, kc_raw, vc_raw, model, l, pos, form, ctx, twin, token)


def shrink_residual(model, log2=7):
    """fused_step_ref.shrink_residual for the two formats: d (Q5_1: d and m) of token_embd, attn_output and ffn_down times 2^-log2;
    tensors of another format (a classifier that is also the embedding's twin) go through fused_step_ref's own"""
    f = np.float16(2.0 ** -log2)
    rest = {}
    for name, t in model.tensors.items():
        if not (name == "token_embd.weight" or name.endswith("attn_output.weight") or name.endswith("ffn_down.weight")):
            continue
        if t.typ not in Q5:
            rest[name] = t
            continue
        blk = t.data.reshape(-1, synth.BLOCK_BYTES[t.typ])
        for lo in ((0,) if t.typ == synth.Q5_0 else (0, 2)):
            d = blk[:, lo:lo + 2].copy().view(np.float16)
            blk[:, lo:lo + 2] = (d * f).astype(np.float16).view(np.uint8)
    if rest:
        import types
        _R_shrink(types.SimpleNamespace(tensors=rest), log2)
    return model


def flip_signs(model, seed=5):
    """block scales d of either sign on every Q5_0 / Q5_1 tensor (Q5_1's m stays as it is: d and m no longer tied)"""
    rng = np.random.default_rng(seed)
    for t in model.tensors.values():
        if t.typ in Q5:
            blk = t.data.reshape(-1, synth.BLOCK_BYTES[t.typ])
            blk[:, 1] ^= (rng.integers(0, 2, size=blk.shape[0], dtype=np.uint8) << 7)
    return model


failures = R.failures
