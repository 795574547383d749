"""The launches of the fast K-quant decode step over a Q2_K BODY (enqueue_segment_k<Q2_K>: k_qkv<Q2_K>, attention, k_gemv_res_nq<F,
SPLIT, QIN> for wo with F the tensor's own format, k_gateup_k_lds<.., Q2_K>, the same for ffn_down, the classifier) restated in
float64 for the tap recorder.  The body is the Q2_K recipe family: attn_q, attn_k, ffn_gate and ffn_up are Q2_K, attn_v, attn_output
and ffn_down each Q2_K, Q3_K or Q4_K (plain Q2_K, the Q2_K / Q2_K_S recipes), the classifier any Q8_K-rhs format.  fused_step_ref's K
forms read Q4_K and Q6_K rows, q5k_step_ref's wrappers add Q5_K rows, q3k_step_ref's Q3_K rows; this module adds Q2_K rows ON TOP of
those wrappers (its weight_rows / _chunk_dots dispatch back to q3k_step_ref's for every other format, which dispatch on), so a
recipe layer's Q3_K and Q4_K rows are read by the same check.  Nothing else in check_layer_k depends on the body's format.

  Q2_K block (buf_q2_k.rs:19-30): scales[16] | qs[64] | d f16 | dmin f16 = 84 bytes.  Element 128 half + 32 s + l of a super-block
      (half < 2, field s < 4, l < 32) has the level (qs[32 half + l] >> 2 s) & 3, i.e. 0 .. 3, and the scale group g = 8 half + 2 s +
      l / 16 (buf_q2_k.rs:44-67); its value is d (scales[g] & 15) level - dmin (scales[g] >> 4).
  Q2_K row dot (q2k_terms = PieceQ2_K::term, gemv_core.hpp): a lane's PIECE (half, h) is the 16 bytes qs[32 half + 16 h .. + 16]; its
      field s is group g = 8 half + 2 s + h.  Per group the exact integer G_g = sum(q2 q8) (|G_g| <= 16 * 3 * 128 < 2^13); the four
      pieces of a super-block add across the quad
          isum = sum_g (scales[g] & 15) G_g   (|isum| <= 16 * 15 * 2^13 < 2^21),
          summs = sum_g bsums[g] (scales[g] >> 4)   (|summs| <= 16 * 2^11 * 15 < 2^19):
      exact integers whose conversions to f32 are exact.  Then ONE f32 expression per SUPER-BLOCK,
          t = (d8 * f32(d)) * (float)isum - (d8 * f32(dmin)) * (float)summs:
      f32(d), f32(dmin) are exact (f16s); each of the two scale products rounds once, each product with its integer once, the
      subtraction once.  With a = d8 d isum, b = d8 dmin summs and A = |a| + |b| (>= |t|): the two halves are off by at most
      2 U |a| (1 + U) and 2 U |b| (1 + U), the difference by U |t| more -- the term by at most 3 U A and second-order terms.  The nsb
      terms of a row (quad lanes 1 .. 3 add +0.0, which changes no bit) are added in some order -- a lane's in ascending order, the
      lanes through a tree, the leading pieces of the prologue forms first --, nsb - 1 additions, each off by at most U times a partial
      sum of |terms| <= sum A.
  The reference's own order (buf_q2_k.rs:216-258) is the SAME expression per super-block (summs and isum as integers, dall * isum as
      f32 - dmin * summs as f32), added super-block after super-block: one of the orders above.  So
          |f32 - exact| <= (n_terms + C_Q2K) U sum A,   n_terms = nsb,   C_Q2K = 3
      three for the term, minus one, plus one for every second-order term (nsb^2 U^2 < 2e-4 U for the longest row here, 56
      super-blocks).  Order-free, so it covers the prologue-first add order of wo, ffn_down and gate | up too.  A is taken from the
      two halves, not from |t|: a block whose d isum and dmin summs nearly cancel keeps the roundings of both.

What this module also holds is the list of subtly WRONG kernels the Q2_K body loader could be (the checker's own tests: every one must
land outside the bound)."""
import contextlib

import numpy as np

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests import q3k_step_ref as Q3
from tests.fused_step_ref import EXCUSED_CAP, U, _u16, f16v  # noqa: F401

C_Q2K = 3
# nibbles_swapped: scale and min nibbles exchanged; min_added: + dmin summs; d_dmin_swapped: the halves of the (d, dmin) record
# exchanged; field_half_swapped: field s and half-piece h exchanged in the group index (g = 8 half + 2 h + s for s < 2: the
# quants and the bsum of another group against the field's own scale byte); bsum_neighbour: bsums of group g + 1; mask_0f: quants masked with 0x0F0F0F0F
# (fields s and s + 1 together); min_dropped_h1: no min term on the h = 1 pieces (what a lane that never received the scale bytes does
# to summs); scale_twin_half: the scale bytes of the other half (the h = 0 lane of the other pair handing its bytes over)
WRONG = ("nibbles_swapped", "min_added", "d_dmin_swapped", "field_half_swapped", "bsum_neighbour", "mask_0f", "min_dropped_h1",
         "scale_twin_half")
FAMILY = (synth.Q2_K, synth.Q3_K, synth.Q4_K)  # what attn_v / attn_output / ffn_down of the family may be


def group_of(half, s, h, wrong=None):
    """the scale group of field s of piece (half, h); wrong = field_half_swapped: s and h exchanged where both are bits (s < 2)"""
    if wrong == "field_half_swapped" and s < 2:
        s, h = h, s
    return 8 * half + 2 * s + h


def weight_rows(t, r0, r1):
    """q3k_step_ref.weight_rows (Q3_K, and the formats behind it) with Q2_K from the raw 84-byte block: d, dmin, the raw 2-bit plane
    qs [.., half, l] (bytes), the sixteen scale bytes, and what they make -- lv (levels 0 .. 3 in element order), sc (scales & 15), mn
    (scales >> 4)"""
    if t.typ != synth.Q2_K:
        return Q3.weight_rows(t, r0, r1)
    rows, k = t.shape
    b = np.ascontiguousarray(t.data).view(np.uint8).reshape(rows, k // 256, 84)[r0:r1]
    qs = b[:, :, 16:80].astype(np.int64).reshape(b.shape[0], b.shape[1], 2, 32)
    s16 = b[:, :, 0:16].astype(np.int64)
    return {"typ": t.typ, "d": f16v(_u16(b[:, :, 80:82])), "dmin": f16v(_u16(b[:, :, 82:84])), "qs": qs, "s16": s16,
            "lv": levels(qs).astype(np.float64), "sc": (s16 & 15).astype(np.float64), "mn": (s16 >> 4).astype(np.float64)}


def levels(qs, wrong=None):
    """the levels in element order, [.., 256], from the byte plane qs [.., 2, 32] (half, l): (qs >> 2 s) & 3 for element 128 half +
    32 s + l.  wrong = mask_0f: the mask of a 4-bit format, (qs >> 2 s) & 15"""
    mask = 15 if wrong == "mask_0f" else 3
    out = np.stack([(qs >> (2 * s)) & mask for s in range(4)], axis=-2)  # [.., half, s, l]
    return out.reshape(qs.shape[:-2] + (256,))


def k_values(w):
    """the dequantized elements of Q2_K rows, f64 [rows, nsb * 256] (16 groups of 16 elements: element order IS group order)"""
    r, nsb = w["d"].shape
    lv = w["lv"].reshape(r, nsb, 16, 16)
    return ((w["d"][:, :, None] * w["sc"])[:, :, :, None] * lv - (w["dmin"][:, :, None] * w["mn"])[:, :, :, None]).reshape(r, -1)


def k_terms(w, act, wrong=None):
    """Q2_K weight rows against one row's Q8_K blocks: per SUPER-BLOCK of every row the exact term d8 (d isum - dmin summs) and the
    magnitude A its roundings act on -> (terms, A), each [rows, nsb].  wrong: a kernel that is subtly wrong in the named way"""
    assert w["typ"] == synth.Q2_K and (wrong is None or wrong in WRONG), wrong
    r, nsb = w["d"].shape
    d8, bs = act["d"], act["bsums"].astype(np.float64)
    assert d8.size == nsb and bs.shape == (nsb, 16), (d8.size, nsb, bs.shape)
    lv = levels(w["qs"], wrong).astype(np.float64)
    x = act["q"].astype(np.float64).reshape(nsb, 16, 16)  # ELEMENT order: [scale group g, i]
    # the group whose quants and bsum the piece (half, h) reads for its field s, by the group the field BELONGS to (element order)
    at = np.array([group_of(g // 8, (g % 8) // 2, g % 2, wrong) for g in range(16)])
    x, bs = x[:, at, :], bs[:, at]
    G = np.einsum("rsgi,sgi->rsg", lv.reshape(r, nsb, 16, 16), x)
    assert np.max(np.abs(G)) < 2 ** 13 * (8 if wrong else 1)
    s16 = w["s16"]
    if wrong == "scale_twin_half":
        s16 = np.roll(s16, 8, axis=-1)
    sc, mn = (s16 & 15).astype(np.float64), (s16 >> 4).astype(np.float64)
    if wrong == "nibbles_swapped":
        sc, mn = mn, sc
    if wrong == "min_dropped_h1":
        mn = mn * (1 - np.arange(16) % 2)[None, None, :]
    off = np.roll(bs, -1, axis=1) if wrong == "bsum_neighbour" else bs  # (the entry of group g + 1, as an off-by-one in the index would take)
    isum = (sc * G).sum(axis=2)
    summs = (mn * off[None]).sum(axis=2)
    assert wrong or (np.max(np.abs(isum)) < 2 ** 24 and np.max(np.abs(summs)) < 2 ** 24)
    d, dmin = (w["dmin"], w["d"]) if wrong == "d_dmin_swapped" else (w["d"], w["dmin"])
    a, b = d * d8[None] * isum, dmin * d8[None] * summs
    return (a + b if wrong == "min_added" else a - b), np.abs(a) + np.abs(b)


def _chunk_dots(w, typ, act, k, drop_last_block, wrong=None):
    if typ != synth.Q2_K:
        return Q3._chunk_dots(w, typ, act, k, drop_last_block, wrong)
    assert act["qt"] == o.Q8_K
    terms, A = k_terms(w, act, wrong)
    if drop_last_block:
        terms = terms[:, :-1]
    return terms.sum(axis=1), (A.shape[1] + C_Q2K) * U * A.sum(axis=1)


@contextlib.contextmanager
def q2k_rows():
    """fused_step_ref's row dots read Q2_K rows (and, through the wrappers behind, Q3_K and Q5_K rows) inside this block"""
    saved = R.weight_rows, R._chunk_dots
    R.weight_rows, R._chunk_dots = weight_rows, _chunk_dots
    try:
        yield
    finally:
        R.weight_rows, R._chunk_dots = saved


def row_dots(t, act, chunk=256, drop_last_block=False, wrong=None):
    with q2k_rows():
        return R.row_dots(t, act, chunk, drop_last_block, wrong)


def check_layer(tap, kc_raw, vc_raw, model, l, pos, form, ctx, twin=None, token=None):
    """every launch of the tapped layer (and the classifier) of a step over a Q2_K body -> {launch: Result}"""
    assert model.wtype == synth.Q2_K and tap["plan"]["path"] == 2, (model.wtype, tap["plan"])
    for n in ("attn_q", "attn_k", "ffn_gate", "ffn_up"):
        assert model.tensors[f"blk.{l}.{n}.weight"].typ == synth.Q2_K, n
    for n in ("attn_v", "attn_output", "ffn_down"):
        assert model.tensors[f"blk.{l}.{n}.weight"].typ in FAMILY, n
    with q2k_rows():
        return R.check_layer_k(tap, kc_raw, vc_raw, model, l, pos, form, ctx, twin, token)


# byte offsets of the f16 block scales (d; d | dmin) of the formats a member of the family holds in the matrices that write the residual
_SCALES_AT = {synth.Q2_K: (80, 82), synth.Q3_K: (108,), synth.Q4_K: (0, 2), synth.Q6_K: (208,)}


def shrink_residual(model, log2=9):
    """fused_step_ref.shrink_residual for a member of the Q2_K family: every block scale of the matrices that write the residual stream
    (the embedding, attn_output, ffn_down) times 2^-log2 -- Q2_K's d and dmin sit at bytes 80 / 82 of the block"""
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
    """block scales of either sign: the sign bit of every f16 block scale (Q2_K's d and dmin: bytes 81 and 83, each its own draw) on
    every K-quant tensor"""
    rng = np.random.default_rng(seed)
    for t in model.tensors.values():
        at = _SCALES_AT.get(t.typ, ())
        blk = t.data.reshape(-1, synth.BLOCK_BYTES[t.typ]) if at else None
        for lo in at:
            blk[:, lo + 1] ^= (rng.integers(0, 2, size=blk.shape[0], dtype=np.uint8) << 7)
    return model


failures = R.failures
