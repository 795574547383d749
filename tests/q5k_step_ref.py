"""The launches of the fast K-quant decode step over a Q5_K BODY (enqueue_segment_k<Q5_K>: k_qkv<Q5_K>, attention, k_gemv_res_nq<Q5_K,
SPLIT, QIN> for wo, k_gateup_k_lds<.., Q5>, the same for ffn_down, the classifier) restated in float64 for the tap recorder --
tests/fused_step_ref.py's K forms (check_layer_k and everything under it: the Q8_K interval check with its EXCUSED_CAP, the norm
intervals, the attention and classifier checks, the Q6_K rows of a *_K_M layer, none of which depend on the body's format) with the
one thing a Q5_K body changes in a launch: the row dot.

  Q5_K block, in the reference's field order (buf_q5_k.rs:13-21): qs[128] | qh[32] | scales[12] | d f16 | dmin f16 = 176 bytes.  The
      6-bit scale / minimum fields are Q4_K's (util.rs:19-27).  Element 64 p + 32 g + l of a super-block (pair p < 4, g = 0: the low
      nibbles, g = 1: the high ones, l < 32) has the level (nibble g of qs[32 p + l]) + 16 * (bit 2 p + g of qh[l]), 0 .. 31, the
      scale sc[2 p + g] and the minimum mn[2 p + g] (buf_q5_k.rs:24-63).
  Q5_K row dot (q5k_term, gemv_core.hpp): a lane's PIECE (pair p, half h) is the 16 bytes qs[32 p + 16 h .. + 16] with the fifth bits
      of qh[16 h .. + 16] -- the elements 64 p + 16 h + i (low nibbles) and 64 p + 32 + 16 h + i (high), i < 16, against the Q8_K
      quants of the same elements in ELEMENT order (the plane `q`, not the class-major `qp` Q4_K rows read) -- with exact integers
      isum = sc[2p] sum(q5 q8 | low) + sc[2p+1] sum(q5 q8 | high), |isum| <= 2 * 63 * 16 * 31 * 128 < 2^23, and msum = mn[2p] bsum_lo +
      mn[2p+1] bsum_hi < 2^19 (bsums entries 4 p + h and 4 p + 2 + h of the plane the launch read), and the f32 term
      f32(d_w d8) isum - f32(dmin_w d8) msum: Q4_K's own function, FIVE roundings (the two scale products, the two products with the
      integers -- whose conversions are exact below 2^24 --, the subtraction; the build has -ffp-contract=off).  With A = |d_w d8 isum| +
      |dmin_w d8 msum| the term is off by at most (2 U |dd isum| + 2 U |dmin msum|)(1 + U) + U |term| <= 3 U A (1 + 2 U).  The 8 nsb
      terms of a row are added in some order -- a lane's pieces in ascending order, the 64 lanes through a tree, the leading pieces of
      the prologue forms first --, n - 1 additions, each off by at most U times a partial sum of |terms| <= U sum A (1 + 3 U):
          |f32 - exact| <= (n_terms + C_K) U sum A,   C_K = 3
      three for the term, minus one, plus one for every second-order term (n_terms^2 U^2 < 0.02 U for the longest row here, 448
      pieces): fused_step_ref's Q4_K derivation word for word, because the f32 part IS the same code; only the integers differ.

check_layer swaps this module's weight_rows / _chunk_dots in for fused_step_ref's while it runs (they dispatch back for every other
format), so every K check reads Q5_K rows without a copy of its own."""
import contextlib

import numpy as np

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests.fused_step_ref import C_K, EXCUSED_CAP, U, _u16, f16v  # noqa: F401

WRONG = ("fifth_bit_dropped", "fifth_bits_swapped", "qh_wrong_pair", "scale_neighbour", "min_neighbour", "dmin_plus")
_R_weight_rows, _R_chunk_dots = R.weight_rows, R._chunk_dots


def fifth_bits(qh, shift_pair=0, swap=False):
    """qh [.., 32] bytes -> the fifth bit of every element, [.., 256] in element order: bit 2 p + g of qh[l] for element 64 p + 32 g + l.
    shift_pair / swap: the wrong kernels of the checker's own tests"""
    out = np.empty(qh.shape[:-1] + (4, 2, 32), dtype=np.int64)
    for p in range(4):
        for g in range(2):
            out[..., p, g, :] = (qh >> (2 * ((p + shift_pair) % 4) + (1 - g if swap else g))) & 1
    return out.reshape(qh.shape[:-1] + (256,))


def weight_rows(t, r0, r1):
    """fused_step_ref.weight_rows with Q5_K: d, dmin, sc, mn as Q4_K's; nib (the 4-bit part) and qh kept beside q = nib + 16 * bit"""
    if t.typ != synth.Q5_K:
        return _R_weight_rows(t, r0, r1)
    rows, k = t.shape
    nb = k // 256
    b = np.ascontiguousarray(t.data).view(np.uint8).reshape(rows, nb, 176)[r0:r1]
    s12 = b[:, :, 160:172].astype(np.int64)
    sc, mn = np.empty(b.shape[:2] + (8,)), np.empty(b.shape[:2] + (8,))
    for j in range(4):
        sc[:, :, j], mn[:, :, j] = s12[:, :, j] & 63, s12[:, :, j + 4] & 63
        sc[:, :, j + 4] = (s12[:, :, j + 8] & 0xF) | ((s12[:, :, j] >> 6) << 4)
        mn[:, :, j + 4] = (s12[:, :, j + 8] >> 4) | ((s12[:, :, j + 4] >> 6) << 4)
    qs = b[:, :, 0:128].reshape(b.shape[0], b.shape[1], 4, 32)
    nib = np.stack([qs & 0x0F, qs >> 4], axis=3).reshape(b.shape[0], b.shape[1], 256).astype(np.float64)  # pair p: 32 low nibbles, 32 high
    qh = b[:, :, 128:160].astype(np.int64)
    return {"typ": t.typ, "d": f16v(_u16(b[:, :, 172:174])), "dmin": f16v(_u16(b[:, :, 174:176])), "sc": sc, "mn": mn, "nib": nib, "qh": qh,
            "q": nib + 16.0 * fifth_bits(qh)}


def k_values(w):
    """the dequantized elements of Q5_K rows, f64 [rows, nsb * 256]: Q4_K's expression on the 5-bit levels"""
    return R.k_values(dict(w, typ=synth.Q4_K))


def k_pieces(w, act, wrong=None):
    """Q5_K weight rows against one row's Q8_K blocks: per piece (pair p, half h) of every row the exact term and the magnitude A its
    roundings act on -> (terms, A), each [rows, nsb, 8] (piece j = 2 p + h).  wrong: a kernel that is subtly wrong in the named way"""
    assert w["typ"] == synth.Q5_K and (wrong is None or wrong in WRONG), wrong
    r, nsb = w["d"].shape
    d8, bs = act["d"], act["bsums"].astype(np.float64)
    assert d8.size == nsb, (d8.size, nsb)
    q = w["q"]
    if wrong == "fifth_bit_dropped":
        q = w["nib"]
    elif wrong == "fifth_bits_swapped":
        q = w["nib"] + 16.0 * fifth_bits(w["qh"], swap=True)
    elif wrong == "qh_wrong_pair":
        q = w["nib"] + 16.0 * fifth_bits(w["qh"], shift_pair=1)
    x = act["q"].astype(np.float64).reshape(nsb, 4, 2, 2, 16)  # ELEMENT order: [pair p, nibble half g, piece half h, byte i]
    S = np.einsum("rspghi,spghi->rspgh", q.reshape(r, nsb, 4, 2, 2, 16), x)
    sc, mn = w["sc"].copy(), w["mn"].copy()
    if wrong == "scale_neighbour":
        sc[:, 0, 2] = w["sc"][:, 0, 3]
    if wrong == "min_neighbour":
        mn[:, 0, 2] = w["mn"][:, 0, 3]
    isum = (sc.reshape(r, nsb, 4, 2)[..., None] * S).sum(axis=3)                              # [r, nsb, p, h]
    msum = (mn.reshape(r, nsb, 4, 2)[..., None] * bs.reshape(nsb, 4, 2, 2)[None]).sum(axis=3)  # entries 4 p + 2 g + h
    assert np.max(np.abs(isum)) < 2 ** 23 and np.max(np.abs(msum)) < 2 ** 19
    a = (w["d"] * d8[None])[:, :, None, None] * isum
    b = (w["dmin"] * d8[None])[:, :, None, None] * msum
    terms = a - b
    if wrong == "dmin_plus":
        terms[:, 0, 1, 0] = (a + b)[:, 0, 1, 0]
    return terms.reshape(r, nsb, 8), (np.abs(a) + np.abs(b)).reshape(r, nsb, 8)


def _chunk_dots(w, typ, act, k, drop_last_block, wrong=None):
    if typ != synth.Q5_K:
        return _R_chunk_dots(w, typ, act, k, drop_last_block, wrong)
    assert act["qt"] == o.Q8_K
    terms, A = k_pieces(w, act, wrong)
    if drop_last_block:
        terms = terms[:, :-1]
    return terms.sum(axis=(1, 2)), (A.shape[1] * 8 + C_K) * U * A.sum(axis=(1, 2))


@contextlib.contextmanager
def q5k_rows():
    """fused_step_ref's row dots read Q5_K rows inside this block"""
    saved = R.weight_rows, R._chunk_dots
    R.weight_rows, R._chunk_dots = weight_rows, _chunk_dots
    try:
        yield
    finally:
        R.weight_rows, R._chunk_dots = saved


def row_dots(t, act, chunk=256, drop_last_block=False, wrong=None):
    with q5k_rows():
        return R.row_dots(t, act, chunk, drop_last_block, wrong)


def check_layer(tap, kc_raw, vc_raw, model, l, pos, form, ctx, twin=None, token=None):
    """every launch of the tapped layer (and the classifier) of a step over a Q5_K body -> {launch: Result}"""
    assert model.wtype == synth.Q5_K and tap["plan"]["path"] == 2, (model.wtype, tap["plan"])
    with q5k_rows():
        return R.check_layer_k(tap, kc_raw, vc_raw, model, l, pos, form, ctx, twin, token)


def shrink_residual(model, log2=9):
    """fused_step_ref.shrink_residual for a Q5_K / Q5_K_M model: every block scale of the matrices that write the residual stream (the
    embedding, attn_output, ffn_down) times 2^-log2 -- Q5_K's d and dmin sit at bytes 172 / 174 of the block, Q6_K's d at 208"""
    for name, t in model.tensors.items():
        if not (name == "token_embd.weight" or name.endswith("attn_output.weight") or name.endswith("ffn_down.weight")):
            continue
        assert t.typ in (synth.Q5_K, synth.Q6_K), name
        blk = t.data.reshape(-1, synth.BLOCK_BYTES[t.typ])
        for lo in {synth.Q5_K: (172, 174), synth.Q6_K: (208,)}[t.typ]:
            bits = np.ascontiguousarray(blk[:, lo:lo + 2]).view(np.uint16).reshape(-1)
            v = (f16v(bits) * 2.0 ** -log2).astype(np.float16)
            blk[:, lo:lo + 2] = v.view(np.uint8).reshape(-1, 2)
    return model


def flip_signs(model, seed=5):
    """block scales of either sign: the sign bits of Q5_K's d / dmin (bytes 173 / 175) and of Q6_K's d (209)"""
    rng = np.random.default_rng(seed)
    for t in model.tensors.values():
        at = {synth.Q5_K: (173, 175), synth.Q6_K: (209,)}.get(t.typ, ())
        blk = t.data.reshape(-1, synth.BLOCK_BYTES[t.typ]) if at else None
        for byte in at:
            blk[:, byte] ^= (rng.integers(0, 2, size=blk.shape[0], dtype=np.uint8) << 7)
    return model


failures = R.failures
