"""ONE TABLE OF WEIGHT FORMATS for the float64 checkers (tests/fused_step_ref.py: the decode step; tests/prefill_pass_ref.py: the row
dots of the prompt pass).  FORMATS is keyed by the synth type; a row states once, per format,

  the block layout   bytes and elements of a block, the byte offsets of its f16 scale fields (shrink_residual / flip_signs), the rhs
                     quantization its rows are read against, the GGMLType attribute name, whether it is a 256-element format;
  the row reader     rows(b, wrong): the blocks [rows, nb, block bytes] -> exact integer / f64 fields, the raw fields beside them.  The
                     subtly wrong LOADERS of Q5_0 / Q5_1 act here, so every reader takes `wrong`;
  the row-dot rule   dots(w, act, wrong) -> (terms, A, cap): the exact terms of every row against one row's activation blocks, the
                     magnitudes A the roundings of the kernel's f32 expression act on (None: the terms' own), an upper limit of the bound
                     (Q4_1 / Q5_1) -- and the constant C of its bound (n_terms + C) U sum A, which chunk_dots, the ONE tail, forms;
  the wrong kernels  the names a checker's own tests hand to `wrong`: every one must land outside the bound;
  the f16 GEMM       f16w: k_gemm_f16w's form for the format (gemm_f16w.hip) restated in ELEMENT order -- operands(blk, nr, nb, wrong) ->
                     (A' f16 as float64, W exact float64, the bound of A' against W) --, blocks whose A' are small integers (the exact
                     tier), blocks that hit every scale code (where the format has codes), and the names of its own wrong restatements.
                     B' is permuted by the kernel's k-slot order within one block of the format (32 or 256 elements): block_elems is the
                     group size tests/f16w_gemm_ref.b_groups sorts.

U = 2^-24, the unit roundoff of f32 (the f16 GEMM's restatements: U_F16 = 2^-11).  The derivation of each bound stands in the docstring of its rule; those of Q4_0 / Q8_0 / Q4_1 /
Q4_K / Q6_K in the module docstring of tests/fused_step_ref.py, where they were first written down."""
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from crabml_amd import synth
from oracle import oracle as o
from tests.helpers import GEMV_REL

U = 2.0 ** -24
C_DOT = 3
C_K = 3      # K-quant row dots over pieces: see the module docstring of tests/fused_step_ref.py
C_Q3K = 9
C_Q2K = 3


def f16v(bits):
    return np.ascontiguousarray(bits).view(np.float16).astype(np.float64)


def _u16(b):
    return np.ascontiguousarray(b).view(np.uint16)[..., 0]


# ---- Q4_0 / Q8_0 / Q4_1 (buf_q4_0.rs, buf_q8_0.rs, buf_q4_1.rs) ----
def q8_0_rows(b, wrong=None):
    return {"d": f16v(_u16(b[:, :, 0:2])), "q": np.ascontiguousarray(b[:, :, 2:]).view(np.int8).astype(np.float64)}


def _nibbles(qs):
    return np.concatenate([qs & 0x0F, qs >> 4], axis=2).astype(np.float64)  # element j < 16: low nibble of byte j; j >= 16: high nibble of byte j - 16


def q4_0_rows(b, wrong=None):
    return {"d": f16v(_u16(b[:, :, 0:2])), "q": _nibbles(b[:, :, 2:]) - 8.0}


def q4_1_rows(b, wrong=None):
    return {"d": f16v(_u16(b[:, :, 0:2])), "q": _nibbles(b[:, :, 4:]), "m": f16v(_u16(b[:, :, 2:4]))}


def block_dots(w, act, wrong=None):
    """Q4_0 / Q8_0 x Q8_0: products of exact small integers and f16 scales; two roundings per block term, (nb + C_DOT) U sum |t_b|"""
    x = (act["q"] * act["d"][:, None]).reshape(-1)
    nblk = w["d"].shape[1]
    assert x.size == nblk * 32, (x.size, nblk * 32)
    wd = (w["q"] * w["d"][:, :, None]).reshape(w["q"].shape[0], nblk, 32)  # exact in f64
    return np.einsum("rbi,bi->rb", wd, x.reshape(nblk, 32)), None, None


def f16_product_dots(w, act, wrong=None):
    """Q4_1 x Q8_1: the term is f16(d_w d_x) * sumi + f16(m s), the f16 products part of the expression and restated exactly; two
    roundings on |f16(d_w d_x) sumi| + |f16(m s)|, never more than 8 GEMV_REL sum_i |w_i x_i| (the two parts of a term cancel)"""
    assert act["qt"] == o.Q8_1
    xq = act["q"].astype(np.float64)
    xd = (act["q"] * act["d"][:, None]).astype(np.float64)
    sumi = np.einsum("rbi,bi->rb", w["q"], xq)
    P = (w["d"] * act["d"][None, :]).astype(np.float16).astype(np.float64)  # f16 products, rounded once (the exact product fits f64)
    M = (w["m"] * act["s"][None, :]).astype(np.float16).astype(np.float64)
    deq = np.einsum("rbi,bi->r", np.abs(w["q"] * w["d"][:, :, None] + w["m"][:, :, None]), np.abs(xd))
    return P * sumi + M, np.abs(P * sumi) + np.abs(M), 8 * GEMV_REL * deq


# ---- Q5_0 / Q5_1 ----
# a loader that ...: drops the fifth bits; takes the high half's bits for the low half and the other way round; takes bit i of qh for
# element i's NEIGHBOUR in the dword (the bits of a nibble group reversed); forgets the -16 (Q5_0) / the minimum (Q5_1); reads the
# scale of the next block (a third plane addressed one unit off); reads qh of the next block
WRONG_Q5_01 = ("qh_bits_dropped", "qh_halves_swapped", "qh_bits_reversed_in_group", "offset_dropped", "scale_neighbour", "qh_neighbour")


def q5_levels(qs, qh, wrong=None):
    """the 32 levels 0 .. 31 of every Q5_0 / Q5_1 block in element order, [.., 32], from qs [.., 16] and qh [..] (the u32)"""
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


def _q5_rows(b, h, wrong):
    qh = np.ascontiguousarray(b[:, :, h:h + 4]).view("<u4")[..., 0]
    d = f16v(_u16(b[:, :, 0:2]))
    if wrong == "scale_neighbour":
        d = np.roll(d, -1, axis=1)
    return {"d": d, "qs": b[:, :, h + 4:], "qh": qh}, q5_levels(b[:, :, h + 4:], qh, wrong).astype(np.float64)


def q5_0_rows(b, wrong=None):
    """Q5_0 block (buf_q5_0.rs:13-19): d f16 | qh u32 | qs[16] = 22 bytes.  Element i < 16 has the level (qs[i] & 15) | bit i of qh << 4,
    element 16 + i the level (qs[i] >> 4) | bit 16 + i of qh << 4; its value is (level - 16) * d (buf_q5_0.rs:22-37).  q = level - 16"""
    w, lv = _q5_rows(b, 2, wrong)
    w["q"] = lv - (0.0 if wrong == "offset_dropped" else 16.0)
    return w


def q5_1_rows(b, wrong=None):
    """Q5_1 block (buf_q5_1.rs:10-17): d f16 | m f16 | qh u32 | qs[16] = 24 bytes, Q5_0's levels, value level * d + m.  q = level"""
    w, lv = _q5_rows(b, 4, wrong)
    w["q"] = lv
    m = f16v(_u16(b[:, :, 2:4]))
    w["m"] = m * 0.0 if wrong == "offset_dropped" else m
    return w


def q5_0_dots(w, act, wrong=None):
    """Q5_0 row dot (BlockFmt<Q5_0>::term, gemv_core.hpp; the reference: buf_q5_0.rs:158): sumi = sum (level - 16) * q8 is an exact
    integer, |sumi| <= 32 * 16 * 127 < 2^24, so (float)sumi is exact; the term is ((float)sumi * d_w) * d_x, TWO roundings, and the nb
    terms are added in some order: the Q4_0 derivation stands word for word, |f32 - exact| <= (nb + C_DOT) U sum_b |t_b|.  With
    w["q"] = level - 16 and w["d"] the f16 scale, Q4_0's rule computes exactly this."""
    assert act["qt"] == o.Q8_0 and np.abs(np.einsum("rbi,bi->rb", w["q"], act["q"].astype(np.float64))).max() <= 32 * 16 * 127
    return block_dots(w, act)


def q5_1_dots(w, act, wrong=None):
    """Q5_1 row dot (BlockFmt<Q5_1>::term; buf_q5_1.rs:156): f16(d_w d_x) * (float)sumi + f16(m s), sumi = sum level * q8 exact (|sumi| <=
    32 * 31 * 128 < 2^24), the two f16 products part of the expression and restated exactly (the exact product of two f16 values
    fits float64, rounded once to f16): Q4_1's bound, (nb + C_DOT) U sum_b (|f16(d_w d_x) sumi| + |f16(m s)|), never more than
    8 GEMV_REL sum_i |w_i x_i|.  Q4_1's rule with w["q"] = level computes exactly this."""
    return f16_product_dots(w, act)


# ---- Q4_K / Q5_K ----
def _scale_min_k4(s12):
    """the eight 6-bit scales and minimums of a Q4_K / Q5_K super-block from scales[12] (util.rs:19-27)"""
    sc, mn = np.empty(s12.shape[:2] + (8,)), np.empty(s12.shape[:2] + (8,))
    for j in range(4):
        sc[:, :, j], mn[:, :, j] = s12[:, :, j] & 63, s12[:, :, j + 4] & 63
        sc[:, :, j + 4] = (s12[:, :, j + 8] & 0xF) | ((s12[:, :, j] >> 6) << 4)
        mn[:, :, j + 4] = (s12[:, :, j + 8] >> 4) | ((s12[:, :, j + 4] >> 6) << 4)
    return sc, mn


def q4_k_rows(b, wrong=None):
    """d f16 | dmin f16 | scales[12] | qs[128] (buf_q4_k.rs:13-19); the 6-bit fields: util.rs:19-27; order: buf_q4_k.rs:24-47"""
    sc, mn = _scale_min_k4(b[:, :, 4:16].astype(np.int64))
    qs = b[:, :, 16:144].reshape(b.shape[0], b.shape[1], 4, 32)
    q = np.stack([qs & 0x0F, qs >> 4], axis=3).reshape(b.shape[0], b.shape[1], 256).astype(np.float64)  # pair p: 32 low nibbles, 32 high
    return {"d": f16v(_u16(b[:, :, 0:2])), "dmin": f16v(_u16(b[:, :, 2:4])), "sc": sc, "mn": mn, "q": q}


def q4_k_values(w):
    """the dequantized elements of Q4_K (and, on the 5-bit levels, Q5_K) rows, f64 [rows, nsb * 256]"""
    r, nsb = w["d"].shape
    v = (w["d"][:, :, None] * w["sc"])[:, :, :, None] * w["q"].reshape(r, nsb, 8, 32) - (w["dmin"][:, :, None] * w["mn"])[:, :, :, None]
    return v.reshape(r, -1)


def _scales_mins(w, wrong):
    sc, mn = w["sc"].copy(), w["mn"].copy()
    if wrong == "scale_neighbour":
        sc[:, 0, 2] = w["sc"][:, 0, 3]
    if wrong == "min_neighbour":
        mn[:, 0, 2] = w["mn"][:, 0, 3]
    return sc, mn


def q4_k_dots(w, act, wrong=None):
    """Q4_K rows against one row's Q8_K blocks: per piece of every row (the kernels' 16-byte unit, 8 per super-block) the exact term and
    the magnitude A its roundings act on, each [rows, nsb, 8] (the derivation: the module docstring of tests/fused_step_ref.py)"""
    assert act["qt"] == o.Q8_K
    r, nsb = w["d"].shape
    d8, bs = act["d"], act["bsums"].astype(np.float64)
    assert d8.size == nsb, (d8.size, nsb)
    # a lane's piece (pair p, class half h) takes, of either 32-group of the pair, the elements e with e % 8 in 4 h .. 4 h + 3 (dwords
    # 4 h .. of the class-major planes: q4k_loadx / q4k_ints): [32-group g, e / 8, class half h, class within the half]
    x = act.get("qp_q", act["q"]).astype(np.float64).reshape(nsb, 8, 4, 2, 4)
    S = np.einsum("rsgahi,sgahi->rsgh", w["q"].reshape(r, nsb, 8, 4, 2, 4), x)
    sc, mn = _scales_mins(w, wrong)
    T = sc[:, :, :, None] * S
    # (the minimum term only needs every bsums entry once per super-block: piece (p, h) takes entries 4 p + h and 4 p + 2 + h, the
    # CONTIGUOUS halves h of its two groups, as q4k_loadx does)
    M = mn[:, :, :, None] * bs.reshape(nsb, 8, 2)[None]
    isum, msum = T[:, :, 0::2] + T[:, :, 1::2], M[:, :, 0::2] + M[:, :, 1::2]  # piece (pair p, half h): groups 2 p and 2 p + 1
    a = (w["d"] * d8[None])[:, :, None, None] * isum
    b = (w["dmin"] * d8[None])[:, :, None, None] * msum
    terms = a - b
    if wrong == "dmin_plus":
        terms[:, 0, 1, 0] = (a + b)[:, 0, 1, 0]
    return terms.reshape(r, nsb, 8), (np.abs(a) + np.abs(b)).reshape(r, nsb, 8), None


WRONG_Q5_K = ("fifth_bit_dropped", "fifth_bits_swapped", "qh_wrong_pair", "scale_neighbour", "min_neighbour", "dmin_plus")


def fifth_bits(qh, shift_pair=0, swap=False):
    """Q5_K's qh [.., 32] bytes -> the fifth bit of every element, [.., 256] in element order: bit 2 p + g of qh[l] for element
    64 p + 32 g + l.  shift_pair / swap: the wrong kernels of the checker's own tests"""
    out = np.empty(qh.shape[:-1] + (4, 2, 32), dtype=np.int64)
    for p in range(4):
        for g in range(2):
            out[..., p, g, :] = (qh >> (2 * ((p + shift_pair) % 4) + (1 - g if swap else g))) & 1
    return out.reshape(qh.shape[:-1] + (256,))


def q5_k_rows(b, wrong=None):
    """Q5_K block, in the reference's field order (buf_q5_k.rs:13-21): qs[128] | qh[32] | scales[12] | d f16 | dmin f16 = 176 bytes.  The
    6-bit scale / minimum fields are Q4_K's (util.rs:19-27).  Element 64 p + 32 g + l of a super-block (pair p < 4, g = 0: the low
    nibbles, g = 1: the high ones, l < 32) has the level (nibble g of qs[32 p + l]) + 16 * (bit 2 p + g of qh[l]), 0 .. 31, the
    scale sc[2 p + g] and the minimum mn[2 p + g] (buf_q5_k.rs:24-63).  d, dmin, sc, mn as Q4_K's; nib (the 4-bit part) and qh kept
    beside q = nib + 16 * bit"""
    sc, mn = _scale_min_k4(b[:, :, 160:172].astype(np.int64))
    qs = b[:, :, 0:128].reshape(b.shape[0], b.shape[1], 4, 32)
    nib = np.stack([qs & 0x0F, qs >> 4], axis=3).reshape(b.shape[0], b.shape[1], 256).astype(np.float64)  # pair p: 32 low nibbles, 32 high
    qh = b[:, :, 128:160].astype(np.int64)
    return {"d": f16v(_u16(b[:, :, 172:174])), "dmin": f16v(_u16(b[:, :, 174:176])), "sc": sc, "mn": mn, "nib": nib, "qh": qh,
            "q": nib + 16.0 * fifth_bits(qh)}


def q5_k_dots(w, act, wrong=None):
    """Q5_K row dot (q5k_term, gemv_core.hpp): a lane's PIECE (pair p, half h) is the 16 bytes qs[32 p + 16 h .. + 16] with the fifth bits
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
    pieces): the Q4_K derivation word for word, because the f32 part IS the same code; only the integers differ.
    -> (terms, A), each [rows, nsb, 8] (piece j = 2 p + h)"""
    assert act["qt"] == o.Q8_K and (wrong is None or wrong in WRONG_Q5_K), wrong
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
    sc, mn = _scales_mins(w, wrong)
    isum = (sc.reshape(r, nsb, 4, 2)[..., None] * S).sum(axis=3)                              # [r, nsb, p, h]
    msum = (mn.reshape(r, nsb, 4, 2)[..., None] * bs.reshape(nsb, 4, 2, 2)[None]).sum(axis=3)  # entries 4 p + 2 g + h
    assert np.max(np.abs(isum)) < 2 ** 23 and np.max(np.abs(msum)) < 2 ** 19
    a = (w["d"] * d8[None])[:, :, None, None] * isum
    b = (w["dmin"] * d8[None])[:, :, None, None] * msum
    terms = a - b
    if wrong == "dmin_plus":
        terms[:, 0, 1, 0] = (a + b)[:, 0, 1, 0]
    return terms.reshape(r, nsb, 8), (np.abs(a) + np.abs(b)).reshape(r, nsb, 8), None


# ---- Q6_K ----
WRONG_Q6_K = ("qh_bits_dropped", "qh_twin_shift", "scales_swapped", "q6_scale_shift", "offset_dropped", "bsum_neighbour", "d_sign_lost")


def q6_levels(lo4, qh, twin=False, drop=False):
    """the 6-bit levels 0 .. 63 in element order, [.., 256], from lo4 [.., 2, 4, 32] (the nibbles, element order) and qh [.., 64]: bits
    2 j, 2 j + 1 of qh[32 h + l] for element 128 h + 32 j + l.  twin: the field of the lane with the other `a` (j ^ 1); drop: none"""
    out = np.empty(lo4.shape, dtype=np.int64)
    for h in range(2):
        for j in range(4):
            hi2 = (qh[..., 32 * h:32 * h + 32] >> (2 * (j ^ 1 if twin else j))) & 3
            out[..., h, j, :] = lo4[..., h, j, :] + (0 if drop else 16 * hi2)
    return out.reshape(lo4.shape[:-3] + (256,))


def q6_k_rows(b, wrong=None):
    """Q6_K block (buf_q6_k.rs:11-18): ql[128] | qh[64] | scales i8[16] | d f16 = 210 bytes.  Element 128 h + 32 j + l of a super-block
    (half h, quarter j < 4, l < 32) has the level (nibble j >> 1 of ql[64 h + 32 (j & 1) + l]) + 16 * (bits 2 j, 2 j + 1 of
    qh[32 h + l]) - 32 and the scale sc[8 h + 2 j + l / 16] (buf_q6_k.rs:21-48; element order of dequantize: buf_q6_k.rs:93-120).
    q6 (the levels - 32), sc and q = q6 * scale in the dequantizer's order, and beside them the raw fields as the kernel's pieces take
    them, lo4 (the nibbles in element order) and qh: the two unpacks must agree"""
    ql, qh = b[:, :, 0:128].astype(np.int64), b[:, :, 128:192].astype(np.int64)
    sc = np.ascontiguousarray(b[:, :, 192:208]).view(np.int8).astype(np.float64)
    q = np.empty(b.shape[:2] + (256,), dtype=np.float64)
    scale = np.empty_like(q)
    for half in range(2):
        lq, hq = ql[:, :, 64 * half:64 * half + 64], qh[:, :, 32 * half:32 * half + 32]
        for j, (lo, sh) in enumerate(((lq[:, :, 0:32] & 0xF, 0), (lq[:, :, 32:64] & 0xF, 2), (lq[:, :, 0:32] >> 4, 4), (lq[:, :, 32:64] >> 4, 6))):
            base = 128 * half + 32 * j
            q[:, :, base:base + 32] = (lo | (((hq >> sh) & 3) << 4)) - 32
            for g in range(2):
                scale[:, :, base + 16 * g:base + 16 * g + 16] = sc[:, :, 8 * half + 2 * j + g][:, :, None]
    w = {"d": f16v(_u16(b[:, :, 208:210])), "q": q * scale, "q6": q, "sc": sc, "qh": qh}
    ql = ql.reshape(b.shape[0], b.shape[1], 2, 2, 32)  # [half h, a, l]
    w["lo4"] = np.stack([ql[:, :, :, 0] & 0xF, ql[:, :, :, 1] & 0xF, ql[:, :, :, 0] >> 4, ql[:, :, :, 1] >> 4], axis=3)  # quarter j = a + 2 * (high nibble)
    assert np.array_equal(q6_levels(w["lo4"], w["qh"]) - 32, w["q6"])
    return w


def q6_k_values(w):
    return (w["q"] * w["d"][:, :, None]).reshape(w["q"].shape[0], -1)


def q6_k_dots(w, act, wrong=None):
    """Q6_K row dot (q6k_term, gemv_core.hpp): a lane's PIECE (h, a, p) is the 16 bytes ql[64 h + 32 a + 16 p .. + 16] with the two-bit
    fields 2 a (low nibbles) and 2 a + 4 (high) of qh[32 h + 16 p .. + 16]: the low nibbles are scale group g = 8 h + 2 a + p, the
    high ones group g + 4.  Exact integers lo = sum(q6 q8 | group g) - 32 bsums[g], hi likewise for g + 4 (|lo|, |hi| <= 16 * 63 *
    128 + 32 * 16 * 128 < 2^18), scaled by the signed byte scales (|sc lo| < 2^25: the conversions to f32 may round), and the f32
    term f32(d_w d8) * (f32(sc_lo lo) + f32(sc_hi hi)).  The derivation in the module docstring of tests/fused_step_ref.py stands word
    for word: three roundings per piece on A = |d_w d8| (|sc_lo lo| + |sc_hi hi|), the 8 nsb terms of a row added in some order --
        |f32 - exact| <= (8 nsb + C_K) U sum A
    order-free, so it covers the prologue-first add order of wo, ffn_down and gate | up too.
    -> (terms, A), each [rows, nsb, 8], per piece (h, a, p) = index 4 h + 2 a + p of every row"""
    assert act["qt"] == o.Q8_K and (wrong is None or wrong in WRONG_Q6_K), wrong
    r, nsb = w["d"].shape
    d8, bs = act["d"], act["bsums"].astype(np.float64)
    assert d8.size == nsb and bs.shape == (nsb, 16), (d8.size, nsb, bs.shape)
    q = q6_levels(w["lo4"], w["qh"], twin=wrong == "qh_twin_shift", drop=wrong == "qh_bits_dropped").astype(np.float64)
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
    return ((dd * (G[:, :, :, 0] + G[:, :, :, 1])).reshape(r, nsb, 8),
            (np.abs(dd) * (np.abs(G[:, :, :, 0]) + np.abs(G[:, :, :, 1]))).reshape(r, nsb, 8), None)


# ---- Q3_K ----
WRONG_Q3_K = ("hmask_dropped", "hmask_other_half", "hmask_twin_piece", "offset_dropped", "scale_high_neighbour", "scale_without_32", "bsum_neighbour")


def q3_levels(q2, hmask, wrong=None):
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


def q3_scales(s12, wrong=None):
    """the sixteen 6-bit scales of a Q3_K super-block minus 32, [.., 16], from scales[12].  wrong: scale_high_neighbour (the high two
    bits from the neighbouring byte of scales[8 .. 11]), scale_without_32"""
    out = np.empty(s12.shape[:-1] + (16,), dtype=np.int64)
    for g in range(16):
        lo = (s12[..., g % 8] >> (4 * (g // 8))) & 0xF
        hi = (s12[..., 8 + ((g % 4) ^ (1 if wrong == "scale_high_neighbour" else 0))] >> (2 * (g // 4))) & 3
        out[..., g] = (lo | (hi << 4)) - (0 if wrong == "scale_without_32" else 32)
    return out


def q3_k_rows(b, wrong=None):
    """Q3_K block (buf_q3_k.rs:19-30): hmask[32] | qs[64] | scales[12] | d f16 = 110 bytes.  Element 128 half + 32 s + l of a super-block
    (half < 2, field s < 4, l < 32) has the level ((qs[32 half + l] >> 2 s) & 3 | bit (4 half + s) of hmask[l] as bit 2) - 4, i.e.
    -4 .. 3, and the scale group g = 8 half + 2 s + l / 16 (buf_q3_k.rs:62-83).  The 6-bit scale of group g (buf_q3_k.rs:44-56): low
    four bits = nibble g / 8 of scales[g % 8], high two bits = bits 2 (g / 4), 2 (g / 4) + 1 of scales[8 + g % 4]; minus 32.
    d, the 2-bit fields q2 [.., half, s, l], hmask, scales[12] and what they make -- lv (levels - 4, element order) and sc (scales - 32)"""
    qs = b[:, :, 32:96].astype(np.int64).reshape(b.shape[0], b.shape[1], 2, 32)
    q2 = np.stack([(qs >> (2 * s)) & 3 for s in range(4)], axis=3)  # [half, s, l]
    hmask, s12 = b[:, :, 0:32].astype(np.int64), b[:, :, 96:108].astype(np.int64)
    return {"d": f16v(_u16(b[:, :, 108:110])), "q2": q2, "hmask": hmask, "s12": s12,
            "lv": (q3_levels(q2, hmask) - 4).astype(np.float64), "sc": q3_scales(s12).astype(np.float64)}


def q3_k_values(w):
    """the dequantized elements of Q3_K rows, f64 [rows, nsb * 256] (16 groups of 16 elements: element order IS group order)"""
    r, nsb = w["d"].shape
    return ((w["d"][:, :, None] * w["sc"])[:, :, :, None] * w["lv"].reshape(r, nsb, 16, 16)).reshape(r, -1)


def q3_k_dots(w, act, wrong=None):
    """Q3_K row dot (q3k_term = PieceQ3_K::term, gemv_core.hpp): a lane's PIECE (half, h) is the 16 bytes qs[32 half + 16 h .. + 16] with
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
    -> (terms, A), each [rows, nsb]: per SUPER-BLOCK of every row the exact term d_w d8 tot"""
    assert act["qt"] == o.Q8_K and (wrong is None or wrong in WRONG_Q3_K), wrong
    r, nsb = w["d"].shape
    d8, bs = act["d"], act["bsums"].astype(np.float64)
    assert d8.size == nsb and bs.shape == (nsb, 16), (d8.size, nsb, bs.shape)
    lv = q3_levels(w["q2"], w["hmask"], wrong).astype(np.float64)  # 0 .. 7, as the kernel's v_dot4 takes them
    x = act["q"].astype(np.float64).reshape(nsb, 16, 16)        # ELEMENT order: [scale group g, i]
    S = np.einsum("rsgi,sgi->rsg", lv.reshape(r, nsb, 16, 16), x)
    off = np.roll(bs, -1, axis=1) if wrong == "bsum_neighbour" else bs  # (the entry of group g + 1, as an off-by-one in the index would take)
    G = S - (0.0 if wrong == "offset_dropped" else 4.0 * off[None])
    assert np.max(np.abs(G)) <= 2 ** 13 + (2 ** 13 if wrong else 0)
    sc = q3_scales(w["s12"], wrong).astype(np.float64)
    tot = (sc * G).sum(axis=2)
    assert wrong or np.max(np.abs(tot)) < 2 ** 24
    # the reference's eight lanes (element e of a group feeds lane e % 8; the -4 is part of its levels)
    aux = np.einsum("rsg,rsghl,sghl->rsl", sc, (lv - 4.0).reshape(r, nsb, 16, 2, 8), x.reshape(nsb, 16, 2, 8))
    dd = w["d"] * d8[None]
    return dd * tot, np.abs(dd) * np.abs(aux).sum(axis=2), None


# ---- Q2_K ----
# nibbles_swapped: scale and min nibbles exchanged; min_added: + dmin summs; d_dmin_swapped: the halves of the (d, dmin) record
# exchanged; field_half_swapped: field s and half-piece h exchanged in the group index (g = 8 half + 2 h + s for s < 2: the
# quants and the bsum of another group against the field's own scale byte); bsum_neighbour: bsums of group g + 1; mask_0f: quants masked with 0x0F0F0F0F
# (fields s and s + 1 together); min_dropped_h1: no min term on the h = 1 pieces (what a lane that never received the scale bytes does
# to summs); scale_twin_half: the scale bytes of the other half (the h = 0 lane of the other pair handing its bytes over)
WRONG_Q2_K = ("nibbles_swapped", "min_added", "d_dmin_swapped", "field_half_swapped", "bsum_neighbour", "mask_0f", "min_dropped_h1",
              "scale_twin_half")


def q2_group_of(half, s, h, wrong=None):
    """the scale group of field s of piece (half, h); wrong = field_half_swapped: s and h exchanged where both are bits (s < 2)"""
    if wrong == "field_half_swapped" and s < 2:
        s, h = h, s
    return 8 * half + 2 * s + h


def q2_levels(qs, wrong=None):
    """the levels in element order, [.., 256], from the byte plane qs [.., 2, 32] (half, l): (qs >> 2 s) & 3 for element 128 half +
    32 s + l.  wrong = mask_0f: the mask of a 4-bit format, (qs >> 2 s) & 15"""
    mask = 15 if wrong == "mask_0f" else 3
    out = np.stack([(qs >> (2 * s)) & mask for s in range(4)], axis=-2)  # [.., half, s, l]
    return out.reshape(qs.shape[:-2] + (256,))


def q2_k_rows(b, wrong=None):
    """Q2_K block (buf_q2_k.rs:19-30): scales[16] | qs[64] | d f16 | dmin f16 = 84 bytes.  Element 128 half + 32 s + l of a super-block
    (half < 2, field s < 4, l < 32) has the level (qs[32 half + l] >> 2 s) & 3, i.e. 0 .. 3, and the scale group g = 8 half + 2 s +
    l / 16 (buf_q2_k.rs:44-67); its value is d (scales[g] & 15) level - dmin (scales[g] >> 4).
    d, dmin, the raw 2-bit plane qs [.., half, l] (bytes), the sixteen scale bytes, and what they make -- lv (levels 0 .. 3 in element
    order), sc (scales & 15), mn (scales >> 4)"""
    qs = b[:, :, 16:80].astype(np.int64).reshape(b.shape[0], b.shape[1], 2, 32)
    s16 = b[:, :, 0:16].astype(np.int64)
    return {"d": f16v(_u16(b[:, :, 80:82])), "dmin": f16v(_u16(b[:, :, 82:84])), "qs": qs, "s16": s16,
            "lv": q2_levels(qs).astype(np.float64), "sc": (s16 & 15).astype(np.float64), "mn": (s16 >> 4).astype(np.float64)}


def q2_k_values(w):
    """the dequantized elements of Q2_K rows, f64 [rows, nsb * 256] (16 groups of 16 elements: element order IS group order)"""
    r, nsb = w["d"].shape
    lv = w["lv"].reshape(r, nsb, 16, 16)
    return ((w["d"][:, :, None] * w["sc"])[:, :, :, None] * lv - (w["dmin"][:, :, None] * w["mn"])[:, :, :, None]).reshape(r, -1)


def q2_k_dots(w, act, wrong=None):
    """Q2_K row dot (q2k_terms = PieceQ2_K::term, gemv_core.hpp): a lane's PIECE (half, h) is the 16 bytes qs[32 half + 16 h .. + 16]; its
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
    -> (terms, A), each [rows, nsb]: per SUPER-BLOCK of every row the exact term d8 (d isum - dmin summs)"""
    assert act["qt"] == o.Q8_K and (wrong is None or wrong in WRONG_Q2_K), wrong
    r, nsb = w["d"].shape
    d8, bs = act["d"], act["bsums"].astype(np.float64)
    assert d8.size == nsb and bs.shape == (nsb, 16), (d8.size, nsb, bs.shape)
    lv = q2_levels(w["qs"], wrong).astype(np.float64)
    x = act["q"].astype(np.float64).reshape(nsb, 16, 16)  # ELEMENT order: [scale group g, i]
    # the group whose quants and bsum the piece (half, h) reads for its field s, by the group the field BELONGS to (element order)
    at = np.array([q2_group_of(g // 8, (g % 8) // 2, g % 2, wrong) for g in range(16)])
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
    return (a + b if wrong == "min_added" else a - b), np.abs(a) + np.abs(b), None


# ---- the f16 GEMM (k_gemm_f16w, gemm_f16w.hip): the block scales folded into f16 operands A', summed in f32 inside the matrix core ----
# Every rule below takes the blocks of the asked rows, blk [nr * nb, block bytes] (row after row), and returns (A' f16 as float64, W
# exact float64, error bound of A' against W), each [nr * nb, block elements], in ELEMENT order (the kernel's k-slot order is its own
# business: it has to pair the slots right to match).  u(v) = max(2^-11 |v|, 2^-25) bounds one f16 rounding of the exact value v.
U_F16 = 2.0 ** -11  # f16 unit roundoff (normal range)
SUB_F16 = 2.0 ** -25  # half the f16 subnormal spacing


def _f16(v):
    """one rounding of an exact float64 value to f16"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, np.float64).astype(np.float16)


def _u(v):
    """bound of one f16 rounding of the exact value v"""
    return np.maximum(U_F16 * np.abs(v), SUB_F16)


def _f16at(blk, a):
    return blk[:, a:a + 2].copy().view(np.float16).astype(np.float64)[:, 0:1]


_ONE = np.array([1.0], np.float16).view(np.uint8)


@dataclass
class F16W:
    operands: Callable                     # (blk, nr, nb, wrong) -> (A', W, bound)
    int_blocks: Callable                   # (rng, nb) -> [nb, block bytes]: blocks whose A' are small integers
    wrong: tuple = ()                      # the subtly wrong restatements the checker's own tests name
    code_blocks: Optional[Callable] = None  # (rng) -> 64 super-blocks that hit every scale code


def _nib(qs):
    """Q4_0 / Q4_1 nibbles of (nb, 16) bytes in element order: low nibbles = elements 0..15, high = 16..31"""
    return np.concatenate([qs & 15, qs >> 4], axis=1).astype(np.int64)


def _one_rounding(w):
    return _f16(w).astype(np.float64), w, _u(w)


def q4_0_f16w(blk, nr, nb, wrong=None):
    """A' = f16((q - 8) d): the exact product rounded once"""
    assert wrong is None
    return _one_rounding((_nib(blk[:, 2:]) - 8) * _f16at(blk, 0))


def q8_0_f16w(blk, nr, nb, wrong=None):
    """A' = f16(q d): the exact product rounded once"""
    assert wrong is None
    return _one_rounding(blk[:, 2:].view(np.int8).astype(np.int64) * _f16at(blk, 0))


def q4_1_f16w(blk, nr, nb, wrong=None):
    """A' = f16(n d + m): one rounding"""
    assert wrong is None
    return _one_rounding(_nib(blk[:, 4:]) * _f16at(blk, 0) + _f16at(blk, 2))


def q4_0_ints(rng, nb):
    """d = 1"""
    out = np.zeros((nb, 18), np.uint8)
    out[:, 0:2] = _ONE
    out[:, 2:] = rng.integers(0, 256, (nb, 16))
    return out


def q8_0_ints(rng, nb):
    """d = 1, quants -16 .. 16"""
    out = np.zeros((nb, 34), np.uint8)
    out[:, 0:2] = _ONE
    out[:, 2:] = rng.integers(-16, 17, (nb, 32)).astype(np.int8).view(np.uint8)
    return out


def q4_1_ints(rng, nb):
    """d = 1, m = 0 .. -8"""
    out = np.zeros((nb, 20), np.uint8)
    out[:, 0:2] = _ONE
    out[:, 2:4] = (-rng.integers(0, 9, nb)).astype(np.float16).view(np.uint8).reshape(nb, 2)
    out[:, 4:] = rng.integers(0, 256, (nb, 16))
    return out


def _q5_fields(blk, h, nr, nb, wrong):
    qh = np.ascontiguousarray(blk[:, h:h + 4]).view("<u4")[:, 0].reshape(nr, nb)  # (per row: a neighbour is the next block of the ROW)
    lv = q5_levels(blk[:, h + 4:].reshape(nr, nb, 16), qh, wrong).astype(np.float64).reshape(-1, 32)
    d = _f16at(blk, 0)
    if wrong == "scale_neighbour":
        d = np.roll(d.reshape(nr, nb), -1, axis=1).reshape(-1, 1)
    return d, lv


def q5_0_f16w(blk, nr, nb, wrong=None):
    """WF_Q5_0.  The kernel: 0x6400 | nibble | fifth bit << 4 is the f16 number 1024 + q5, -1040 makes it q5 - 16 exactly, then one
    product: A' = f16((q5 - 16) d), ONE rounding, |A' - W| <= u(W).  wrong: the operands of a kernel whose loader is subtly wrong in the
    named way (WRONG_Q5_01)"""
    assert wrong is None or wrong in WRONG_Q5_01, wrong
    d, q = _q5_fields(blk, 2, nr, nb, wrong)
    with np.errstate(invalid="ignore", over="ignore"):
        w = (q - (0.0 if wrong == "offset_dropped" else 16.0)) * d
    return _one_rounding(w)


def q5_1_f16w(blk, nr, nb, wrong=None):
    """WF_Q5_1.  The kernel: -1024 makes q5 exactly, then one v_pk_fma_f16: A' = f16(q5 d + m), ONE rounding, |A' - W| <= u(W)"""
    assert wrong is None or wrong in WRONG_Q5_01, wrong
    d, q = _q5_fields(blk, 4, nr, nb, wrong)
    m = _f16at(blk, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        w = q * d + (m * 0.0 if wrong == "offset_dropped" else m)
    return _one_rounding(w)


def q5_0_ints(rng, nb):
    """d = 1, random nibbles and fifth bits"""
    out = np.zeros((nb, 22), np.uint8)
    out[:, 0:2] = _ONE
    out[:, 2:] = rng.integers(0, 256, (nb, 20))
    return out


def q5_1_ints(rng, nb):
    """d = 1, m = 0 .. -8, random nibbles and fifth bits"""
    out = np.zeros((nb, 24), np.uint8)
    out[:, 0:2] = _ONE
    out[:, 2:4] = (-rng.integers(0, 9, nb)).astype(np.float16).view(np.uint8).reshape(nb, 2)
    out[:, 4:] = rng.integers(0, 256, (nb, 20))
    return out


def scale_codes(s12):
    """scales[12] [nb, 12] -> the 6-bit scale and minimum codes of the eight sub-blocks of Q4_K / Q5_K, ([nb, 8], [nb, 8]) (util.rs:19-27)"""
    sc, mn = _scale_min_k4(np.asarray(s12, np.int64)[None])
    return sc[0].astype(np.int64), mn[0].astype(np.int64)


def pack_codes(sc, mn):
    """the inverse of scale_codes: [nb, 8] x 2 -> scales[12]"""
    sc, mn = np.asarray(sc, np.int64), np.asarray(mn, np.int64)
    s12 = np.zeros(sc.shape[:1] + (12,), np.int64)
    for j in range(4):
        s12[:, j] = sc[:, j] | ((sc[:, j + 4] >> 4) << 6)
        s12[:, j + 4] = mn[:, j] | ((mn[:, j + 4] >> 4) << 6)
        s12[:, j + 8] = (sc[:, j + 4] & 15) | ((mn[:, j + 4] & 15) << 4)
    return s12.astype(np.uint8)


def nibbles(qs):
    """qs [nb, 128] of Q4_K / Q5_K -> the 4-bit part of every element in element order, [nb, 256]: pair p is 32 low nibbles, then 32 high"""
    q = qs.astype(np.int64).reshape(-1, 4, 32)
    return np.stack([q & 15, q >> 4], axis=2).reshape(-1, 256)


def _scaled_minus_min(q, dsc, dm, plus=False):
    """A' = f16(q c1 - c2), c1 = f16(d sc), c2 = f16(dmin m) -- q exact, the product exact inside one fma: c1 and c2 one rounding each,
    then ONE rounding of q c1 - c2 (charged against |q c1| + |c2|, not |A'|): |A' - W| <= q u(d sc) + u(dmin m) + u(q |c1| + |c2|)"""
    c1, c2 = _f16(dsc).astype(np.float64), _f16(dm).astype(np.float64)
    return _f16(q * c1 + c2 if plus else q * c1 - c2).astype(np.float64), q * dsc - dm, q * _u(dsc) + _u(dm) + _u(q * np.abs(c1) + np.abs(c2))


def q4_k_f16w(blk, nr, nb, wrong=None):
    """A' = f16(n c1 - c2), c1 = f16(d sc), c2 = f16(dmin m); sub-block 2 j: the low nibbles of qs[32 j ..], 2 j + 1: the high ones"""
    assert wrong is None
    sc, mn = scale_codes(blk[:, 4:16])
    sub = np.arange(256) >> 5
    return _scaled_minus_min(nibbles(blk[:, 16:]), _f16at(blk, 0) * sc[:, sub], _f16at(blk, 2) * mn[:, sub])


def q4_k_ints(rng, nb):
    """d = dmin = 1, sub-scales 0..3, minimums 0..7"""
    out = np.zeros((nb, 144), np.uint8)
    out[:, 0:2] = _ONE
    out[:, 2:4] = _ONE
    sc, mn = rng.integers(0, 4, (nb, 8)), rng.integers(0, 8, (nb, 8))
    out[:, 4:8], out[:, 8:12] = sc[:, :4], mn[:, :4]  # (values < 16: no high bits in bytes 0..7)
    out[:, 12:16] = sc[:, 4:] | (mn[:, 4:] << 4)
    out[:, 16:] = rng.integers(0, 256, (nb, 128))
    return out


# subblocks_swapped: the two sub-blocks of a pair (the low and the high nibbles' scale and minimum) exchanged; qh_next_pair: the qh bits
# of pair p + 1; qh_bits_swapped: the low and the high nibble's qh bits exchanged; plus_c2: q c1 + c2; fifth_bit_8: the fifth bit worth 8
WRONG_F16W_Q5_K = ("subblocks_swapped", "qh_next_pair", "qh_bits_swapped", "plus_c2", "fifth_bit_8")


def q5_k_f16w(blk, nr, nb, wrong=None):
    """WF_Q5_K.  Element 64 p + 32 hi + l of a super-block (pair p < 4, hi < 2, l < 32) has the level q = (nibble hi of qs[32 p + l]) +
    16 (bit 2 p + hi of qh[l]), 0 .. 31, and belongs to sub-block 2 p + hi, whose 6-bit scale code sc and minimum code m are Q4_K's
    fields: W = d sc q - dmin m (buf_q5_k.rs:24-63).  The kernel: A' = f16(q c1 - c2), c1 = f16(d sc), c2 = f16(dmin m): three roundings"""
    assert wrong is None or wrong in WRONG_F16W_Q5_K, wrong
    sc, mn = scale_codes(blk[:, 160:172])
    sub = np.arange(256) >> 5  # element 64 p + 32 hi + l: sub-block 2 p + hi
    if wrong == "subblocks_swapped":
        sub = sub ^ 1
    hb = fifth_bits(blk[:, 128:160].astype(np.int64), shift_pair=1 if wrong == "qh_next_pair" else 0, swap=wrong == "qh_bits_swapped")
    q = (nibbles(blk[:, 0:128]) + (8 if wrong == "fifth_bit_8" else 16) * hb).astype(np.float64)
    return _scaled_minus_min(q, _f16at(blk, 172) * sc[:, sub], _f16at(blk, 174) * mn[:, sub], plus=wrong == "plus_c2")


def q5_k_ints(rng, nb):
    """d = dmin = 1, scale codes 0..3 and minimum codes 0..7 (|A'| <= 31 * 3 + 7: tier 1's sums stay below 2^24 at every shape of
    tests/test_hip_f16w_gemm.py), random levels and fifth bits"""
    out = np.zeros((nb, 176), np.uint8)
    out[:, 0:160] = rng.integers(0, 256, (nb, 160))
    out[:, 160:172] = pack_codes(rng.integers(0, 4, (nb, 8)), rng.integers(0, 8, (nb, 8)))
    out[:, 172:174] = _ONE
    out[:, 174:176] = _ONE
    return out


def q5_k_code_blocks(rng):
    """64 super-blocks that between them hold every 6-bit scale code and every minimum code in every sub-block and, in every block,
    random nibbles and fifth bits (both qh states at every pair and nibble), with random f16 scales of either sign"""
    nb = 64
    raw = synth.random_blocks(rng, nb * 256, synth.Q5_K).reshape(nb, -1).copy()
    i, j = np.arange(nb)[:, None], np.arange(8)[None, :]
    raw[:, 160:172] = pack_codes((i + 8 * j) % 64, (3 * i + 5 * j + 1) % 64)
    raw[:, 0:160] = rng.integers(0, 256, (nb, 160))
    raw[::2, 173] ^= 0x80
    raw[::3, 175] ^= 0x80
    return raw.reshape(-1)


def q6_k_f16w(blk, nr, nb, wrong=None):
    """A' = f16((q - 32) c), c = f16(d sc): |A' - W| <= |q - 32| u(d sc) + u((q - 32) c)"""
    assert wrong is None
    d = _f16at(blk, 208)
    ql, qh = blk[:, :128].astype(np.int64), blk[:, 128:192].astype(np.int64)
    sc = blk[:, 192:208].view(np.int8).astype(np.int64)
    q = np.zeros((blk.shape[0], 256), np.int64)
    s = np.zeros_like(q)
    for h in range(2):
        L, H = ql[:, 64 * h:64 * h + 64], qh[:, 32 * h:32 * h + 32]
        for j, (lo, sh) in enumerate(((L[:, :32] & 15, 0), (L[:, 32:] & 15, 2), (L[:, :32] >> 4, 4), (L[:, 32:] >> 4, 6))):
            e0 = 128 * h + 32 * j
            q[:, e0:e0 + 32] = lo | (((H >> sh) & 3) << 4)
            s[:, e0:e0 + 32] = np.repeat(sc[:, 8 * h + 2 * j:8 * h + 2 * j + 2], 16, axis=1)
    dsc = d * s
    c = _f16(dsc).astype(np.float64)
    return _f16((q - 32) * c).astype(np.float64), (q - 32) * dsc, np.abs(q - 32) * _u(dsc) + _u((q - 32) * c)


def q6_k_ints(rng, nb):
    """d = 1, scales -2..2"""
    out = np.zeros((nb, 210), np.uint8)
    out[:, :192] = rng.integers(0, 256, (nb, 192))
    out[:, 192:208] = rng.integers(-2, 3, (nb, 16)).astype(np.int8).view(np.uint8)
    out[:, 208:210] = _ONE
    return out


# Q2_K / Q3_K.  groups_swapped: the two scale groups of a slot pair (shifts 2 c and 2 c + 1 of the same bytes) exchanged;
# hmask_next_shift: the hmask bit of shift j + 1; plus_c2: n c1 + c2; scale_minus_31: code - 31
WRONG_F16W_Q2_K = ("groups_swapped", "plus_c2")
WRONG_F16W_Q3_K = ("groups_swapped", "hmask_next_shift", "scale_minus_31")


def _group_of_element(wrong=None):
    """the scale group of every element of a Q2_K / Q3_K super-block, [256]"""
    e = np.arange(256)
    h, j, l = e >> 7, (e >> 5) & 3, e & 31
    if wrong == "groups_swapped":
        j = j ^ 1
    return 8 * h + 2 * j + (l >> 4)


def levels2(qs):
    """the 2-bit fields of qs [nsb, 64] in element order, [nsb, 256]"""
    q = qs.astype(np.int64).reshape(-1, 2, 1, 32)
    return ((q >> (2 * np.arange(4)).reshape(1, 1, 4, 1)) & 3).reshape(-1, 256)


def hbits(hmask, wrong=None):
    """bit 4 h + j of hmask[l] for element 128 h + 32 j + l, [nsb, 256]"""
    e = np.arange(256)
    h, j, l = e >> 7, (e >> 5) & 3, e & 31
    if wrong == "hmask_next_shift":
        j = (j + 1) & 3
    return (hmask.astype(np.int64)[:, l] >> (4 * h + j)[None, :]) & 1


def q2_k_f16w(blk, nr, nb, wrong=None):
    """Element 128 h + 32 j + l of a super-block (h < 2, shift j < 4, l < 32) is the level n = (qs[32 h + l] >> 2 j) & 3 of scale group
    g = 8 h + 2 j + l / 16, whose byte scales[g] holds the scale (low nibble) and the minimum (high nibble): W = d sc n - dmin m
    (buf_q2_k.rs:35-66).  The kernel: A' = f16(n c1 - c2), c1 = f16(d sc), c2 = f16(dmin m): three roundings"""
    assert wrong is None or wrong in WRONG_F16W_Q2_K, wrong
    grp = _group_of_element(wrong)
    s16 = blk[:, 0:16].astype(np.int64)
    n = levels2(blk[:, 16:80]).astype(np.float64)
    return _scaled_minus_min(n, _f16at(blk, 80) * (s16 & 15)[:, grp], _f16at(blk, 82) * (s16 >> 4)[:, grp], plus=wrong == "plus_c2")


def q3_k_f16w(blk, nr, nb, wrong=None):
    """The same element has the level q = ((qs[32 h + l] >> 2 j) & 3) - (bit 4 h + j of hmask[l] ? 0 : 4), -4 .. 3, and the same group;
    W = d (code - 32) q (buf_q3_k.rs:37-84).  The kernel: A' = f16(q c), c = f16(d (code - 32)) -- two roundings, |A' - W| <=
    |q| u(d (code - 32)) + u(q c)"""
    assert wrong is None or wrong in WRONG_F16W_Q3_K, wrong
    grp = _group_of_element(wrong)
    code = q3_scales(blk[:, 96:108].astype(np.int64)) + 32  # (q3_scales gives code - 32)
    q = (levels2(blk[:, 32:96]) - 4 * (1 - hbits(blk[:, 0:32], wrong))).astype(np.float64)
    dsc = _f16at(blk, 108) * (code - (31 if wrong == "scale_minus_31" else 32))[:, grp]
    c = _f16(dsc).astype(np.float64)
    return _f16(q * c).astype(np.float64), q * dsc, np.abs(q) * _u(dsc) + _u(q * c)


def q3_k_pack_codes(code):
    """scales[12] of Q3_K from the sixteen 6-bit codes [nb, 16]: the inverse of the reference's aux[] shuffle"""
    code = np.asarray(code, np.int64)
    s12 = np.zeros((code.shape[0], 12), np.int64)
    for g in range(16):
        s12[:, g % 8] |= (code[:, g] & 15) << (4 * (g // 8))
        s12[:, 8 + g % 4] |= (code[:, g] >> 4) << (2 * (g // 4))
    return s12.astype(np.uint8)


def q2_k_ints(rng, nb):
    """d = dmin = 1, scale codes 0..3 and minimums 0..7"""
    out = np.zeros((nb, 84), np.uint8)
    out[:, 0:16] = rng.integers(0, 4, (nb, 16)) | (rng.integers(0, 8, (nb, 16)) << 4)
    out[:, 16:80] = rng.integers(0, 256, (nb, 64))
    out[:, 80:82] = _ONE
    out[:, 82:84] = _ONE
    return out


def q3_k_ints(rng, nb):
    """d = 1, scale codes 30..34"""
    out = np.zeros((nb, 110), np.uint8)
    out[:, 0:96] = rng.integers(0, 256, (nb, 96))
    out[:, 96:108] = q3_k_pack_codes(rng.integers(30, 35, (nb, 16)))
    out[:, 108:110] = _ONE
    return out


def q2_k_code_blocks(rng):
    """64 super-blocks that between them hold every 4-bit scale and minimum in every group and, in every block, all four levels at every
    shift (random bits), with random f16 scales of either sign"""
    nb = 64
    raw = synth.random_blocks(rng, nb * 256, synth.Q2_K).reshape(nb, -1).copy()
    i, g = np.arange(nb)[:, None], np.arange(16)[None, :]
    raw[:, 0:16] = ((i + g) % 16) | (((3 * i + 5 * g + 1) % 16) << 4)
    raw[:, 16:80] = rng.integers(0, 256, (nb, 64))
    raw[::2, 81] ^= 0x80
    raw[::3, 83] ^= 0x80
    return raw.reshape(-1)


def q3_k_code_blocks(rng):
    """64 super-blocks that between them hold every 6-bit scale code and, in every block, both hmask states and all four levels at every
    shift (random bits), with random f16 scales of either sign"""
    nb = 64
    raw = synth.random_blocks(rng, nb * 256, synth.Q3_K).reshape(nb, -1).copy()
    i, g = np.arange(nb)[:, None], np.arange(16)[None, :]
    raw[:, 96:108] = q3_k_pack_codes((i + 4 * g) % 64)
    raw[:, 0:96] = rng.integers(0, 256, (nb, 96))
    raw[::2, 109] ^= 0x80
    return raw.reshape(-1)


# ---- the table ----
@dataclass
class Format:
    typ: int                    # the synth type (the table's key)
    ht: str                     # the GGMLType attribute name
    rhs: int                    # the quantization its rows are read against (o.Q8_0 / Q8_1 / Q8_K)
    scales_at: tuple            # byte offsets of the block's f16 scale fields (d; d | m; d | dmin)
    rows: Callable              # the row reader
    dots: Callable              # the row-dot rule
    C: int                      # ... and the constant of its bound
    wrong: tuple = ()           # the subtly wrong kernels / loaders the checker's own tests name
    signs_at: Optional[tuple] = None  # the scale fields flip_signs flips (None: all of scales_at; Q4_1 / Q5_1: d alone, m stays as it is)
    values: Optional[Callable] = None  # K-quants: the dequantized elements of the reader's rows
    f16w: Optional[F16W] = None  # k_gemm_f16w's form for the format

    @property
    def name(self):
        return synth.TYPE_NAMES[self.typ]

    @property
    def block_bytes(self):
        return synth.BLOCK_BYTES[self.typ]

    @property
    def block_elems(self):
        return synth.BLOCK_ELEMS[self.typ]

    @property
    def kq(self):
        """a 256-element format: its B' slot group is a super-block, its rhs Q8_K"""
        return self.block_elems == 256


FORMATS = {f.typ: f for f in (
    Format(synth.Q4_0, "Q4_0", o.Q8_0, (0,), q4_0_rows, block_dots, C_DOT, f16w=F16W(q4_0_f16w, q4_0_ints)),
    Format(synth.Q8_0, "Q8_0", o.Q8_0, (0,), q8_0_rows, block_dots, C_DOT, f16w=F16W(q8_0_f16w, q8_0_ints)),
    Format(synth.Q4_1, "Q4_1", o.Q8_1, (0, 2), q4_1_rows, f16_product_dots, C_DOT, signs_at=(0,), f16w=F16W(q4_1_f16w, q4_1_ints)),
    Format(synth.Q5_0, "Q5_0", o.Q8_0, (0,), q5_0_rows, q5_0_dots, C_DOT, WRONG_Q5_01, f16w=F16W(q5_0_f16w, q5_0_ints, WRONG_Q5_01)),
    Format(synth.Q5_1, "Q5_1", o.Q8_1, (0, 2), q5_1_rows, q5_1_dots, C_DOT, WRONG_Q5_01, signs_at=(0,),
           f16w=F16W(q5_1_f16w, q5_1_ints, WRONG_Q5_01)),
    Format(synth.Q2_K, "Q2K", o.Q8_K, (80, 82), q2_k_rows, q2_k_dots, C_Q2K, WRONG_Q2_K, values=q2_k_values,
           f16w=F16W(q2_k_f16w, q2_k_ints, WRONG_F16W_Q2_K, q2_k_code_blocks)),
    Format(synth.Q3_K, "Q3K", o.Q8_K, (108,), q3_k_rows, q3_k_dots, C_Q3K, WRONG_Q3_K, values=q3_k_values,
           f16w=F16W(q3_k_f16w, q3_k_ints, WRONG_F16W_Q3_K, q3_k_code_blocks)),
    Format(synth.Q4_K, "Q4K", o.Q8_K, (0, 2), q4_k_rows, q4_k_dots, C_K, ("scale_neighbour", "min_neighbour", "dmin_plus"), values=q4_k_values,
           f16w=F16W(q4_k_f16w, q4_k_ints)),
    Format(synth.Q5_K, "Q5K", o.Q8_K, (172, 174), q5_k_rows, q5_k_dots, C_K, WRONG_Q5_K, values=q4_k_values,
           f16w=F16W(q5_k_f16w, q5_k_ints, WRONG_F16W_Q5_K, q5_k_code_blocks)),
    Format(synth.Q6_K, "Q6K", o.Q8_K, (208,), q6_k_rows, q6_k_dots, C_K, WRONG_Q6_K, values=q6_k_values, f16w=F16W(q6_k_f16w, q6_k_ints)),
)}
BY_NAME = {f.name: f for f in FORMATS.values()}

# what attn_v / attn_output / ffn_down of a body's recipe family may be (the body's own format is held on attn_q, attn_k, ffn_gate, ffn_up)
FAMILY = {synth.Q2_K: (synth.Q2_K, synth.Q3_K, synth.Q4_K), synth.Q3_K: (synth.Q3_K, synth.Q4_K, synth.Q5_K), synth.Q5_K: (synth.Q5_K, synth.Q6_K)}


def weight_rows(t, r0, r1, wrong=None):
    """rows [r0, r1) of a weight tensor (synth.RawTensor) -> its format's dict of exact integer / f64 fields, [rows, nb, ...]"""
    if t.typ not in FORMATS:
        raise ValueError(f"weight type {t.typ}")
    F = FORMATS[t.typ]
    rows, k = t.shape
    b = np.ascontiguousarray(t.data).view(np.uint8).reshape(rows, k // F.block_elems, F.block_bytes)[r0:r1]
    return dict(F.rows(b, wrong), typ=t.typ)


def k_values(w):
    """the dequantized elements of K-quant weight rows (weight_rows), f64, [rows, nsb * 256] -- sum |w_i x_i| of the project's bound"""
    return FORMATS[w["typ"]].values(w)


def chunk_dots(w, act, drop_last_block=False, wrong=None):
    """(exact, bound) of the weight rows `w` (weight_rows) against one row's activation blocks -- THE tail of every format's rule: the
    terms without each row's last block where a kernel whose block loop stops one early is restated, their sum, (n_terms + C) U sum A"""
    F = FORMATS[w["typ"]]
    terms, A, cap = F.dots(w, act, wrong)
    if drop_last_block:  # (a K-quant row's block is a super-block)
        if F.kq:
            terms = terms[:, :-1]
        else:
            terms = terms.copy()
            terms[:, -1] = 0.0
    if A is None:
        A = np.abs(terms)
    axes = tuple(range(1, A.ndim))
    bound = (int(np.prod(A.shape[1:])) + F.C) * U * A.sum(axis=axes)
    return terms.sum(axis=axes), bound if cap is None else np.minimum(cap, bound)
