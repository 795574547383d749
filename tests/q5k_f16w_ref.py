"""The Q5_K form of k_gemm_f16w (gemm_f16w.hip: WF_Q5_K) restated in numpy, in ELEMENT order, for the tests of the kernel
(tests/test_hip_f16w_gemm_q5k.py) and of the prompt pass that runs it in a context created with CRABML_HIP_LLAMA_PREFILL_Q5K_GEMM
(tests/test_hip_prefill_q5k_launches.py).

  Q5_K block, the reference's field order (buf_q5_k.rs:13-21): qs[128] | qh[32] | scales[12] | d f16 | dmin f16 = 176 bytes.  Element
      64 p + 32 hi + l of a super-block (pair p < 4, hi < 2, l < 32) has the level q = (nibble hi of qs[32 p + l]) + 16 (bit 2 p + hi of
      qh[l]), 0 .. 31, and belongs to sub-block 2 p + hi, whose 6-bit scale code sc and minimum code m are Q4_K's fields (util.rs:19-27):
      W = d sc q - dmin m (buf_q5_k.rs:24-63).
      The kernel:  A' = f16(q c1 - c2),  c1 = f16(d sc),  c2 = f16(dmin m)  -- q exact, the product exact inside one fma: three roundings,
      |A' - W| <= q u(d sc) + u(dmin m) + u(q |c1| + |c2|).
  u(v) = max(2^-11 |v|, 2^-25): one f16 rounding of the exact value v (tests/test_hip_f16w_gemm.py).

Also here: the map from the lane's loads to B' slot order 3 (the order Q2_K / Q3_K read, which Q5_K shares), generators of blocks whose
A' are small integers (the exact tier) and of blocks that hit every scale and minimum code in every sub-block with both qh states at
every pair and nibble, the single MUTATIONS of the restatement that the checker's own tests must tell apart from it, and the context
managers that let the existing checkers of tests/test_hip_f16w_gemm.py and tests/prefill_pass_ref.py read the format -- nested in
tests/q23k_f16w_ref.py's, so that a Q3_K_M / Q3_K_L body is read whole."""
import contextlib

import numpy as np

from crabml_amd import synth
from oracle import oracle as o
from tests import q23k_f16w_ref as Q23
from tests import test_hip_f16w_gemm as G
from tests.q5k_step_ref import fifth_bits
from tests.test_hip_f16w_gemm import _f16, _u

FMT = "Q5_K"
# subblocks_swapped: the two sub-blocks of a pair (the low and the high nibbles' scale and minimum) exchanged; qh_next_pair: the qh bits
# of pair p + 1; qh_bits_swapped: the low and the high nibble's qh bits exchanged; plus_c2: q c1 + c2; fifth_bit_8: the fifth bit worth 8
WRONG = ("subblocks_swapped", "qh_next_pair", "qh_bits_swapped", "plus_c2", "fifth_bit_8")


def scale_codes(s12):
    """scales[12] [nb, 12] -> the 6-bit scale and minimum codes of the eight sub-blocks, ([nb, 8], [nb, 8]) (util.rs:19-27)"""
    s12 = np.asarray(s12, np.int64)
    sc, mn = np.empty(s12.shape[:1] + (8,), np.int64), np.empty(s12.shape[:1] + (8,), np.int64)
    for j in range(4):
        sc[:, j], mn[:, j] = s12[:, j] & 63, s12[:, j + 4] & 63
        sc[:, j + 4] = (s12[:, j + 8] & 15) | ((s12[:, j] >> 6) << 4)
        mn[:, j + 4] = (s12[:, j + 8] >> 4) | ((s12[:, j + 4] >> 6) << 4)
    return sc, mn


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
    """qs [nb, 128] -> the 4-bit part of every element in element order, [nb, 256]: pair p is 32 low nibbles, then 32 high ones"""
    q = qs.astype(np.int64).reshape(-1, 4, 32)
    return np.stack([q & 15, q >> 4], axis=2).reshape(-1, 256)


def weight_operands(raw, fmt, rows, k, wrong=None):
    """(A' f16 as float64, W exact float64, error bound of A' against W), each (len(rows), k), for the given weight rows of raw Q5_K
    blocks; wrong: a restatement that is subtly wrong in the named way (WRONG)"""
    assert fmt == FMT and (wrong is None or wrong in WRONG), (fmt, wrong)
    rb = k // 256 * 176
    raw = np.ascontiguousarray(raw).view(np.uint8)
    blk = np.stack([raw[r * rb:(r + 1) * rb] for r in rows]).reshape(-1, 176)
    f16at = lambda a: blk[:, a:a + 2].copy().view(np.float16).astype(np.float64)[:, 0:1]  # noqa: E731
    d, dmin = f16at(172), f16at(174)
    sc, mn = scale_codes(blk[:, 160:172])
    sub = np.arange(256) >> 5  # element 64 p + 32 hi + l: sub-block 2 p + hi
    if wrong == "subblocks_swapped":
        sub = sub ^ 1
    hb = fifth_bits(blk[:, 128:160].astype(np.int64), shift_pair=1 if wrong == "qh_next_pair" else 0, swap=wrong == "qh_bits_swapped")
    q = (nibbles(blk[:, 0:128]) + (8 if wrong == "fifth_bit_8" else 16) * hb).astype(np.float64)
    dsc, dm = d * sc[:, sub], dmin * mn[:, sub]
    c1, c2 = _f16(dsc).astype(np.float64), _f16(dm).astype(np.float64)
    w = q * dsc - dm
    ap = _f16(q * c1 + c2 if wrong == "plus_c2" else q * c1 - c2).astype(np.float64)
    ea = q * _u(dsc) + _u(dm) + _u(q * np.abs(c1) + np.abs(c2))
    nr = len(rows)
    return ap.reshape(nr, k), w.reshape(nr, k), ea.reshape(nr, k)


def order3_pos(E):
    """f16w_pos_q8k(3, 0, E) (f16w_rows.hpp) restated: the position, in halfs from the super-block's start, of element E = 128 h + 32 j + l
    in B' slot order 3 -- chunk j / 2, lane group g = 2 h + l / 16, step s = (l / 4) % 4, slots 4 (j & 1) .. in the order 0, 2, 1, 3"""
    E = np.asarray(E)
    l, j = E & 31, (E >> 5) & 3
    g, s, k, hi, cc = 2 * (E >> 7) + (l >> 4), (l >> 2) & 3, l & 3, j & 1, j >> 1
    return (4 * cc + g) * 32 + 8 * s + 4 * hi + ((k >> 1) | ((k & 1) << 1))


def lane_slots():
    """What the kernel's lanes put into the A' slots, as (element [256], position [256]): in chunk c of a super-block lane group g loads
    the 16-byte piece g & 1 of pair p = 2 (g >> 1) + c -- bytes qs[32 p + 16 (g & 1) + 4 s + b], dword s in step s -- and unpack_q5_k_f16
    writes, to the step's slots 0..7, the low nibbles of bytes 0, 2, 1, 3 and then the high nibbles of bytes 0, 2, 1, 3, each with bit
    2 p + hi of qh[16 (g & 1) + 4 s + b].  The element of (p, hi, l) is 64 p + 32 hi + l; the slot's position is chunk c, group g, step s,
    slot e: (4 c + g) * 32 + 8 s + e -- where B' must hold the same element."""
    elem, pos, qh_bit = [], [], []
    for c in range(2):
        for g in range(4):
            p = 2 * (g >> 1) + c
            for s in range(4):
                for e in range(8):
                    hi, b = e >> 2, (0, 2, 1, 3)[e & 3]
                    l = 16 * (g & 1) + 4 * s + b
                    elem.append(64 * p + 32 * hi + l)
                    pos.append((4 * c + g) * 32 + 8 * s + e)
                    qh_bit.append((l, 4 * (g >> 1) + 2 * c + hi))  # the kernel's shift 4 (g >> 1) + 2 c, then bit hi
    return np.array(elem), np.array(pos), qh_bit


def int_weights(rng, fmt, m, k):
    """blocks whose A' are small integers: d = dmin = 1, scale codes 0..3 and minimum codes 0..7 (|A'| <= 31 * 3 + 7: tier 1's sums stay
    below 2^24 at every shape of tests/test_hip_f16w_gemm.py), random levels and fifth bits"""
    assert fmt == FMT
    nb = m * k // 256
    one = np.array([1.0], np.float16).view(np.uint8)
    out = np.zeros((nb, 176), np.uint8)
    out[:, 0:160] = rng.integers(0, 256, (nb, 160))
    out[:, 160:172] = pack_codes(rng.integers(0, 4, (nb, 8)), rng.integers(0, 8, (nb, 8)))
    out[:, 172:174] = one
    out[:, 174:176] = one
    return out.reshape(-1)


def code_blocks(rng, fmt=FMT):
    """64 super-blocks that between them hold every 6-bit scale code and every minimum code in every sub-block and, in every block,
    random nibbles and fifth bits (both qh states at every pair and nibble), with random f16 scales of either sign"""
    assert fmt == FMT
    nb = 64
    raw = synth.random_blocks(rng, nb * 256, synth.Q5_K).reshape(nb, -1).copy()
    i, j = np.arange(nb)[:, None], np.arange(8)[None, :]
    raw[:, 160:172] = pack_codes((i + 8 * j) % 64, (3 * i + 5 * j + 1) % 64)
    raw[:, 0:160] = rng.integers(0, 256, (nb, 160))
    raw[::2, 173] ^= 0x80
    raw[::3, 175] ^= 0x80
    return raw.reshape(-1)


@contextlib.contextmanager
def _q5k_layer():
    """Q5_K on top of whatever tests/test_hip_f16w_gemm.py's tables currently hold"""
    saved = G.weight_operands, G.int_weights, G.KQ
    saved_tabs = dict(G.HT), dict(G.ROWS)

    def wo(raw, fmt, rows, k):
        return weight_operands(raw, fmt, rows, k) if fmt == FMT else saved[0](raw, fmt, rows, k)

    def iw(rng, fmt, m, k):
        return int_weights(rng, fmt, m, k) if fmt == FMT else saved[1](rng, fmt, m, k)

    G.weight_operands, G.int_weights, G.KQ = wo, iw, tuple(saved[2]) + (FMT,)
    G.HT[FMT] = "Q5K"
    G.ROWS[FMT] = o.Q8_K
    try:
        yield
    finally:
        G.weight_operands, G.int_weights, G.KQ = saved
        for tab, old in ((G.HT, saved_tabs[0]), (G.ROWS, saved_tabs[1])):
            tab.clear()
            tab.update(old)


@contextlib.contextmanager
def q5k_operands():
    """tests/test_hip_f16w_gemm.py's checkers read Q5_K -- and Q2_K / Q3_K (q23k_f16w_ref.q23k_operands) -- inside this block"""
    with Q23.q23k_operands(), _q5k_layer():
        yield


@contextlib.contextmanager
def q5k_pass():
    """tests/prefill_pass_ref.py's check_pass reads passes whose Q5_K matrices took the f16 GEMM inside this block, over Q5_K bodies and
    over the Q3_K recipes that hold Q5_K tensors: q23k_f16w_ref.q23k_pass, plus Q5_K among the GEMM's formats and among the readers of a
    B' in slot order 3.  Nothing else of the checker changes -- its bounds and its excused-share cap are its own"""
    from tests import prefill_pass_ref as P
    with Q23.q23k_pass(), _q5k_layer():
        saved = P.weight_operands, P.check_xh
        saved_fmt = dict(P.F16W_FMT)
        inner_check_xh = P.check_xh

        def check_xh(res, tap, xh_name, act_name, ctx, model=None, wname=None):
            """a Q8_K-row B' whose reader is Q5_K is held to the same multiset per super-block as every K-quant reader's"""
            typ = model.tensors[wname].typ if (model is not None and xh_name in tap) else None
            if typ != synth.Q5_K:
                return inner_check_xh(res, tap, xh_name, act_name, ctx, model, wname)
            acts = P.act_rows(tap, act_name)
            bits, _ = P.b_prime(acts)
            b, k = bits.shape
            got = np.asarray(tap[xh_name], dtype=np.uint16).reshape(b, k)
            same = np.all(G.b_groups(got, FMT, b, k) == G.b_groups(bits, FMT, b, k), axis=2)
            if not same.all():
                r, blk = np.argwhere(~same)[0]
                res.fails.append(f"{ctx} {res.launch}: {xh_name} row {r} block {blk}: B' is not f16(q d) of the tapped planes ({int((~same).sum())} blocks)")

        P.weight_operands, P.check_xh = G.weight_operands, check_xh
        P.F16W_FMT[synth.Q5_K] = FMT
        try:
            yield
        finally:
            P.weight_operands, P.check_xh = saved
            P.F16W_FMT.clear()
            P.F16W_FMT.update(saved_fmt)
