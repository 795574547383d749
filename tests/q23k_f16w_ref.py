"""The Q2_K and Q3_K forms of k_gemm_f16w (gemm_f16w.hip) restated in numpy, in ELEMENT order, for the tests of the kernel
(tests/test_hip_f16w_gemm_q23k.py) and of the prompt pass that runs it (tests/test_hip_prefill_q23k_launches.py).

  Q2_K block (buf_q2_k.rs:19-29): scales[16] | qs[64] | d f16 | dmin f16 = 84 bytes.  Element 128 h + 32 j + l of a super-block (h < 2,
      shift j < 4, l < 32) is the level n = (qs[32 h + l] >> 2 j) & 3 of scale group g = 8 h + 2 j + l / 16, whose byte scales[g] holds
      the scale (low nibble) and the minimum (high nibble): W = d sc n - dmin m (buf_q2_k.rs:35-66).
      The kernel:  A' = f16(n c1 - c2),  c1 = f16(d sc),  c2 = f16(dmin m)  -- n exact, the product exact inside one fma: three roundings,
      |A' - W| <= n u(d sc) + u(dmin m) + u(n |c1| + |c2|).
  Q3_K block (buf_q3_k.rs:19-30): hmask[32] | qs[64] | scales[12] | d f16 = 110 bytes.  The same element has the level q = ((qs[32 h + l]
      >> 2 j) & 3) - (bit 4 h + j of hmask[l] ? 0 : 4), -4 .. 3, and the same group; the 6-bit scale code of group g is nibble g / 8 of
      scales[g % 8] with bits 2 (g / 4), 2 (g / 4) + 1 of scales[8 + g % 4] on top (the reference's aux[] shuffle): W = d (code - 32) q
      (buf_q3_k.rs:37-84).
      The kernel:  A' = f16(q c),  c = f16(d (code - 32))  -- two roundings,  |A' - W| <= |q| u(d (code - 32)) + u(q c).
  u(v) = max(2^-11 |v|, 2^-25): one f16 rounding of the exact value v (tests/test_hip_f16w_gemm.py).

Also here: generators of blocks whose A' are small integers (the exact tier), blocks that hit every scale code and both hmask states
at every shift, the single MUTATIONS of the restatement that the checker's own tests must tell apart from it, and the context manager
that lets the existing checkers of tests/test_hip_f16w_gemm.py and tests/prefill_pass_ref.py read the two formats."""
import contextlib

import numpy as np

from crabml_amd import synth
from oracle import oracle as o
from tests import test_hip_f16w_gemm as G
from tests.q3k_step_ref import scales as q3k_scale_codes
from tests.test_hip_f16w_gemm import _f16, _u

FMTS = ("Q2_K", "Q3_K")
HT = {"Q2_K": "Q2K", "Q3_K": "Q3K"}
# groups_swapped: the two scale groups of a slot pair (shifts 2 c and 2 c + 1 of the same bytes) exchanged; hmask_next_shift: the hmask
# bit of shift j + 1; plus_c2: n c1 + c2; scale_minus_31: code - 31
WRONG = {"Q2_K": ("groups_swapped", "plus_c2"), "Q3_K": ("groups_swapped", "hmask_next_shift", "scale_minus_31")}


def _group_of_element(wrong=None):
    """the scale group of every element of a super-block, [256]"""
    e = np.arange(256)
    h, j, l = e >> 7, (e >> 5) & 3, e & 31
    if wrong == "groups_swapped":
        j = j ^ 1
    return 8 * h + 2 * j + (l >> 4)


def _levels2(qs):
    """the 2-bit fields of qs [nsb, 64] in element order, [nsb, 256]"""
    q = qs.astype(np.int64).reshape(-1, 2, 1, 32)
    return ((q >> (2 * np.arange(4)).reshape(1, 1, 4, 1)) & 3).reshape(-1, 256)


def _hbits(hmask, wrong=None):
    """bit 4 h + j of hmask[l] for element 128 h + 32 j + l, [nsb, 256]"""
    e = np.arange(256)
    h, j, l = e >> 7, (e >> 5) & 3, e & 31
    if wrong == "hmask_next_shift":
        j = (j + 1) & 3
    return (hmask.astype(np.int64)[:, l] >> (4 * h + j)[None, :]) & 1


def weight_operands(raw, fmt, rows, k, wrong=None):
    """(A' f16 as float64, W exact float64, error bound of A' against W), each (len(rows), k), for the given weight rows of raw Q2_K /
    Q3_K blocks; wrong: a restatement that is subtly wrong in the named way (WRONG)"""
    assert fmt in FMTS and (wrong is None or wrong in WRONG[fmt]), (fmt, wrong)
    bb = 84 if fmt == "Q2_K" else 110
    rb = k // 256 * bb
    raw = np.ascontiguousarray(raw).view(np.uint8)
    blk = np.stack([raw[r * rb:(r + 1) * rb] for r in rows]).reshape(-1, bb)
    f16at = lambda a: blk[:, a:a + 2].copy().view(np.float16).astype(np.float64)[:, 0:1]  # noqa: E731
    grp = _group_of_element(wrong)
    if fmt == "Q2_K":
        d, dmin = f16at(80), f16at(82)
        s16 = blk[:, 0:16].astype(np.int64)
        n = _levels2(blk[:, 16:80]).astype(np.float64)
        dsc, dm = d * (s16 & 15)[:, grp], dmin * (s16 >> 4)[:, grp]
        c1, c2 = _f16(dsc).astype(np.float64), _f16(dm).astype(np.float64)
        w = n * dsc - dm
        ap = _f16(n * c1 + c2 if wrong == "plus_c2" else n * c1 - c2).astype(np.float64)
        ea = n * _u(dsc) + _u(dm) + _u(n * np.abs(c1) + np.abs(c2))
    else:
        d = f16at(108)
        code = q3k_scale_codes(blk[:, 96:108].astype(np.int64)) + 32  # (q3k_step_ref.scales gives code - 32)
        q = (_levels2(blk[:, 32:96]) - 4 * (1 - _hbits(blk[:, 0:32], wrong))).astype(np.float64)
        dsc = d * (code - (31 if wrong == "scale_minus_31" else 32))[:, grp]
        c = _f16(dsc).astype(np.float64)
        w = q * dsc
        ap = _f16(q * c).astype(np.float64)
        ea = np.abs(q) * _u(dsc) + _u(q * c)
    nr = len(rows)
    return ap.reshape(nr, k), w.reshape(nr, k), ea.reshape(nr, k)


def _q3k_pack_codes(code):
    """scales[12] of Q3_K from the sixteen 6-bit codes [nb, 16]: the inverse of the reference's aux[] shuffle"""
    code = np.asarray(code, np.int64)
    s12 = np.zeros((code.shape[0], 12), np.int64)
    for g in range(16):
        s12[:, g % 8] |= (code[:, g] & 15) << (4 * (g // 8))
        s12[:, 8 + g % 4] |= (code[:, g] >> 4) << (2 * (g // 4))
    return s12.astype(np.uint8)


def int_weights(rng, fmt, m, k):
    """blocks whose A' are small integers: d = dmin = 1, Q2_K scale codes 0..3 and minimums 0..7, Q3_K scale codes 30..34"""
    nb = m * k // 256
    one = np.array([1.0], np.float16).view(np.uint8)
    if fmt == "Q2_K":
        out = np.zeros((nb, 84), np.uint8)
        out[:, 0:16] = rng.integers(0, 4, (nb, 16)) | (rng.integers(0, 8, (nb, 16)) << 4)
        out[:, 16:80] = rng.integers(0, 256, (nb, 64))
        out[:, 80:82] = one
        out[:, 82:84] = one
    else:
        out = np.zeros((nb, 110), np.uint8)
        out[:, 0:96] = rng.integers(0, 256, (nb, 96))
        out[:, 96:108] = _q3k_pack_codes(rng.integers(30, 35, (nb, 16)))
        out[:, 108:110] = one
    return out.reshape(-1)


def code_blocks(rng, fmt):
    """64 super-blocks that between them hold every scale code in every group -- Q2_K: every 4-bit scale and minimum, Q3_K: every 6-bit
    code -- and, in every block, both hmask states and all four levels at every shift (random bits), with random f16 scales of either
    sign"""
    nb = 64
    raw = synth.random_blocks(rng, nb * 256, synth.TYPE_BY_NAME[fmt]).reshape(nb, -1).copy()
    i, g = np.arange(nb)[:, None], np.arange(16)[None, :]
    if fmt == "Q2_K":
        raw[:, 0:16] = ((i + g) % 16) | (((3 * i + 5 * g + 1) % 16) << 4)
        raw[:, 16:80] = rng.integers(0, 256, (nb, 64))
        raw[::2, 81] ^= 0x80
        raw[::3, 83] ^= 0x80
    else:
        raw[:, 96:108] = _q3k_pack_codes((i + 4 * g) % 64)
        raw[:, 0:96] = rng.integers(0, 256, (nb, 96))
        raw[::2, 109] ^= 0x80
    return raw.reshape(-1)


@contextlib.contextmanager
def q23k_operands():
    """tests/test_hip_f16w_gemm.py's checkers (check_exact, check_f16_operands, b_groups, upload, row_operands) read Q2_K and Q3_K
    inside this block: its weight_operands / int_weights dispatch here for the two formats, its tables know their rows and types"""
    saved = G.weight_operands, G.int_weights, G.KQ
    saved_tabs = dict(G.HT), dict(G.ROWS)

    def wo(raw, fmt, rows, k):
        return weight_operands(raw, fmt, rows, k) if fmt in FMTS else saved[0](raw, fmt, rows, k)

    def iw(rng, fmt, m, k):
        return int_weights(rng, fmt, m, k) if fmt in FMTS else saved[1](rng, fmt, m, k)

    G.weight_operands, G.int_weights, G.KQ = wo, iw, tuple(saved[2]) + FMTS
    G.HT.update(HT)
    G.ROWS.update({f: o.Q8_K for f in FMTS})
    try:
        yield
    finally:
        G.weight_operands, G.int_weights, G.KQ = saved
        for tab, old in ((G.HT, saved_tabs[0]), (G.ROWS, saved_tabs[1])):
            tab.clear()
            tab.update(old)


class _RowReaders:
    """what prefill_pass_ref calls Q5 inside q23k_pass: its row readers are q2k_step_ref's, which read Q2_K rows and hand every other
    format on to q3k_step_ref's (Q3_K), q5k_step_ref's (Q5_K) and fused_step_ref's own"""

    @staticmethod
    def q5k_rows():
        from tests import q2k_step_ref as Q2
        return Q2.q2k_rows()


@contextlib.contextmanager
def q23k_pass():
    """tests/prefill_pass_ref.py's check_pass reads passes over Q2_K / Q3_K bodies inside this block: q23k_operands for the f16 GEMM's
    operands and slot groups, B' of a Q2_K / Q3_K reader accepted by check_xh, the GEMV rows through q2k_step_ref / q3k_step_ref.
    Nothing else of the checker changes -- its bounds and its excused-share cap are its own"""
    from tests import prefill_pass_ref as P
    saved = P.weight_operands, P.check_xh, P.Q5
    saved_fmt = dict(P.F16W_FMT)
    orig_check_xh = P.check_xh

    def check_xh(res, tap, xh_name, act_name, ctx, model=None, wname=None):
        """prefill_pass_ref.check_xh; a Q8_K-row B' whose reader is Q2_K / Q3_K is held to the same multiset per super-block"""
        typ = model.tensors[wname].typ if (model is not None and xh_name in tap) else None
        if typ not in (synth.Q2_K, synth.Q3_K):
            return orig_check_xh(res, tap, xh_name, act_name, ctx, model, wname)
        acts = P.act_rows(tap, act_name)
        bits, _ = P.b_prime(acts)
        b, k = bits.shape
        fmt = P.F16W_FMT[typ]
        got = np.asarray(tap[xh_name], dtype=np.uint16).reshape(b, k)
        same = np.all(G.b_groups(got, fmt, b, k) == G.b_groups(bits, fmt, b, k), axis=2)
        if not same.all():
            r, blk = np.argwhere(~same)[0]
            res.fails.append(f"{ctx} {res.launch}: {xh_name} row {r} block {blk}: B' is not f16(q d) of the tapped planes ({int((~same).sum())} blocks)")

    with q23k_operands():
        P.weight_operands, P.check_xh, P.Q5 = G.weight_operands, check_xh, _RowReaders
        P.F16W_FMT.update({synth.Q2_K: "Q2_K", synth.Q3_K: "Q3_K"})
        try:
            yield
        finally:
            P.weight_operands, P.check_xh, P.Q5 = saved
            P.F16W_FMT.clear()
            P.F16W_FMT.update(saved_fmt)
