"""The Q5_0 and Q5_1 forms of k_gemm_f16w (gemm_f16w.hip: WF_Q5_0 / WF_Q5_1) restated in numpy, in ELEMENT order, for the tests of the
kernel (tests/test_hip_f16w_gemm_q5_01.py) and of the prompt pass that runs it (tests/test_hip_prefill_q5_01.py).

  Q5_0 block (buf_q5_0.rs:13-19): d f16 | qh u32 | qs[16].  Element i < 16 has the level q5 = (qs[i] & 15) | bit i of qh << 4, element
      16 + i the level (qs[i] >> 4) | bit 16 + i of qh << 4; W = (q5 - 16) d.
      The kernel: 0x6400 | nibble | fifth bit << 4 is the f16 number 1024 + q5, -1040 makes it q5 - 16 exactly, then one product:
      A' = f16((q5 - 16) d), ONE rounding, |A' - W| <= u(W).
  Q5_1 block (buf_q5_1.rs:10-17): d f16 | m f16 | qh u32 | qs[16], the same levels; W = q5 d + m.
      The kernel: -1024 makes q5 exactly, then one v_pk_fma_f16: A' = f16(q5 d + m), ONE rounding, |A' - W| <= u(W).
  u(v) = max(2^-11 |v|, 2^-25): one f16 rounding of the exact value v (tests/test_hip_f16w_gemm.py).
  B' is Q4_0's / Q4_1's: f16(q d) of the Q8_0 / Q8_1 rows in slot order 0.

The levels are tests/q5_01_step_ref.levels (one restatement of the unpack for the decode step's checker and this one)."""
import contextlib

import numpy as np

from crabml_amd import synth
from oracle import oracle as o
from tests import test_hip_f16w_gemm as G
from tests.q5_01_step_ref import WRONG, levels
from tests.test_hip_f16w_gemm import _f16, _u

FMTS = ["Q5_0", "Q5_1"]


def _fields(raw, fmt, rows, k, wrong=None):
    typ = synth.TYPE_BY_NAME[fmt]
    bb = o.BLOCK_BYTES[typ]
    rb = k // 32 * bb
    raw = np.ascontiguousarray(raw).view(np.uint8)
    blk = np.stack([raw[r * rb:(r + 1) * rb] for r in rows]).reshape(-1, bb)
    h = 2 if fmt == "Q5_0" else 4
    f16at = lambda a: blk[:, a:a + 2].copy().view(np.float16).astype(np.float64)[:, 0:1]  # noqa: E731
    nr, nb = len(rows), k // 32
    qh = np.ascontiguousarray(blk[:, h:h + 4]).view("<u4")[:, 0].reshape(nr, nb)  # (per row: a neighbour is the next block of the ROW)
    lv = levels(blk[:, h + 4:].reshape(nr, nb, 16), qh, wrong).astype(np.float64).reshape(-1, 32)
    d = f16at(0)
    if wrong == "scale_neighbour":
        d = np.roll(d.reshape(nr, nb), -1, axis=1).reshape(-1, 1)
    return d, (f16at(2) if fmt == "Q5_1" else None), lv


def weight_operands(raw, fmt, rows, k, wrong=None):
    """(A' f16 as float64, W exact float64, error bound of A' against W), each (len(rows), k); wrong: the operands of a kernel whose
    loader is subtly wrong in the named way (q5_01_step_ref.WRONG: the checker's own tests)"""
    assert fmt in FMTS and (wrong is None or wrong in WRONG), (fmt, wrong)
    d, m, q = _fields(raw, fmt, rows, k, wrong)
    off = wrong == "offset_dropped"
    with np.errstate(invalid="ignore", over="ignore"):
        w = (q - (0.0 if off else 16.0)) * d if fmt == "Q5_0" else q * d + (m * 0.0 if off else m)
    nr = len(rows)
    return _f16(w).astype(np.float64).reshape(nr, k), w.reshape(nr, k), _u(w).reshape(nr, k)


def int_weights(rng, fmt, m, k):
    """blocks whose A' are small integers: d = 1 (Q5_1: m = 0 .. -8), random nibbles and fifth bits"""
    assert fmt in FMTS, fmt
    typ = synth.TYPE_BY_NAME[fmt]
    nb = m * k // 32
    out = np.zeros((nb, o.BLOCK_BYTES[typ]), np.uint8)
    out[:, 0:2] = np.array([1.0], np.float16).view(np.uint8)
    h = 2
    if fmt == "Q5_1":
        out[:, 2:4] = (-rng.integers(0, 9, nb)).astype(np.float16).view(np.uint8).reshape(nb, 2)
        h = 4
    out[:, h:] = rng.integers(0, 256, (nb, 20))
    return out.reshape(-1)


def edge_level_blocks(rng, fmt, m, k):
    """random blocks with scales of either sign, and among them blocks whose fifth bits are all set, all clear and alternating, with the
    nibbles at 0 and at 15: levels 0, 15, 16 and 31 next to each other"""
    typ = synth.TYPE_BY_NAME[fmt]
    raw = synth.random_blocks(rng, m * k, typ).reshape(-1, o.BLOCK_BYTES[typ]).copy()
    h = 2 if fmt == "Q5_0" else 4
    raw[::2, 1] ^= 0x80
    for i, (qh, qs) in enumerate(((0xFF, 0xFF), (0x00, 0x00), (0x55, 0xF0), (0xAA, 0x0F), (0xFF, 0x00), (0x00, 0xFF))):
        raw[i::16, h:h + 4] = qh
        raw[i::16, h + 4:] = qs
    return raw.reshape(-1)


def refuse_matrix(model, wname, block=37):
    """one block of the named Q5_0 / Q5_1 tensor rewritten so that the f16 GEMM's range check refuses the matrix while every weight of
    the block is exactly 0 (the edge values of tests/test_hip_f16w_gemm_q5_01.EDGE):
      Q5_0: d = 4096, qh = 0xFFFFFFFF, qs = 0 -- every level is 16, (16 - 16) d = 0, yet 16 |d| = 65536 > 65504;
      Q5_1: d = 2114, m = 0, qh = 0, qs = 0 -- every level is 0, 0 d + 0 = 0, yet f16(31 * 2114 = 65534) is inf.
    The matrix then takes the row-by-row GEMV inside a pass whose other matrices take the GEMM, and its values stay ordinary"""
    t = model.tensors[wname]
    fmt = synth.TYPE_NAMES[t.typ]
    assert fmt in FMTS, (wname, fmt)
    blk = np.array(t.data, dtype=np.uint8).reshape(-1, o.BLOCK_BYTES[t.typ])
    assert block < blk.shape[0]
    blk[block] = 0
    if fmt == "Q5_0":
        blk[block, 0:2] = np.array([4096.0], np.float16).view(np.uint8)
        blk[block, 2:6] = 0xFF
    else:
        blk[block, 0:2] = np.array([2114.0], np.float16).view(np.uint8)
    t.data = blk.reshape(-1)
    w = weight_operands(t.data, fmt, [block * 32 // t.shape[1]], t.shape[1])[1].reshape(-1, 32)[block % (t.shape[1] // 32)]
    assert np.all(w == 0.0), w
    return model


@contextlib.contextmanager
def q5_01_operands():
    """tests/test_hip_f16w_gemm.py's checkers read Q5_0 and Q5_1 inside this block"""
    saved = G.weight_operands, G.int_weights
    saved_tabs = dict(G.HT), dict(G.ROWS)

    def wo(raw, fmt, rows, k):
        return weight_operands(raw, fmt, rows, k) if fmt in FMTS else saved[0](raw, fmt, rows, k)

    def iw(rng, fmt, m, k):
        return int_weights(rng, fmt, m, k) if fmt in FMTS else saved[1](rng, fmt, m, k)

    G.weight_operands, G.int_weights = wo, iw
    G.HT.update({"Q5_0": "Q5_0", "Q5_1": "Q5_1"})
    G.ROWS.update({"Q5_0": o.Q8_0, "Q5_1": o.Q8_1})
    try:
        yield
    finally:
        G.weight_operands, G.int_weights = saved
        for tab, old in ((G.HT, saved_tabs[0]), (G.ROWS, saved_tabs[1])):
            tab.clear()
            tab.update(old)


class _RowReaders:
    """what prefill_pass_ref calls Q5 inside q5_01_pass: its row readers are q5_01_step_ref's, which read Q5_0 / Q5_1 rows and hand every
    other format on to fused_step_ref's own"""

    @staticmethod
    def q5k_rows():
        from tests import q5_01_step_ref as S
        return S.q5_rows()


@contextlib.contextmanager
def q5_01_pass():
    """tests/prefill_pass_ref.py's check_pass reads passes over Q5_0 / Q5_1 bodies inside this block: q5_01_operands for the f16 GEMM's A',
    the two formats in F16W_FMT, the GEMV and classifier rows through q5_01_step_ref.q5_rows.  B' is Q4_0's 32-element-block multiset,
    as check_xh already holds it for Q8_0 / Q8_1 rows.  Nothing else of the checker changes -- its bounds and its excused-share cap are
    its own"""
    from tests import prefill_pass_ref as P
    saved = P.weight_operands, P.Q5
    saved_fmt = dict(P.F16W_FMT)
    with q5_01_operands():
        P.weight_operands, P.Q5 = G.weight_operands, _RowReaders
        P.F16W_FMT.update({synth.Q5_0: "Q5_0", synth.Q5_1: "Q5_1"})
        try:
            yield
        finally:
            P.weight_operands, P.Q5 = saved
            P.F16W_FMT.clear()
            P.F16W_FMT.update(saved_fmt)
