"""The Q5_0 and Q5_1 forms of k_gemm_f16w (gemm_f16w.hip) by themselves, through crabml_hip_debug_gemm_f16w.

  A' = f16((q5 - 16) d)       Q5_0 (one rounding)          A' = f16(q5 d + m)       Q5_1 (one v_pk_fma_f16, one rounding)
  B' = f16(q d) of the Q8_0 / Q8_1 rows, Q4_0's k-slot order
restated in element order by tests/q5_01_f16w_ref.py.  The checks are the three tiers and the range edges of
tests/test_hip_f16w_gemm.py, run by that file's own functions with the two formats substituted (q5_01_f16w_ref.q5_01_operands): exact
integers bit for bit over every (F, T) instance, the k pieces, three matrices in one launch with both B' writers and the gate | up
form; the f16 operands summed in float64; the derived bound against float64 of the dequantized operation; junk behind the live B';
the B' overflow flag; weight scales that put A' past 65504."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import q5_01_f16w_ref as Q
from tests import test_hip_f16w_gemm as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_exact_integer_operands_give_the_integer_dot_bit_for_bit(ca, hdev, fmt):
    """tier 1: every (F, T) instance at ksplit 1 over SHAPES_Q, the k pieces, three matrices of different m in one launch with both
    B' writers"""
    with Q.q5_01_operands():
        G.test_exact_integer_operands_give_the_integer_dot_bit_for_bit(ca, hdev, fmt)


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_gate_up_form(ca, hdev, fmt):
    """the gate | up instances: exact integers through the plain two-matrix launch of every T, and h = silu(g) * u of the epilogue
    equal to the plain launch's g and u, bit for bit"""
    with Q.q5_01_operands():
        for i, (m, k, b, T) in enumerate(((128, 288, 33, 2), (192, 1024, 65, 4), (64, 2080, 200, 8))):
            r = G.check_exact(ca, hdev, fmt, [m, m], k, b, (2, T, 1, 0), 500 + i)
            assert r["used"] == (2, T, 1, 0)
        G.test_gate_up_epilogue_is_silu_mul_of_the_plain_launch(ca, hdev, fmt)


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_f16_operands_summed_in_float64_and_the_dequantized_operation(ca, hdev, fmt):
    """tiers 2 and 3 (check_f16_operands holds every launch to both): random blocks over the (F, T) instances and the k pieces, then
    blocks with every fifth bit set, none, alternating, the nibbles at 0 and 15 (levels 0, 15, 16, 31) and scales of either sign"""
    with Q.q5_01_operands():
        G.test_f16_operands_summed_in_float64(ca, hdev, fmt)
        rng = np.random.default_rng(61)
        raw = Q.edge_level_blocks(rng, fmt, 16, 1056)  # 33 blocks per row: a ragged last chunk
        for force, b in (((1, 2, 1, 0), 17), ((2, 8, 1, 0), 130), ((0, 0, 0, -1), 64)):
            G.check_f16_operands(ca, hdev, fmt, 16, 1056, b, force, 70 + b, raw=raw)


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_matches_the_dequantized_operation_through_the_launchers_own_form(ca, hdev, fmt):
    """tier 3 through the launcher's own choice of F, T and k pieces, at shapes where it takes two fragments (wide), k pieces (long
    rows) and neither; A' - W is one f16 rounding of (q5 - 16) d / of q5 d + m"""
    rng = np.random.default_rng(3)
    with Q.q5_01_operands():
        seen = []
        for (m, k, b) in ((8192, 512, 512), (256, 4096, 200), (64, 1024, 40)):
            x = (rng.standard_normal(b * k) * rng.uniform(0.1, 4.0)).astype(np.float32)
            r = G.check_f16_operands(ca, hdev, fmt, m, k, b, (0, 0, 0, -1), m + b, x=x)
            seen.append(tuple(r["used"][:3]))
        assert any(u[0] == 2 for u in seen) and any(u[2] > 1 for u in seen) and len({u[1] for u in seen}) > 1, seen


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_junk_behind_the_live_rows_does_not_matter(ca, hdev, fmt):
    with Q.q5_01_operands():
        G.test_junk_behind_the_live_rows_does_not_matter(ca, hdev, fmt)


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_overflow_flag_is_raised_exactly_when_a_b_value_is_inf(ca, hdev, fmt):
    with Q.q5_01_operands():
        G.test_overflow_flag_is_raised_exactly_when_a_b_value_is_inf(ca, hdev, fmt)


# (d, m) of one block and whether the matrix must be refused, derived by hand.
# Q5_0: the largest |A'| is 16 |d| (level 0), an exact product: 16 * 4094 = 65504, the largest f16 -- taken; the next f16 above 4094 is
#   4096: 65536 -- refused.
# Q5_1: A' = f16(q5 d + m) is linear in q5 = 0 .. 31, so the largest is at an end: |m| (finite f16: always in range) or |f16(31 d + m)|,
#   which is inf from 65520 on (the midpoint between 65504 and 2^16; ties go to the even mantissa, which is 2^16's).  d = 2048:
#   31 d = 63488; m = 2031 gives 65519 -> 65504, taken; its f16 neighbour m = 2032 gives 65520 -> inf, refused.  m = 0: d = 2112 gives
#   65472, taken; its f16 neighbour d = 2114 gives 65534 -> inf, refused.  Opposite signs: d = 4000, m = -60000 gives 64000 at level 31
#   and -60000 at level 0, taken (31 |d| + |m| would be far outside: the range is that of the values, not of their magnitudes).
EDGE = {"Q5_0": [((4096.0, None), True), ((4094.0, None), False), ((np.inf, None), True), ((np.nan, None), True)],
        "Q5_1": [((2048.0, 2032.0), True), ((2048.0, 2031.0), False), ((2114.0, 0.0), True), ((2112.0, 0.0), False),
                 ((4000.0, -60000.0), False), ((np.inf, 0.0), True), ((1.0, np.inf), True), ((np.nan, 0.0), True), ((1.0, np.nan), True)]}


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_weight_scales_that_put_a_past_f16_are_refused(ca, hdev, fmt):
    """one block whose scales can make |A'| > 65504, or are not finite: the launcher does not take the matrix; the in-range
    neighbour is taken and stays finite -- for either sign of the scales, with levels 0 and 31 in the block"""
    rng = np.random.default_rng(29)
    m, k, b = 64, 512, 33
    typ = synth.TYPE_BY_NAME[fmt]
    bb = o.BLOCK_BYTES[typ]
    h = 2 if fmt == "Q5_0" else 4
    x = rng.standard_normal(b * k).astype(np.float32)
    with Q.q5_01_operands():
        for (d, mm), refused in EDGE[fmt]:
            for sign in (1.0, -1.0):
                raw = synth.random_blocks(rng, m * k, typ).reshape(-1, bb).copy()
                raw[7, h:h + 2] = 0x00      # elements 0-15 without their fifth bit and with nibble 0: level 0,
                raw[7, h + 2:h + 4] = 0xFF  # elements 16-31 with it and with nibble 15: level 31
                raw[7, h + 4:] = 0xF0
                raw[7, 0:2] = np.array([sign * d], np.float16).view(np.uint8)
                if fmt == "Q5_1":
                    raw[7, 2:4] = np.array([sign * mm], np.float16).view(np.uint8)
                w = G.upload(ca, hdev, raw.reshape(-1), fmt, m, k)
                if refused:
                    with pytest.raises(Exception, match="refused"):
                        G.run(ca, hdev, [w], x, b, k, (1, 4, 1, 0))
                else:
                    out = G.run(ca, hdev, [w], x, b, k, (1, 4, 1, 0))["out"][0]
                    assert np.all(np.isfinite(out)), (fmt, d, mm, sign)
                    ap = G.weight_operands(raw.reshape(-1), fmt, range(m), k)[0]
                    assert np.all(np.isfinite(ap)) and np.abs(ap).max() > 6.0e4, "the accepted neighbour must reach the edge of f16"
