"""The Q5_K form of k_gemm_f16w (gemm_f16w.hip: WF_Q5_K) by itself, through crabml_hip_debug_gemm_f16w.

  A' = f16(q c1 - c2), c1 = f16(d sc), c2 = f16(dmin m), q = nibble + 16 (qh bit) = 0..31                       (three roundings)
  B' = f16(q d) of the Q8_K rows (q d in f32 first), in the k-slot order Q2_K / Q3_K read
restated in element order by tests/q5k_f16w_ref.py.  The checks are the three tiers and the range edges of
tests/test_hip_f16w_gemm.py, run by that file's own functions with the format substituted (q5k_f16w_ref.q5k_operands): exact integers
bit for bit over every (F, T) instance, the k pieces, three matrices in one launch with both B' writers and the gate | up form; the f16
operands summed in float64; the derived bound against float64 of the dequantized operation; junk behind the live B'; the B' overflow
flag; weight scales that put A' past 65504.  (The prompt pass sends a Q5_K matrix to this kernel only in a context created with
CRABML_HIP_LLAMA_PREFILL_Q5K_GEMM: tests/test_hip_prefill_q5k_launches.py.)"""
import numpy as np
import pytest

from crabml_amd import synth
from tests import q5k_f16w_ref as Q
from tests import test_hip_f16w_gemm as G

pytestmark = pytest.mark.gpu
FMT = Q.FMT


def test_exact_integer_operands_give_the_integer_dot_bit_for_bit(ca, hdev):
    """tier 1: every (F, T) instance at ksplit 1 over SHAPES_K, ksplit 2 / 4 / 8 at k = 4096 and 2048, three matrices of different m in
    one launch with both B' writers"""
    with Q.q5k_operands():
        G.test_exact_integer_operands_give_the_integer_dot_bit_for_bit(ca, hdev, FMT)


def test_gate_up_form(ca, hdev):
    """the gate | up instances: exact integers through the plain two-matrix launch of every T, and h = silu(g) * u of the epilogue
    equal to the plain launch's g and u, bit for bit"""
    with Q.q5k_operands():
        for i, (m, k, b, T) in enumerate(((128, 512, 33, 2), (192, 1024, 65, 4), (64, 2048, 200, 8))):
            r = G.check_exact(ca, hdev, FMT, [m, m], k, b, (2, T, 1, 0), 500 + i)
            assert r["used"] == (2, T, 1, 0)
        G.test_gate_up_epilogue_is_silu_mul_of_the_plain_launch(ca, hdev, FMT)


def test_f16_operands_summed_in_float64_and_the_dequantized_operation(ca, hdev):
    """tiers 2 and 3 (check_f16_operands holds every launch to both): random blocks over the (F, T) instances and the k pieces, then
    the blocks that hit every scale and minimum code in every sub-block and both qh states at every pair and nibble, with scales of
    either sign"""
    with Q.q5k_operands():
        G.test_f16_operands_summed_in_float64(ca, hdev, FMT)
        rng = np.random.default_rng(61)
        raw = Q.code_blocks(rng)  # 64 super-blocks: 16 rows of k = 1024
        for force, b in (((1, 2, 1, 0), 17), ((2, 8, 1, 0), 130), ((0, 0, 0, -1), 64)):
            G.check_f16_operands(ca, hdev, FMT, 16, 1024, b, force, 70 + b, raw=raw)


def test_matches_the_dequantized_operation_through_the_launchers_own_form(ca, hdev):
    """tier 3 through the launcher's own choice of F, T and k pieces, at shapes where it takes two fragments (wide), k pieces (long
    rows) and neither.  The bound per output is test_hip_f16w_gemm.test_matches_the_dequantized_operation's, with A' - W from
    q5k_f16w_ref: q u(d sc) + u(dmin m) + u(q |c1| + |c2|)."""
    rng = np.random.default_rng(3)
    with Q.q5k_operands():
        seen = []
        for (m, k, b) in ((8192, 512, 512), (256, 4096, 200), (64, 1024, 40)):
            x = (rng.standard_normal(b * k) * rng.uniform(0.1, 4.0)).astype(np.float32)
            r = G.check_f16_operands(ca, hdev, FMT, m, k, b, (0, 0, 0, -1), m + b, x=x)
            seen.append(tuple(r["used"][:3]))
        assert any(u[0] == 2 for u in seen) and any(u[2] > 1 for u in seen) and len({u[1] for u in seen}) > 1, seen


def test_junk_behind_the_live_rows_does_not_matter(ca, hdev):
    with Q.q5k_operands():
        G.test_junk_behind_the_live_rows_does_not_matter(ca, hdev, FMT)


def test_overflow_flag_is_raised_exactly_when_a_b_value_is_inf(ca, hdev):
    with Q.q5k_operands():
        G.test_overflow_flag_is_raised_exactly_when_a_b_value_is_inf(ca, hdev, FMT)


# (d, dmin) of one block -- every value an f16 -- and whether the matrix must be refused: 31 |f16(63 d)| + |f16(63 dmin)| against 65504.
# f16 has steps of 2 from 2048, of 1 / 32 from 32 and of 32 from 32768.  63 * 33.53125 = 2112.47 -> 2112, times 31 = 65472; plus
# 63 * 0.5 = 31.5: 65503.5 (taken: A' = f16(65503.5) = 65504, the largest f16); plus 63 * 0.53125 = 33.46875: 65505.47 (refused).
# 63 * 33.5625 = 2114.44 -> 2114, times 31 = 65534 (refused).  f16(0.01) = 0.010002, times 63 = 0.6301, times 31 = 19.5;
# 63 * 1039 = 65457 -> 65472, plus 19.5: 65491.5 (taken); 63 * 1041 = 65583 -> inf (refused).
EDGE = [((33.53125, 0.5), False), ((33.53125, 0.53125), True), ((33.5625, 0.0), True), ((0.01, 1039.0), False), ((0.01, 1041.0), True),
        ((np.inf, 0.0), True), ((0.01, np.inf), True), ((np.nan, 0.0), True), ((0.01, np.nan), True)]


def test_weight_scales_that_put_a_past_f16_are_refused(ca, hdev):
    """one super-block with the largest codes (63, 63) and levels (31) whose scales can make |A'| > 65504, or are not finite: the
    launcher does not take the matrix; the in-range neighbour is taken and stays finite -- for either sign of the scales (d and dmin of
    opposite signs: the magnitudes of q c1 and c2 add)"""
    rng = np.random.default_rng(29)
    m, k, b = 64, 512, 33
    x = rng.standard_normal(b * k).astype(np.float32)
    with Q.q5k_operands():
        for (d, dmin), refused in EDGE:
            for sign in (1.0, -1.0):
                raw = synth.random_blocks(rng, m * k, synth.Q5_K).reshape(-1, 176).copy()
                raw[7, 0:160] = 0xFF  # nibble 15 and fifth bit 1 everywhere: q = 31
                raw[7, 160:172] = Q.pack_codes(np.full((1, 8), 63), np.full((1, 8), 63))[0]
                with np.errstate(invalid="ignore"):
                    raw[7, 172:174] = np.array([sign * d], np.float16).view(np.uint8)
                    raw[7, 174:176] = np.array([-sign * dmin], np.float16).view(np.uint8)
                w = G.upload(ca, hdev, raw.reshape(-1), FMT, m, k)
                if refused:
                    with pytest.raises(Exception, match="refused"):
                        G.run(ca, hdev, [w], x, b, k, (1, 4, 1, 0))
                else:
                    out = G.run(ca, hdev, [w], x, b, k, (1, 4, 1, 0))["out"][0]
                    assert np.all(np.isfinite(out)), (d, dmin, sign)
                    ap = G.weight_operands(raw.reshape(-1), FMT, range(m), k)[0]
                    assert np.all(np.isfinite(ap)) and np.abs(ap).max() > 6.0e4, "the accepted neighbour must reach the edge of f16"
