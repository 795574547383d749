"""The Q2_K and Q3_K forms of k_gemm_f16w (gemm_f16w.hip) by themselves, through crabml_hip_debug_gemm_f16w.

  A' = f16(n c1 - c2), c1 = f16(d (sc & 15)), c2 = f16(dmin (sc >> 4)), n = 0..3                          Q2_K (three roundings)
  A' = f16(q c), c = f16(d (code - 32)), q = low2 - (hbit ? 0 : 4) = -4..3                               Q3_K (two roundings)
  B' = f16(q d) of the Q8_K rows (q d in f32 first), ONE k-slot order for both formats
restated in element order by tests/q23k_f16w_ref.py.  The checks are the three tiers and the range edges of
tests/test_hip_f16w_gemm.py, run by that file's own functions with the two formats substituted (q23k_f16w_ref.q23k_operands): exact
integers bit for bit over every (F, T) instance, the k pieces, three matrices in one launch with both B' writers and the gate | up
form; the f16 operands summed in float64; the derived bound against float64 of the dequantized operation; junk behind the live B';
the B' overflow flag; weight scales that put A' past 65504."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import q23k_f16w_ref as Q
from tests import test_hip_f16w_gemm as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_exact_integer_operands_give_the_integer_dot_bit_for_bit(ca, hdev, fmt):
    """tier 1: every (F, T) instance at ksplit 1 over SHAPES_K, ksplit 2 / 4 / 8 at k = 4096 and 2048, three matrices of different m in
    one launch with both B' writers"""
    with Q.q23k_operands():
        G.test_exact_integer_operands_give_the_integer_dot_bit_for_bit(ca, hdev, fmt)


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_gate_up_form(ca, hdev, fmt):
    """the gate | up instances: exact integers through the plain two-matrix launch of every T, and h = silu(g) * u of the epilogue
    equal to the plain launch's g and u, bit for bit"""
    with Q.q23k_operands():
        for i, (m, k, b, T) in enumerate(((128, 512, 33, 2), (192, 1024, 65, 4), (64, 2048, 200, 8))):
            r = G.check_exact(ca, hdev, fmt, [m, m], k, b, (2, T, 1, 0), 500 + i)
            assert r["used"] == (2, T, 1, 0)
        G.test_gate_up_epilogue_is_silu_mul_of_the_plain_launch(ca, hdev, fmt)


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_f16_operands_summed_in_float64_and_the_dequantized_operation(ca, hdev, fmt):
    """tiers 2 and 3 (check_f16_operands holds every launch to both): random blocks over the (F, T) instances and the k pieces, then
    the blocks that hit every scale code and both hmask states at every shift, with scales of either sign"""
    with Q.q23k_operands():
        G.test_f16_operands_summed_in_float64(ca, hdev, fmt)
        rng = np.random.default_rng(61)
        raw = Q.code_blocks(rng, fmt)  # 64 super-blocks: 16 rows of k = 1024
        for force, b in (((1, 2, 1, 0), 17), ((2, 8, 1, 0), 130), ((0, 0, 0, -1), 64)):
            G.check_f16_operands(ca, hdev, fmt, 16, 1024, b, force, 70 + b, raw=raw)


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_matches_the_dequantized_operation_through_the_launchers_own_form(ca, hdev, fmt):
    """tier 3 through the launcher's own choice of F, T and k pieces, at shapes where it takes two fragments (wide), k pieces (long
    rows) and neither.  The bound per output is test_hip_f16w_gemm.test_matches_the_dequantized_operation's, with A' - W from
    q23k_f16w_ref: Q2_K n u(d sc) + u(dmin m) + u(n |c1| + |c2|), Q3_K |q| u(d sc) + u(q c)."""
    rng = np.random.default_rng(3)
    with Q.q23k_operands():
        seen = []
        for (m, k, b) in ((8192, 512, 512), (256, 4096, 200), (64, 1024, 40)):
            x = (rng.standard_normal(b * k) * rng.uniform(0.1, 4.0)).astype(np.float32)
            r = G.check_f16_operands(ca, hdev, fmt, m, k, b, (0, 0, 0, -1), m + b, x=x)
            seen.append(tuple(r["used"][:3]))
        assert any(u[0] == 2 for u in seen) and any(u[2] > 1 for u in seen) and len({u[1] for u in seen}) > 1, seen


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_junk_behind_the_live_rows_does_not_matter(ca, hdev, fmt):
    with Q.q23k_operands():
        G.test_junk_behind_the_live_rows_does_not_matter(ca, hdev, fmt)


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_overflow_flag_is_raised_exactly_when_a_b_value_is_inf(ca, hdev, fmt):
    with Q.q23k_operands():
        G.test_overflow_flag_is_raised_exactly_when_a_b_value_is_inf(ca, hdev, fmt)


# (d, dmin) of one block and whether the matrix must be refused.  Q2_K: 3 |f16(15 d)| + |f16(15 dmin)| against 65504 -- f16(15 * 1460) =
# 21904, times 3 = 65712; f16(15 * 1450) = 21744, times 3 = 65232, plus 15 * 16 = 240: 65472, plus 15 * 20 = 300: 65532.  Q3_K:
# 4 |f16(32 d)| -- 32 * 512 = 16384, times 4 = 65536; 32 * 511.5 = 16368, times 4 = 65472.
EDGE = {"Q2_K": [((1460.0, 0.0), True), ((1450.0, 16.0), False), ((1450.0, 20.0), True), ((0.01, 4400.0), True), ((0.01, 4300.0), False),
                 ((np.inf, 0.0), True), ((0.01, np.nan), True)],
        "Q3_K": [((512.0, None), True), ((511.5, None), False), ((np.inf, None), True), ((np.nan, None), True)]}


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_weight_scales_that_put_a_past_f16_are_refused(ca, hdev, fmt):
    """one super-block whose scales can make |A'| > 65504, or are not finite: the launcher does not take the matrix; the in-range
    neighbour is taken and stays finite -- for either sign of the scales, with the largest scale codes in the block"""
    rng = np.random.default_rng(29)
    m, k, b = 64, 512, 33
    typ = synth.TYPE_BY_NAME[fmt]
    bb = o.BLOCK_BYTES[typ]
    x = rng.standard_normal(b * k).astype(np.float32)
    with Q.q23k_operands():
        for (d, dmin), refused in EDGE[fmt]:
            for sign in (1.0, -1.0):
                raw = synth.random_blocks(rng, m * k, typ).reshape(-1, bb).copy()
                if fmt == "Q2_K":
                    raw[7, 0:16] = 0xFF  # scale 15, minimum 15
                    raw[7, 80:82] = np.array([sign * d], np.float16).view(np.uint8)
                    raw[7, 82:84] = np.array([-sign * dmin], np.float16).view(np.uint8)
                else:
                    raw[7, 96:108] = Q._q3k_pack_codes(np.zeros((1, 16), np.int64))[0]  # code 0: |code - 32| = 32
                    raw[7, 0:32] = 0  # hbit 0 and
                    raw[7, 32:96] = 0  # low2 0: q = -4
                    raw[7, 108:110] = np.array([sign * d], np.float16).view(np.uint8)
                w = G.upload(ca, hdev, raw.reshape(-1), fmt, m, k)
                if refused:
                    with pytest.raises(Exception, match="refused"):
                        G.run(ca, hdev, [w], x, b, k, (1, 4, 1, 0))
                else:
                    out = G.run(ca, hdev, [w], x, b, k, (1, 4, 1, 0))["out"][0]
                    assert np.all(np.isfinite(out)), (fmt, d, dmin, sign)
                    ap = G.weight_operands(raw.reshape(-1), fmt, range(m), k)[0]
                    assert np.all(np.isfinite(ap)) and np.abs(ap).max() > 6.0e4, "the accepted neighbour must reach the edge of f16"
