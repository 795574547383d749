"""tests/q23k_f16w_ref.py checked on the CPU: the numpy restatement of the Q2_K / Q3_K forms of k_gemm_f16w dequantizes like the oracle,
its A' stays inside the stated bound, its integer generators give integers, and single mutations of it are told apart from it on the
inputs the GPU tests use."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import q23k_f16w_ref as Q
from tests import test_hip_f16w_gemm as G


def _inputs(fmt):
    rng = np.random.default_rng(7 if fmt == "Q2_K" else 9)
    typ = synth.TYPE_BY_NAME[fmt]
    return {"random": synth.random_blocks(rng, 64 * 256, typ), "codes": Q.code_blocks(rng, fmt), "ints": Q.int_weights(rng, fmt, 8, 2048)}


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_w_is_the_oracles_dequantize_and_a_is_inside_the_bound(fmt):
    typ = synth.TYPE_BY_NAME[fmt]
    for name, raw in _inputs(fmt).items():
        n = raw.size // o.BLOCK_BYTES[typ] * 256
        ap, w, ea = Q.weight_operands(raw, fmt, range(n // 256), 256)
        ref = o.dequantize(raw, typ).reshape(-1, 256)
        # (the oracle returns f32: d (code - 32) q is exact there, and d sc n and dmin m are, so that their difference rounds once)
        assert np.array_equal(w.astype(np.float32), ref), (fmt, name, np.max(np.abs(w - ref)))
        assert np.all(np.isfinite(ap)) and np.all(np.abs(ap - w) <= ea), (fmt, name, np.max(np.abs(ap - w) / ea))


def test_code_blocks_hit_every_scale_code_and_both_hmask_states_at_every_shift():
    rng = np.random.default_rng(3)
    b2 = Q.code_blocks(rng, "Q2_K").reshape(-1, 84)
    for g in range(16):
        assert set(b2[:, g] & 15) == set(range(16)) and set(b2[:, g] >> 4) == set(range(16)), g
    b3 = Q.code_blocks(rng, "Q3_K").reshape(-1, 110)
    from tests.q3k_step_ref import scales
    code = scales(b3[:, 96:108].astype(np.int64)) + 32
    seen = set()
    for g in range(16):
        seen |= set(code[:, g])
    assert seen == set(range(64))
    hb = Q._hbits(b3[:, 0:32]).reshape(-1, 2, 4, 32)
    lv = Q._levels2(b3[:, 32:96]).reshape(-1, 2, 4, 32)
    for h in range(2):
        for j in range(4):
            assert set(hb[:, h, j].reshape(-1)) == {0, 1} and set(lv[:, h, j].reshape(-1)) == {0, 1, 2, 3}, (h, j)
    # either sign of d (Q2_K: and of dmin)
    assert {0, 0x80} == set(b3[:, 109] & 0x80) == set(b2[:, 81] & 0x80) == set(b2[:, 83] & 0x80)


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_integer_generators_give_integer_operands(fmt):
    rng = np.random.default_rng(5)
    raw = Q.int_weights(rng, fmt, 4, 1024)
    ap, w, ea = Q.weight_operands(raw, fmt, range(4), 1024)
    assert np.all(ap == np.round(ap)) and np.array_equal(ap, w)
    assert np.abs(ap).max() <= (3 * 3 + 7 if fmt == "Q2_K" else 4 * 2) and np.abs(ap).max() >= 6
    with Q.q23k_operands():  # ... and through the existing checker's dispatch, with rows that quantize to themselves
        assert np.array_equal(G.weight_operands(raw, fmt, range(4), 1024)[0], ap)
        xi = G.int_rows(rng, fmt, 2, 1024)
        assert np.array_equal(G.row_operands(xi, fmt, 2, 1024)[0], xi.reshape(2, 1024).astype(np.float64))
    assert "Q2_K" not in G.ROWS and "Q3_K" not in G.HT and G.KQ == ("Q4_K", "Q6_K")  # (the substitution ends with the block)


@pytest.mark.parametrize("fmt,wrong", [(f, w) for f in Q.FMTS for w in Q.WRONG[f]])
def test_single_mutations_are_told_apart(fmt, wrong):
    """every mutation changes A' on every kind of input the GPU tests use: on the integer blocks the exact tier's integer dot moves (small
    integer rows against the row), on the random and the code blocks A' leaves the bound against W"""
    for name, raw in _inputs(fmt).items():
        nsb = raw.size // (84 if fmt == "Q2_K" else 110)
        ap, w, ea = Q.weight_operands(raw, fmt, range(nsb), 256)
        bad = Q.weight_operands(raw, fmt, range(nsb), 256, wrong)[0]
        assert not np.array_equal(ap, bad), (fmt, wrong, name)
        if name == "ints":
            x = np.random.default_rng(1).integers(-8, 9, (4, 256)).astype(np.float64)
            assert not np.array_equal(x @ ap.T, x @ bad.T), (fmt, wrong)
        else:
            assert np.any(np.abs(bad - w) > ea), (fmt, wrong, name)
