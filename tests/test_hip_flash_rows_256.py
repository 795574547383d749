"""The flash-rows family at head_dim 256 (k_attn_flash_rows_w, k_attn_flash_rows_split_w + k_attn_flash_rows_merge<256>: fills of 32
positions, workgroups of at most 4 row waves; crabml_amd/csrc/fused_attention.hpp) against float64 on the same f16 inputs, at the
family's stated bound of 1.5e-3 of max|out|, and through a Gemma context created with CRABML_HIP_LLAMA_PREFILL_FLASH_ROWS_HD256."""
import numpy as np
import pytest

from crabml_amd import synth
from tests.helpers import FAST_TOL
from tests.test_hip_flash_attention import f64_causal_attention
from tests.test_hip_gemma import rel_errs, restated

pytestmark = pytest.mark.gpu
HD = 256
BOUND = 1.5e-3  # the family's: probabilities enter the second product as f16
FLASH_ROWS_HD256 = -2147483648  # CRABML_HIP_LLAMA_PREFILL_FLASH_ROWS_HD256 (include/crabml_hip_debug.h): bit 31


def inputs(rng, n_heads, n_kv, pos0, rows):
    q = (rng.standard_normal(rows * n_heads * HD) / np.sqrt(HD)).astype(np.float32)
    k = rng.standard_normal((n_kv, pos0 + rows, HD)).astype(np.float16).view(np.uint16)
    v = rng.standard_normal((n_kv, pos0 + rows, HD)).astype(np.float16).view(np.uint16)
    return q, k, v


def rel(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("n_heads,n_kv", [(8, 1), (2, 1), (4, 4), (8, 2)])
def test_one_launch_kernel_equals_float64_arithmetic(ca, n_heads, n_kv):
    """a 16-row wave, a 64-row workgroup and a 32-position fill each crossed with and without a tail, passes that start mid-cache;
    junk behind the live positions (capacity = live + 37) changes no bit"""
    dev = ca.HipTensorDevice(0)
    rng = np.random.default_rng(31 * n_kv + n_heads)
    worst = 0.0
    for pos0, rows in ((0, 1), (0, 17), (0, 64), (0, 65), (5, 33), (64, 64), (100, 129), (777, 150)):
        q, k, v = inputs(rng, n_heads, n_kv, pos0, rows)
        got = dev.debug_flash_attention_rows(q, k.reshape(-1), v.reshape(-1), n_heads, n_kv, HD, pos0, rows)
        for junk in (0xFFFF, 0x7C00, 0x7BFF):
            kj = np.full((n_kv, pos0 + rows + 37, HD), junk, dtype=np.uint16)
            vj = np.full((n_kv, pos0 + rows + 37, HD), junk, dtype=np.uint16)
            kj[:, :pos0 + rows], vj[:, :pos0 + rows] = k, v
            gj = dev.debug_flash_attention_rows(q, kj.reshape(-1), vj.reshape(-1), n_heads, n_kv, HD, pos0, rows)
            assert np.array_equal(gj.view(np.uint32), got.view(np.uint32)), (pos0, rows, hex(junk))
        assert np.all(np.isfinite(got)), (pos0, rows)
        err = rel(got, f64_causal_attention(q, k, v, n_heads, n_kv, HD, pos0, rows))
        worst = max(worst, err)
        assert err <= BOUND, (pos0, rows, err)
    print(f"flash rows 256 vs float64, {n_heads} heads / {n_kv} kv: worst {worst:.2e} of max|out|")


@pytest.mark.parametrize("n_heads,n_kv", [(8, 1), (8, 2)])
def test_split_form_and_merge_equal_float64_arithmetic(ca, n_heads, n_kv):
    """1, 3 and 32 slices (clamped to the pass's tiles); the hook's partials start as NaN words, so an unwritten one shows in out"""
    dev = ca.HipTensorDevice(0)
    rng = np.random.default_rng(17 * n_kv + n_heads)
    worst = 0.0
    for pos0, rows in ((130, 8), (1000, 32), (2049, 15)):
        q, k, v = inputs(rng, n_heads, n_kv, pos0, rows)
        ref = f64_causal_attention(q, k, v, n_heads, n_kv, HD, pos0, rows)
        one = dev.debug_flash_attention_rows(q, k.reshape(-1), v.reshape(-1), n_heads, n_kv, HD, pos0, rows)
        for slices in (1, 3, 32):
            got = dev.debug_flash_attention_rows_split(q, k.reshape(-1), v.reshape(-1), n_heads, n_kv, HD, pos0, rows, slices)
            assert not np.isnan(got).any(), (pos0, rows, slices)
            err = rel(got, ref)
            worst = max(worst, err)
            assert err <= BOUND, (pos0, rows, slices, err)
            if slices == 1:
                assert rel(got, one) <= BOUND, (pos0, rows)
    print(f"flash rows 256 split vs float64, {n_heads} heads / {n_kv} kv: worst {worst:.2e} of max|out|")


def test_one_forced_slice_equals_the_one_launch_kernel_bit_for_bit(ca):
    """both forms run flash_rows_walk, every wave owning its 16 rows from the first tile to the last: 33 rows (a ragged third
    fragment) at position 100, the split hook with one slice against the one-launch hook, compared as words.  Both normalise by
    the quotient O / l (k_attn_flash_rows_merge<256>: fma(O, e^0, 0) / fma(l, e^0, 0)); with O * (1 / l) in the one-launch kernel
    16890 of the 67584 words differed by one unit in the last place."""
    dev = ca.HipTensorDevice(0)
    q, k, v = inputs(np.random.default_rng(256), 8, 2, 100, 33)
    one = dev.debug_flash_attention_rows(q, k.reshape(-1), v.reshape(-1), 8, 2, HD, 100, 33)
    got = dev.debug_flash_attention_rows_split(q, k.reshape(-1), v.reshape(-1), 8, 2, HD, 100, 33, 1)
    a, b = one.view(np.uint32).astype(np.int64), got.view(np.uint32).astype(np.int64)
    print(f"flash rows 256, one slice vs one launch: {int(np.count_nonzero(a != b))} of {a.size} words differ, by at most {int(np.max(np.abs(a - b)))}")
    assert np.array_equal(one.view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("shape", ["tiny-gemma", "tiny-gemma-g8"])
def test_flagged_gemma_context_runs_the_family(ca, shape):
    """prefill in passes at pos0 = 0, 72, 144 (the last one short), then 4 decode steps on the cache the passes wrote, against the
    restatement and against a flagged context that ran the token loop; the plan says the family only with the flag"""
    model = synth.build_model(synth.SHAPES[shape], synth.Q4_0, seed=29)
    toks = [(7 * i + 3) % 1000 for i in range(204)]
    ref, _ = restated(model, True, toks, seq_len=320)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    assert ca.debug_step_plan(conf, w, dev, 320, 1, extra_flags=FLASH_ROWS_HD256)["attn_flash_rows"] == 1
    assert ca.debug_step_plan(conf, w, dev, 320, 1)["attn_flash_rows"] == 0
    tol = FAST_TOL["FLASH:Q4_0"][1]
    r = ca.HipLlamaRunner(conf, w, dev, 320, True, extra_flags=FLASH_ROWS_HD256, prefill_chunk=72)
    got = [np.array(r.prefill(toks[:200]))] + [r.forward(t, 200 + i).copy() for i, t in enumerate(toks[200:])]
    errs = rel_errs(got, ref[199:])
    print(f"{shape}: prefill + 4 steps vs the restatement {errs}")
    assert errs.max() <= tol, errs
    loop = ca.HipLlamaRunner(conf, w, dev, 320, True, extra_flags=FLASH_ROWS_HD256)
    ll = [loop.forward(t, i).copy() for i, t in enumerate(toks)]
    assert rel_errs(got, ll[199:]).max() <= tol
