"""k_attn_flash_rows_split + k_attn_flash_rows_merge -- the split-KV form of the fast prompt pass's causal attention, what a short pass
deep in the cache runs (crabml_amd/csrc/fused_attention.hpp; chosen by flash_rows_slices, fused.hip) -- against float64 on the same f16
inputs, the decision, and a deep 32-row pass through a context.  Bound: FLASH_ROWS_REL = 1.5e-3 of max|out|, the one-launch form's.

Group 7 under the 64 KiB score row keeps its prompt pass on the per-(head, row) kernel (tests/test_hip_long_cache.py), so its context
here has a cache of 16384 positions, past that row; group 4 has 8192."""
import numpy as np
import pytest

from crabml_amd import synth
from tests import gqa_group_models as M
from tests import prefill_pass_ref as P
from tests.helpers import FAST_TOL
from tests.poison import release_devices, tokens_for  # noqa: F401 (autouse fixture)
from tests.test_hip_flash_attention import f64_causal_attention
from tests.test_hip_prefill_launches import run_case as prefill_case, tokens_of

pytestmark = pytest.mark.gpu

FLASH_ROWS_REL = 1.5e-3
NO_FLASH_ROWS_SPLIT = 1073741824
SHAPES = [(8, 2, 64), (8, 2, 128), (14, 2, 64), (8, 8, 128), (8, 1, 128)]  # groups 4, 4, 7 (two workgroups per kv head), 1, 8
# (pos0, rows, slices): one slice with a ragged second fragment; a single row; rows 0 .. 7 see nothing of the last slice (m = -inf);
# the diagonal starts on a slice boundary; more slices asked than tiles; full fragments over uneven slices; slices of one tile each
CASES = [(0, 17, 1), (130, 1, 3), (120, 40, 3), (128, 40, 3), (5, 16, 8), (200, 64, 4), (1000, 33, 16)]


def inputs(seed, n_heads, n_kv, hd, pos0, rows):
    rng = np.random.default_rng(seed)
    q = (rng.standard_normal(rows * n_heads * hd) / np.sqrt(hd)).astype(np.float32)
    k = rng.standard_normal((n_kv, pos0 + rows, hd)).astype(np.float16).view(np.uint16)
    v = rng.standard_normal((n_kv, pos0 + rows, hd)).astype(np.float16).view(np.uint16)
    return q, k, v


def rel_err(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("pos0,rows,slices", CASES)
@pytest.mark.parametrize("n_heads,n_kv,hd", SHAPES)
def test_split_kernel_equals_float64_arithmetic(ca, n_heads, n_kv, hd, pos0, rows, slices):
    dev = ca.HipTensorDevice(0)
    q, k, v = inputs(1000 * n_heads + 10 * n_kv + hd + pos0, n_heads, n_kv, hd, pos0, rows)
    got = dev.debug_flash_attention_rows_split(q, k.reshape(-1), v.reshape(-1), n_heads, n_kv, hd, pos0, rows, slices)
    assert np.all(np.isfinite(got))  # (the hook's partials start as NaN words: none unwritten was read)
    err = rel_err(got, f64_causal_attention(q, k, v, n_heads, n_kv, hd, pos0, rows))
    print(f"split rows vs float64, {n_heads}/{n_kv} x {hd}, pos0 {pos0}, {rows} rows, {slices} slices: {err:.2e} of max|out|")
    assert err <= FLASH_ROWS_REL, err
    for junk in (0xFFFF, 0x7C00):  # NaN / Inf behind the live cache reach no output
        kj = np.full((n_kv, pos0 + rows + 37, hd), junk, dtype=np.uint16)
        vj = kj.copy()
        kj[:, :pos0 + rows], vj[:, :pos0 + rows] = k, v
        gj = dev.debug_flash_attention_rows_split(q, kj.reshape(-1), vj.reshape(-1), n_heads, n_kv, hd, pos0, rows, slices)
        assert np.array_equal(gj.view(np.uint32), got.view(np.uint32)), hex(junk)


@pytest.mark.parametrize("n_heads,n_kv,hd", SHAPES)
def test_one_forced_slice_against_the_one_launch_kernel(ca, n_heads, n_kv, hd):
    """each form is within FLASH_ROWS_REL of float64, so they are within twice that of each other (no bit-equality: the one-launch form
    merges two waves' states per row)"""
    dev = ca.HipTensorDevice(0)
    q, k, v = inputs(77 + hd, n_heads, n_kv, hd, 100, 33)
    one = dev.debug_flash_attention_rows(q, k.reshape(-1), v.reshape(-1), n_heads, n_kv, hd, 100, 33)
    got = dev.debug_flash_attention_rows_split(q, k.reshape(-1), v.reshape(-1), n_heads, n_kv, hd, 100, 33, 1)
    assert np.all(np.isfinite(got)) and rel_err(got, one) <= 2 * FLASH_ROWS_REL


def test_the_decision(ca):
    dev = ca.HipTensorDevice(0)
    assert dev.debug_flash_rows_slices(8, 2, 32, 0) == 1        # ends under attn_long_from
    assert dev.debug_flash_rows_slices(32, 8, 512, 0) == 1      # a first pass of 512 rows
    assert dev.debug_flash_rows_slices(32, 8, 320, 30000) == 1  # 5 x 32 workgroups: past half of the 256 CUs already
    assert dev.debug_flash_rows_slices(8, 2, 32, 8128) > 1


@pytest.mark.parametrize("shape,seq", [("tiny-gqa", 8192), ("tiny-qwen2-g7", 16384)])
def test_a_deep_32_row_pass_through_a_context(ca, shape, seq):
    model = M.build(shape, "Q4_0", seed=92) if shape in M.SHAPES else synth.build_model(synth.SHAPES[shape], synth.Q4_0, seed=92)
    s = model.shape
    fill = tokens_for(s, 8128, salt=6)
    dev = ca.HipTensorDevice(0)
    assert dev.debug_flash_rows_slices(s.n_heads, s.n_kv_heads, 32, 8128) > 1
    plans = prefill_case(ca, f"split-pass/{shape}/Q4_0", model, seq, True, 32, [1], setup=lambda r: r.prefill(fill))
    assert plans[1]["pos0"] == 8128 and plans[1]["attn_kernel"] == P.ATTN_FLASH_ROWS, plans[1]
    conf, w = synth.to_hip(model, dev)
    lg = []
    for flags in (0, NO_FLASH_ROWS_SPLIT):
        r = ca.HipLlamaRunner(conf, w, dev, seq, True, extra_flags=flags)
        r.prefill(fill)
        lg.append(np.array(r.prefill(tokens_of(model, 32))))
    err = rel_err(lg[0], lg[1])
    print(f"{shape}: split vs one-launch logits of the pass, {err:.2e} of max|logit|")
    assert np.all(np.isfinite(lg[0])) and err <= FAST_TOL["Q4_0"][1], err
