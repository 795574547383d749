"""ffn_down of the fused step over rhs planes staged in LDS, its weights requested ahead (rows_partial_deep, gemv_core.hpp) against the
loop it replaces, BIT FOR BIT: where a step's activation unit comes from and when a row's weight loads are issued changes -- every
lane adds the same terms in the same ascending unit order.

  1. the fused step: ffn_down (k_gemv_res_nq with one row per wave) under the default flags against the same weights under
     CRABML_HIP_LLAMA_NQ_TWO_UNIT_ROUNDS (the A/B bit that keeps the two-unit loop over global memory), two runners in one process: the
     logits of four greedy tokens as uint32, then the KV-cache bytes.  Hidden sizes at the edges of the loop, counted in 64-unit steps
     (Q4_0 / Q4_1 have one unit per 32-element block, Q8_0 two): one full step, a ragged second, exactly seven (Q8_0: 14), a ragged
     eighth -- with two steps ahead: a lone last batch, a ragged one, odd and even step counts.  Below 8192 the split is forced both
     ways (one row per wave meets the new loop; two rows per wave keep the old one under either flag: the bit must change nothing
     there); from 8192 up the default rule gives two workgroups per chunk.
  2. the stand-alone GEMV across launch_wave_rows' rule: m = 4096 rows (one row per wave) against the same rows stacked twice
     (m = 8192: two rows per wave); m = 1 and 3 for the clamped row index.  Deep request rounds measured slower in these kernels
     (profiles/request_rounds.md) and did not ship: both sides run the one-step-per-round loop, and this pins the equality that any
     later change of the request order on one side of the rule has to keep.

The float64 pins of both (tests/test_hip_fused_launches.py::test_real_row_lengths, tests/test_hip_gemv.py) run the new default."""
import numpy as np
import pytest

from crabml_amd import synth

pytestmark = pytest.mark.gpu

NQ_TWO_UNIT_ROUNDS, SPLIT_ALWAYS, SPLIT_NEVER = 134217728, 16, 32
HT = {"Q4_0": "Q4_0", "Q8_0": "Q8_0", "Q4_1": "Q4_1"}


def shape(hidden):
    return synth.ModelShape("rounds", 512, hidden, 2, 8, 2, 1024, 64, 1e-5, None)


def flip_signs(model, seed=5):
    """block scales d of either sign on every Q4_0 / Q8_0 / Q4_1 tensor (as tests/test_hip_fused_launches.py has it)"""
    rng = np.random.default_rng(seed)
    for t in model.tensors.values():
        if t.typ in (synth.Q4_0, synth.Q8_0, synth.Q4_1):
            blk = t.data.reshape(-1, synth.BLOCK_BYTES[t.typ])
            blk[:, 1] ^= (rng.integers(0, 2, size=blk.shape[0], dtype=np.uint8) << 7)
    return model


def same_step(ca, model, flags, ctx, strict=False):
    """two runners on the same weights, `flags` and `flags | the A/B bit`: four greedy tokens from position 0"""
    dev = ca.HipTensorDevice(0, False, 0, strict)
    conf, w = synth.to_hip(model, dev)
    a = ca.HipLlamaRunner(conf, w, dev, 64, True, extra_flags=flags)
    b = ca.HipLlamaRunner(conf, w, dev, 64, True, extra_flags=flags | NQ_TWO_UNIT_ROUNDS)
    tok = 1
    for pos in range(4):
        la, lb = a.forward(tok, pos), b.forward(tok, pos)
        assert np.all(np.isfinite(la)), (ctx, pos)
        assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)), f"{ctx}: logits of token {pos} differ from the two-unit rounds'"
        tok = int(np.argmax(la))
    # the cache is [n_kv_heads][seq_len][head_dim] f16; rows past the four written positions are whatever the allocation held
    s = model.shape
    rows = lambda r, layer, v: r.debug_kv(layer, v, True).reshape(s.n_kv_heads, 64, s.head_dim * 2)[:, :4]
    for layer in range(s.n_layers):
        for v in (False, True):
            assert np.array_equal(rows(a, layer, v), rows(b, layer, v)), f"{ctx}: layer {layer} {'v' if v else 'k'} cache differs"


CASES = [(h, f) for h in (2048, 3072, 14336, 15360) for f in ("Q4_0", "Q8_0")] + [(3072, "Q4_1"), (15360, "Q4_1")]


@pytest.mark.parametrize("hidden,fmt", CASES)
def test_fused_step_equals_two_unit_rounds(ca, hidden, fmt):
    model = synth.build_model(shape(hidden), synth.TYPE_BY_NAME[fmt], seed=hidden // 64 + len(fmt))
    for flags in ((SPLIT_ALWAYS, SPLIT_NEVER) if hidden < 8192 else (0,)):
        same_step(ca, model, flags, f"{fmt} hidden {hidden} flags {flags}")


@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0"])
def test_fused_step_block_scales_of_either_sign(ca, fmt):
    model = flip_signs(synth.build_model(shape(15360), synth.TYPE_BY_NAME[fmt], seed=41))
    same_step(ca, model, 0, f"signs {fmt}")


def test_strict_order_device_ignores_the_bit(ca):
    """the strict-order step runs k_gemv_res_nq_ord: the bit changes nothing there"""
    model = synth.build_model(shape(14336), synth.Q4_0, seed=43)
    same_step(ca, model, 0, "strict Q4_0 hidden 14336", strict=True)


@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0", "Q4_1"])
@pytest.mark.parametrize("k", [32, 2048, 3072, 14336, 15360])
def test_gemv_across_the_decision_rule(ca, hdev, fmt, k):
    typ = synth.TYPE_BY_NAME[fmt]
    rng = np.random.default_rng(k + len(fmt))
    row_bytes = synth.BLOCK_BYTES[typ] * (k // 32)
    raw = synth.random_blocks(rng, 4096 * k, typ)
    assert raw.size == 4096 * row_bytes
    hx = ca.HipTensor.new(rng.standard_normal(k).astype(np.float32), [k], hdev)
    gt = getattr(ca.GGMLType, HT[fmt])

    def gemv(rows_raw, m):
        return ca.HipTensor.from_cpu(rows_raw, [m, k], gt, hdev).matmul_vec(hx).export().view(np.uint32)

    plain = gemv(np.concatenate([raw, raw]), 8192)  # two rows per wave
    assert np.array_equal(plain[:4096], plain[4096:])
    assert np.array_equal(gemv(raw, 4096), plain[:4096]), f"{fmt} 4096 x {k}"
    for m in (1, 3):  # the last wave's clamped row index
        assert np.array_equal(gemv(raw[:m * row_bytes].copy(), m), plain[:m]), f"{fmt} {m} x {k}"
