"""The prompt pass with everything it must not consume poisoned: the cache rows past the live positions, the decode step's data
scratch and the pass's own row buffers (HipLlamaRunner.debug_poison, what = 1 | 2 | 4).

Per case a runner first runs the whole scenario once, which allocates the row buffers (and the long-row score / probability
scratch, where the scenario gets there), then reset(), and runs it again with the fill in front of every call.  Runner A is filled
with a pattern, runner B with zeros, runner C is left alone: the pass's logits, the live cache rows, and the logits of four greedy
steps behind it must be equal bit for bit, A against B and C against B.

Which kernels a case runs is read from a tapped pass of a fourth runner (debug_prefill_tap's plan words) and held against the
case's name; the strict-order device has no tap and states its device only."""
import numpy as np
import pytest

from crabml_amd import synth
from tests.poison import (CACHE_TAIL, EXACT_ATTENTION, NO_TILE_ATTENTION, PASS_ROWS, PATTERNS, PREFILL_INT8_GEMM, STEP_SCRATCH, ZERO, cache_rows,
                          release_devices, same, same_cache, tokens_for)  # noqa: F401 (autouse fixture)

pytestmark = pytest.mark.gpu

WHAT = CACHE_TAIL | STEP_SCRATCH | PASS_ROWS
FLASH_ROWS, TILE, LONG_ROWS, HEAD_ROW = 1, 2, 3, 4  # CRABML_HIP_PFPLAN_ATTN_KERNEL
F16W, INT8, GEMV = 1, 2, 3                          # CRABML_HIP_PFPLAN_KERNEL_Q


class Case:
    def __init__(self, form, shape, fmt, rows, attn, gemm, seq=64, kv_f16=True, strict=False, flags=0, long_from=0, before=0, mix=False):
        self.form, self.shape, self.fmt, self.rows, self.attn, self.gemm, self.seq, self.kv_f16 = form, shape, fmt, rows, attn, gemm, seq, kv_f16
        self.strict, self.flags, self.long_from, self.before, self.mix = strict, flags, long_from, before, mix


CASES = [
    Case("k_attn_tile, int8 GEMM, 17 rows", "tiny-gqa", "Q4_0", 17, TILE, INT8),
    Case("k_attn_tile, f32 cache", "tiny-gqa", "Q8_0", 17, TILE, INT8, kv_f16=False),
    Case("k_attn_tile, f16 GEMM, 33 rows", "tiny-gqa", "Q4_0", 33, TILE, F16W),
    Case("k_attn per (head, row): NO_TILE_ATTENTION", "tiny-gqa", "Q4_0", 20, HEAD_ROW, INT8, flags=NO_TILE_ATTENTION),
    Case("k_attn per (head, row): group 7", "tiny-qwen2-g7", "Q4_0", 20, HEAD_ROW, INT8),
    Case("k_attn_flash_rows, 40 rows", "tiny-gqa", "Q4_0", 40, FLASH_ROWS, F16W, long_from=8),
    Case("f16 GEMM, 200 rows", "tiny-gqa", "Q4_0", 200, FLASH_ROWS, F16W, seq=256),
    Case("int8 GEMM at 40 rows (PREFILL_INT8_GEMM), Q4_1", "tiny-hd128", "Q4_1", 40, TILE, INT8, flags=PREFILL_INT8_GEMM),
    Case("a pass that starts inside the cache (pos0 = 5)", "tiny-gqa", "Q4_0", 33, TILE, F16W, before=5),
    Case("Q4_K_M body", "tiny-gqa", "Q4_K", 40, TILE, F16W, mix=True),
    Case("exact long-row kernels past 1024 positions", "tiny-gqa", "Q4_0", 40, LONG_ROWS, F16W, seq=1104, flags=EXACT_ATTENTION, before=1000),
    Case("strict device", "tiny-gqa", "Q4_0", 20, None, None, strict=True),
    Case("strict device, Q4_K body", "tiny-gqa", "Q4_K", 17, None, None, strict=True),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.form)
def test_poisoned_tail_scratch_and_row_buffers_change_no_pass(ca, case):
    model = synth.build_model(synth.SHAPES[case.shape], synth.TYPE_BY_NAME[case.fmt], seed=71, k_m_mix=case.mix)
    s = model.shape
    dev = ca.HipTensorDevice(0, False, 0, case.strict)
    conf, w = synth.to_hip(model, dev)
    mk = lambda: ca.HipLlamaRunner(conf, w, dev, case.seq, case.kv_f16, extra_flags=case.flags, attn_long_from=case.long_from)
    head, rows = tokens_for(s, case.before, salt=1), tokens_for(s, case.rows, salt=2)
    n = case.before + case.rows

    if not case.strict:  # the named kernels are what runs
        t = mk()
        if head:
            t.prefill(head)
        plan = t.debug_prefill_tap(rows, 0)["plan"]
        print(f"{case.form}: {case.shape} {case.fmt}{'_M' if case.mix else ''} rows {plan['rows']} at {plan['pos0']} -> attn_kernel {plan['attn_kernel']}, "
              f"f16w {plan['f16w']}, kernel_q {plan['kernel_q']}, recomputed {plan['recomputed']}")
        assert (plan["rows"], plan["pos0"]) == (case.rows, case.before), plan
        assert plan["attn_kernel"] == case.attn and plan["kernel_q"] == case.gemm and plan["f16w"] == (1 if case.gemm == F16W else 0), (case.form, plan)
        assert plan["recomputed"] == 0, plan

    def scenario(r, fill):
        def poison():
            if fill is not None:
                r.debug_poison(WHAT, *fill)
        out = []
        if head:
            poison()
            out.append(r.prefill(head).copy())
        poison()
        out.append(r.prefill(rows).copy())
        cache = cache_rows(r, s, case.kv_f16, n, case.seq)
        for step in range(4):
            tok = int(np.argmax(out[-1]))
            poison()
            out.append(r.forward(tok, n + step).copy())
        return out, cache + cache_rows(r, s, case.kv_f16, n + 4, case.seq)

    def run(fill):
        r = mk()
        scenario(r, None)  # allocates every buffer the scenario uses
        r.reset()
        return scenario(r, fill)

    base, base_cache = run(ZERO)
    assert all(np.all(np.isfinite(x)) for x in base), case.form
    plain, plain_cache = run(None)
    assert all(same(a, b) for a, b in zip(plain, base)) and same_cache(plain_cache, base_cache), f"{case.form}: the hook itself moved a result"
    for name, fill in PATTERNS.items():
        got, got_cache = run(fill)
        for i, (a, b) in enumerate(zip(got, base)):
            assert same(a, b), f"{case.form}: pattern {name} reached the logits of call {i} (passes first, then four greedy steps)"
        assert same_cache(got_cache, base_cache), f"{case.form}: pattern {name} reached the live cache rows"
