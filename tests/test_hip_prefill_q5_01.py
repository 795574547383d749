"""The prompt pass of Q5_0 / Q5_1 models end to end.  From 32 rows a fast pass runs every layer matrix on the f16 matrix-core GEMM
(gemm_f16w.hip: WF_Q5_0 / WF_Q5_1, pinned by themselves in tests/test_hip_f16w_gemm_q5_01.py); a shorter pass keeps the row-by-row
GEMV.  Which kernel a matrix took is read from the plan words of a tapped pass (debug_prefill_tap: kernel_* = 1 the f16 GEMM, 3 the
GEMV).  A 40-token and a 23-token prompt on tiny-gqa and tiny-hd128: the logits of the last row and of one decoded step behind it
against the oracle's token loop inside the existing FAST_TOL row of the format; the strict device bit for bit at both lengths.

Not pinned here (stated, not hidden): the launches of such a pass row by row against float64, as tests/test_hip_prefill_launches.py
does for Q4_0 / Q8_0 / Q4_1."""
import numpy as np
import pytest

from crabml_amd import synth
from tests.helpers import FAST_TOL
from tests.test_hip_prefill import kv_equal, oracle_run

pytestmark = pytest.mark.gpu

TOKS = [1] + [int(t) for t in np.random.default_rng(5).integers(2, 1000, size=40)]
KERNELS = ("kernel_q", "kernel_k", "kernel_v", "kernel_wo", "kernel_gate", "kernel_up", "kernel_down")
_REF = {}


def reference(shape, fmt):
    """(model, the oracle's logits per position of TOKS, its runner), computed once per model and left unchanged"""
    if (shape, fmt) not in _REF:
        model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=91)
        ref, orr = oracle_run(model, True, TOKS)
        _REF[(shape, fmt)] = (model, ref, orr)
    return _REF[(shape, fmt)]


@pytest.mark.parametrize("n", [40, 23])
@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128"])
def test_fast_pass_takes_the_gemm_from_32_rows_and_stays_in_tolerance(ca, shape, fmt, n):
    model, ref, _ = reference(shape, fmt)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    plan = ca.HipLlamaRunner(conf, w, dev, 64, True).debug_prefill_tap(TOKS[:n], 1)["plan"]
    want = 1 if n >= 32 else 3
    assert plan["rows"] == n and plan["f16w"] == (1 if n >= 32 else 0) and plan["recomputed"] == 0, plan
    assert [plan[k] for k in KERNELS] == [want] * 7, plan
    r = ca.HipLlamaRunner(conf, w, dev, 64, True)
    lg = r.prefill(TOKS[:n])
    nxt = r.forward(TOKS[n], n)
    errs = [float(np.max(np.abs(got - exp)) / np.max(np.abs(exp))) for got, exp in ((lg, ref[n - 1]), (nxt, ref[n]))]
    print(f"{shape} {fmt} n={n}: last row {errs[0]:.3e}, decoded step {errs[1]:.3e} of FAST_TOL {FAST_TOL[fmt][1]}")
    assert max(errs) <= FAST_TOL[fmt][1], (shape, fmt, n, errs)


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128"])
def test_strict_pass_is_bit_identical_at_both_lengths(ca, shape, fmt):
    model, ref, orr = reference(shape, fmt)
    dev = ca.HipTensorDevice(0, False, 0, True)
    conf, w = synth.to_hip(model, dev)
    for n in (23, 40):
        r = ca.HipLlamaRunner(conf, w, dev, 64, True)
        lg = r.prefill(TOKS[:n])
        assert np.array_equal(lg.view(np.uint32), ref[n - 1].view(np.uint32)), (shape, fmt, n)
        assert np.array_equal(r.forward(TOKS[n], n).view(np.uint32), ref[n].view(np.uint32)), (shape, fmt, n)
    assert kv_equal(r, orr, model, 41, True)
