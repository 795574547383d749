"""The prompt pass of Q5_0 / Q5_1 models end to end.  From 32 rows a fast pass runs every layer matrix on the f16 matrix-core GEMM
(gemm_f16w.hip: WF_Q5_0 / WF_Q5_1, pinned by themselves in tests/test_hip_f16w_gemm_q5_01.py); a shorter pass keeps the row-by-row
GEMV.  Which kernel a matrix took is read from the plan words of a tapped pass (debug_prefill_tap: kernel_* = 1 the f16 GEMM, 3 the
GEMV).  A 40-token and a 23-token prompt on tiny-gqa and tiny-hd128: the logits of the last row and of one decoded step behind it
against the oracle's token loop inside the existing FAST_TOL row of the format; the strict device bit for bit at both lengths.

Against the oracle's token loop at 200 rows, and on the tiny-wide shape (ffn_down's k pieces) at 40 and 200, the f16 pass and the
PREFILL_INT8_GEMM pass (the GEMV row by row) in the form of tests/test_hip_prefill_q23k_launches.test_fast_prompt_pass_f16_weight_gemm.

The launches of such a pass row by row against float64: tests/test_hip_prefill_q5_01_launches.py."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests.helpers import FAST_TOL, record_observed, to_oracle
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


PREFILL_INT8_GEMM = 524288  # CRABML_HIP_LLAMA_PREFILL_INT8_GEMM
WIDE = synth.ModelShape("tiny-wide", 512, 4096, 1, 4, 2, 512, 256, 1e-5, None)


@pytest.mark.parametrize("shape,n", [("tiny-gqa", 200), ("tiny-wide", 40), ("tiny-wide", 200)])
@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
def test_fast_prompt_pass_f16_weight_gemm(ca, fmt, shape, n):
    """Against the oracle's token loop the f16 pass sits inside the format's fast tolerance (FAST_TOL[fmt][1]), as the flagged pass
    (the GEMV row by row) does; the two agree inside it and are NOT equal (the flag must change the arithmetic); the greedy continuation
    starts with the same token; the pass is bit-identical run to run (tiny-wide: ffn_down's k pieces are added in a fixed order)."""
    model = synth.build_model(WIDE if shape == "tiny-wide" else synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=91 if shape != "tiny-wide" else 17)
    prompt = [(11 * i + 5) % model.shape.vocab for i in range(n)]
    odev = o.OracleDevice(thread_num=8, use_avx2=False)
    oconf, ow = to_oracle(model, odev)
    orr = o.OracleLlamaRunner(oconf, ow, odev, n + 16, True)
    ref = None
    for i, t in enumerate(prompt):
        ref = orr.forward([t], i)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    a = ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=512)
    b = ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=512, extra_flags=PREFILL_INT8_GEMM)
    la, lb = np.array(a.prefill(prompt)), np.array(b.prefill(prompt))
    la2 = np.array(ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=512).prefill(prompt))
    scale = float(np.max(np.abs(ref)))
    ea, eb, eab = (float(np.max(np.abs(x - y))) / scale for x, y in ((la, ref), (lb, ref), (la, lb)))
    tol = FAST_TOL[fmt][1]
    print(f"{shape}/{fmt}/{n}: f16 vs oracle {ea:.3g}, flagged vs oracle {eb:.3g}, f16 vs flagged {eab:.3g}, bound {tol:.3g}")
    record_observed({f"end-to-end/{shape}/{fmt}/{n}": {"f16_vs_oracle": ea, "flagged_vs_oracle": eb, "f16_vs_flagged": eab, "bound": tol}},
                    "prefill_q5_01_launch_pins.json")
    assert eb <= tol, ("flagged pass vs oracle", eb)
    assert ea <= max(tol, 1.25 * eb), ("f16 pass vs oracle", ea)
    assert eab <= tol, ("f16 pass vs flagged pass", eab)
    assert not np.array_equal(la, lb)  # (equal logits would mean the matrices never left the GEMV)
    assert np.array_equal(la.view(np.uint32), la2.view(np.uint32))
    nxt = int(np.argmax(ref))
    assert list(a.decode_greedy(nxt, 4))[0] == list(b.decode_greedy(nxt, 4))[0]
    assert a.kv_cache_len() == b.kv_cache_len() == n + 4
