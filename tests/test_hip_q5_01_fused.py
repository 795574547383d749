"""Every launch of the fast fused decode step over Q5_0 / Q5_1 layers (enqueue_segment_t<Q5_0 / Q5_1>: k_qkv, attention, k_gemv_res_nq
for wo, k_gateup_q, k_gemv_res_nq for ffn_down, the classifier; a Q5_1 body in front of a Q6_K classifier: enqueue_segment_k<Q5_1>)
pinned against float64, launch by launch, as tests/test_hip_fused_launches.py pins Q4_0 / Q8_0 / Q4_1.  The checker is
tests/q5_01_step_ref.py (its derivation: that module's docstring; its own tests, and the excused shares of the interval checks for
the models below from the reference alone: tests/test_q5_01_step_ref.py, whose CASES list this file runs).

A runner is teacher-forced greedily on its own tokens up to `pos` (from the graph), then takes ONE tapped step; the tapped (eager)
step's logits equal a graph twin's bit for bit.  Every case asserts the plan's path: a Q5_0 / Q5_1 context on the per-op segments
fails here.  Why each shape is here:
  tiny-gqa     wk / wv hold a quarter of wq's blocks: Q5_0's third plane is addressed from each matrix's own two pointers; GQA group 4
  tiny-hd128   head_dim 128
  15m          dim 288: 9 blocks per row, a ragged single 64-unit step; head_dim 48, so attention's stand-alone quantizer runs
  tiny-qwen2   biases, NEOX rope
  ffn130       hidden 4160: ffn_down rows of 130 blocks -- three 64-unit steps, two live lanes in the last; with two workgroups per
               chunk (SPLIT_CHUNKS_ALWAYS) the launch is rows_partial_deep's pipelined loop and its clamped tail
Positions 0, 7 and 100 of a 128-position cache: from 96 cached positions the long-context attention (k_attn_flash where the geometry
has it) writes wo's rhs.

Not pinned here (stated, not hidden): the strict-order device (its ordered launches are bit-exact to the oracle:
tests/test_hip_fused.py), tensor-parallel ranks and mixed bodies (per-op segments), and the prompt pass."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests import q5_01_step_ref as Q
from tests.helpers import EXACT_NORM, FAST_TOL, record_observed, to_oracle
from tests.test_q5_01_step_ref import CASES, FMT, SPLIT_ALWAYS, build

pytestmark = pytest.mark.gpu

_OBSERVED = {}
BY_KEY = {c[0]: c for c in CASES}


def record(key, results):
    _OBSERVED[key] = {"error_over_bound": {k: round(r.worst, 4) for k, r in results.items()},
                      "excused_share": {k: {n: round(v, 4) for n, v in r.excused.items()} for k, r in results.items() if r.excused}}
    record_observed(_OBSERVED, "fused_q5_01_launch_pins.json")


def expect_flash(model, pos):
    s = model.shape
    return s.head_dim in (64, 128) and s.n_heads // s.n_kv_heads in (1, 2, 4, 8) and pos + 1 >= 96


def run_case(ca, key):
    """-> {(layer, pos): the tapped step's launch plan}"""
    _, _, fmt, _, _, flags, seq, positions, layers, want_path = BY_KEY[key]
    model = build(BY_KEY[key])
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    assert ca.debug_step_plan(conf, w, dev, seq, True, extra_flags=flags)["path"] == want_path
    mk = lambda: ca.HipLlamaRunner(conf, w, dev, seq, True, True, True, extra_flags=flags)  # noqa: E731
    r, twin = mk(), mk()
    fails, plans = [], {}
    for pos in positions:
        twin.reset()
        tok = int(twin.decode_greedy(1, pos)[-1]) if pos else 1
        want = twin.forward(tok, pos).copy()
        for layer in layers:
            ctx = f"{key} layer {layer} pos {pos}"
            r.reset()
            if pos:
                assert int(r.decode_greedy(1, pos)[-1]) == tok, ctx
            tap = r.debug_tap(tok, pos, layer)
            assert r.kv_cache_len() == pos + 1
            plan = plans[(layer, pos)] = tap["plan"]
            assert plan["path"] == want_path, (ctx, plan)
            defer, flash = plan["defer_norm"] == 1, plan["attn_variant"] >= 16
            # the hop-free norm is Q5_0's default (as Q4_0's) and never Q5_1's (as Q4_1's); every chunk's workgroup is resident here
            assert defer == (fmt == "Q5_0" and not (flags & EXACT_NORM) and want_path == 1), (ctx, plan)
            if want_path == 1:
                assert plan["norm_epilogue"] == 1 and ("wo.rsums" in tap) == defer, (ctx, plan)
            assert flash == expect_flash(model, pos), (ctx, plan)
            assert np.array_equal(tap["logits"].view(np.uint32), want.view(np.uint32)), f"{ctx}: the tapped (eager) step's logits differ from the graph's"
            form = R.Form(defer=defer, kv_f16=True, seq_cap=seq, flash_from=pos + 1 if flash else 0)
            kc, vc = r.debug_kv(layer, False, True), r.debug_kv(layer, True, True)
            res = Q.check_layer(tap, kc, vc, model, layer, pos, form, ctx, token=tok)
            for name, rr in res.items():
                print(f"{ctx} {name}: error / bound {rr.worst:.3f} excused {rr.excused}")
            record(f"{key}/L{layer}/p{pos}", res)
            fails += Q.failures(res)
    assert not fails, "\n".join(fails)
    return plans


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128", "15m", "tiny-qwen2"])
def test_default_step_every_launch(ca, shape, fmt):
    """the default step: hop-free for Q5_0, exact-norm launches with Q8_1 planes for Q5_1; layers 0 and 1, positions 0, 7 and 100"""
    plans = run_case(ca, f"default/{shape}/{fmt}")
    for (layer, pos), plan in plans.items():
        assert (plan["split_wo"], plan["split_down"]) == (1, 1), plan
        # layer 0 reads its own norm launch's planes through the plain loaders; layer 1 of a hop-free context the deferred one
        assert plan["qkv_loader"] in ((3,) if fmt == "Q5_0" and layer == 1 else (1, 2)), plan


@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128", "15m", "tiny-qwen2"])
def test_q5_0_exact_norm_twin(ca, shape):
    """CRABML_HIP_LLAMA_EXACT_NORM switches Q5_0 back to the exact norm in the epilogue"""
    plans = run_case(ca, f"exact-norm/{shape}/Q5_0")
    assert all(p["defer_norm"] == 0 and p["qkv_loader"] in (1, 2) for p in plans.values()), plans


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
def test_ffn_down_rows_of_130_blocks(ca, fmt):
    """two workgroups per chunk (split 2: one row per wave, 16 waves per CU), which is what nq_request_depth answers NQ_DEEP for: the
    plan has no word for the depth itself, split_down == 2 on a device of at least 32 CUs is its precondition"""
    plans = run_case(ca, f"ffn130/{fmt}")
    for plan in plans.values():
        assert (plan["split_wo"], plan["split_down"]) == (2, 2) and plan["n_cu"] >= 32, plan


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
def test_block_scales_of_either_sign(ca, fmt):
    run_case(ca, f"signs/tiny-gqa/{fmt}")


def test_shrunk_residual_stream(ca):
    """a residual stream small enough for RMSNorm's eps to matter in every launch"""
    run_case(ca, "shrunk/tiny-gqa/Q5_0")


def test_q6_k_classifier(ca):
    """llama.cpp's Q5_0 / Q5_1 files: a Q5_0 body stays on the five launches (path 1, the classifier's Q8_K planes from its own norm
    and quantizer launches), a Q5_1 body takes enqueue_segment_k<Q5_1> (path 2)"""
    run_case(ca, "q6k-classifier/tiny-gqa/Q5_0")
    plans = run_case(ca, "q6k-classifier/tiny-gqa/Q5_1")
    assert all(p["norm_epi_k"] == 0 and p["qin"] == 0 for p in plans.values()), plans


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
def test_lazy_queue_runs_the_fused_step(ca, fmt):
    """Llama2Runner::forward on a fast device: the recorded calls reach the same step -- the bits of crabml_hip_llama_forward, four
    tokens, every one of them fused -- and stay inside the format's row of FAST_TOL against the oracle"""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], FMT[fmt], seed=87)
    toks = [1, 365, 400, 282]
    odev = o.OracleDevice(thread_num=4, use_avx2=False)
    oconf, ow = to_oracle(model, odev)
    orr = o.OracleLlamaRunner(oconf, ow, odev, 32, True)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    r = ca.Llama2Runner(conf, w, dev, 32, True)
    f = ca.HipLlamaRunner(conf, w, dev, 32, True, False)
    errs = []
    for i, t in enumerate(toks):
        ref = orr.forward([t], i)
        a = r.forward([t], i).copy()
        c = f.forward(t, i)
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), f"queue vs fused entry point, step {i}"
        errs.append(float(np.max(np.abs(a - ref)) / np.max(np.abs(ref))))
    print(f"{fmt}: queue vs oracle {errs}")
    assert max(errs) <= FAST_TOL[fmt][1], errs
    assert dev.lazy_stats()["fused_tokens"] == 4, dev.lazy_stats()


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
def test_a_long_context_is_created(ca, fmt):
    """20000 positions on tiny-hd128: a plan with the long-context attention behind it, and a context that runs a step"""
    model = synth.build_model(synth.SHAPES["tiny-hd128"], FMT[fmt], seed=88)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    plan = ca.debug_step_plan(conf, w, dev, 20000, True)
    assert plan["path"] == 1 and plan["attn_long_ok"] == 1 and plan["attn_long_from"] < 20000, plan
    r = ca.HipLlamaRunner(conf, w, dev, 20000, True)
    assert np.all(np.isfinite(r.forward(1, 0)))
