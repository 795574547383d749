"""GQA groups 3, 5, 6 and 7 (Llama-3.2-3B; Qwen2.5-14B / 32B; 1.5B; 7B / 0.5B) in the decode step's long-context attention: the
split-KV kernel k_attn_flash of the fast device from 96 cached positions, and the exact kernels (k_attn_scores / k_attn_softmax /
k_attn_pv) of the strict-order device and of CRABML_HIP_LLAMA_EXACT_ATTENTION from 224.

  1. k_attn_flash by itself against float64 on the same f16 inputs (FLASH_REL = 2e-5 of max|out|, the kernel's stated tolerance), its
     ticket form bit-equal to the two-launch form;
  2. the plan words of a context: the decode step takes the long-context kernels, the prompt pass's k_attn_flash_rows stays off;
  3. every launch of a tapped step at the hand-over (94 / 95 / 96 / 200) against float64 (tests/fused_step_ref.py), both bodies of
     the step -- the loop of tests/test_hip_fused_launches.py / test_hip_fused_k_launches.py, with this file's own expectation;
  4. the same past the ticket range (position 1030: k_attn_flash with the merge launch);
  5. graph, eager and Llama2Runner bit-equal over the switch, decode_greedy against a host arg-max loop;
  6. the exact kernels: strict-device logits bit-identical to the oracle through them and through the one-workgroup kernel, and a
     tapped EXACT_ATTENTION step either side of 224 whose attention equals the reference's bit for bit.

The models and seeds are those tests/test_gqa_groups_ref.py cleared on the oracle's own step (tests/gqa_group_models.py)."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests import gqa_group_models as M
from tests.helpers import to_oracle
from tests.qwen2_ref import OracleQwen2Runner, to_oracle_qwen2

pytestmark = pytest.mark.gpu

EXACT_ATTENTION, NO_LONG_ATTENTION, NO_K_NORM_IN = 4194304, 64, 16777216


# ---- 1. the kernel alone ----
def f64_attention(q, k, v, n_heads, n_kv, hd, seq):
    q16 = q.astype(np.float16).astype(np.float64).reshape(n_heads, hd)
    kf, vf = k.astype(np.float64), v.astype(np.float64)
    grp = n_heads // n_kv
    out = np.zeros((n_heads, hd))
    for h in range(n_heads):
        s = kf[h // grp] @ q16[h]
        p = np.exp(s - s.max())
        out[h] = (p / p.sum()) @ vf[h // grp]
    return out.reshape(-1)


def flash_case(dev, rng, n_heads, n_kv, hd, seq, slices, spread=1.0, kind="normal"):
    """-> the worst error of k_attn_flash + merge against float64, of max|out| (the inputs of tests/test_hip_flash_attention.py)"""
    q = (rng.standard_normal(n_heads * hd) * spread / np.sqrt(hd)).astype(np.float32)
    k = rng.standard_normal((n_kv, seq, hd)).astype(np.float16)
    v = rng.standard_normal((n_kv, seq, hd)).astype(np.float16)
    if kind == "spike":  # one position dominates, far from the slice that holds the running maximum first
        k[:, seq // 2] *= 6.0
    elif kind == "ties":  # every score equal: uniform probabilities over all slices
        k[:] = k[:, :1]
    elif kind == "dead":  # scores so low in all but the last slice that their weights underflow to 0 in the merge
        k[:, : seq - 1] = (-np.abs(k[:, : seq - 1].astype(np.float32)) * 3).astype(np.float16)
        q = np.abs(q) * 8
    got, ticket = dev.debug_flash_attention(q, k.view(np.uint16).reshape(-1), v.view(np.uint16).reshape(-1), n_heads, n_kv, hd, seq, slices)
    ctx = (n_heads, n_kv, hd, seq, slices, kind)
    assert np.array_equal(got.view(np.uint32), ticket.view(np.uint32)), f"{ctx}: the ticket form differs from the two-launch form"
    assert np.all(np.isfinite(got)), ctx
    ref = f64_attention(q, k, v, n_heads, n_kv, hd, seq)
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


GEOMETRIES = [(6, 2, 128), (3, 1, 64), (10, 2, 128), (5, 1, 64), (12, 2, 64), (6, 1, 128), (14, 2, 128), (28, 4, 128), (7, 1, 64)]


@pytest.mark.parametrize("n_heads,n_kv,hd", GEOMETRIES)
def test_flash_attention_of_the_new_groups_equals_float64_arithmetic(ca, n_heads, n_kv, hd):
    dev = ca.HipTensorDevice(0)
    rng = np.random.default_rng(1000 * n_heads + 10 * n_kv + hd)
    worst = 0.0
    for seq in (1, 3, 8, 31, 127, 128, 129, 257, 1000, 2049):
        for slices in (1, 7, 32):
            err = flash_case(dev, rng, n_heads, n_kv, hd, seq, slices)
            worst = max(worst, err)
            assert err <= R.FLASH_REL, (n_heads, n_kv, hd, seq, slices, err)
    print(f"flash vs float64, {n_heads} heads / {n_kv} kv x {hd}: worst {worst:.2e} of max|out|")


@pytest.mark.parametrize("kind", ["spike", "ties", "dead"])
def test_flash_attention_merge_edge_cases_group_7(ca, kind):
    dev = ca.HipTensorDevice(0)
    rng = np.random.default_rng(7)
    for seq in (130, 513):
        err = flash_case(dev, rng, 28, 4, 128, seq, 32, spread=4.0, kind=kind)
        print(f"group 7 {kind} seq {seq}: {err:.2e} of max|out|")
        assert err <= R.FLASH_REL, (kind, seq, err)


# ---- 2. the plan words ----
@pytest.mark.parametrize("shape", sorted(M.SHAPES))
def test_plan_words_of_the_new_groups(ca, shape):
    model = M.build(shape, "Q4_0")
    fdev, sdev = ca.HipTensorDevice(0), ca.HipTensorDevice(0, False, 0, True)
    conf, w = synth.to_hip(model, fdev)
    sconf, sw = synth.to_hip(model, sdev)
    p = ca.debug_step_plan(conf, w, fdev, 320, True)
    got = {k: p[k] for k in ("attn_flash", "attn_long_ok", "attn_long_from", "flash_ticket_until", "attn_s_rows", "attn_flash_rows")}
    # the decode step: k_attn_flash from 96 cached positions, its ticket form below 768; the prompt pass keeps its kernels (no
    # k_attn_flash_rows for a group outside 1 / 2 / 4 / 8)
    assert got == dict(attn_flash=1, attn_long_ok=1, attn_long_from=96, flash_ticket_until=768, attn_s_rows=96, attn_flash_rows=0), (shape, p)
    assert ca.debug_step_plan(conf, w, fdev, 320, False)["attn_long_ok"] == 0                               # f32 cache
    assert ca.debug_step_plan(conf, w, fdev, 320, True, extra_flags=NO_LONG_ATTENTION)["attn_long_ok"] == 0
    even = M.GROUP[shape] % 2 == 0  # k_attn_pv_split carries two heads per workgroup: an odd group keeps k_attn_pv
    for name, e in (("exact-attention", ca.debug_step_plan(conf, w, fdev, 320, True, extra_flags=EXACT_ATTENTION)),
                    ("strict", ca.debug_step_plan(sconf, sw, sdev, 320, True))):
        got = {k: e[k] for k in ("attn_flash", "exact_long_ok", "attn_long_ok", "attn_long_from", "pv_split", "attn_flash_rows")}
        assert got == dict(attn_flash=0, exact_long_ok=1, attn_long_ok=1, attn_long_from=224, pv_split=int(even), attn_flash_rows=0), (shape, name, e)


# ---- 3 / 4. every launch of a tapped step ----
def tapped_steps(ca, key, model, seq, positions, layers, flags=0):
    """-> {(layer, pos): the tapped step's plan words}.  A runner is teacher-forced greedily on its own tokens up to `pos` (from the
    graph) and takes one tapped step; the tapped logits equal a graph twin's bit for bit; every launch is held to float64 from the bytes
    it read, the attention in the form the plan words name (k_attn_flash: FLASH_REL; otherwise the reference's bits)."""
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    mk = lambda fl: ca.HipLlamaRunner(conf, w, dev, seq, True, True, True, extra_flags=fl)  # noqa: E731
    r, twin, planes_twin = mk(flags), mk(flags), None
    fails, plans = [], {}
    for pos in positions:
        twin.reset()
        tok = int(twin.decode_greedy(1, pos)[-1])
        want = twin.forward(tok, pos).copy()
        for layer in layers:
            ctx = f"{key} layer {layer} pos {pos}"
            r.reset()
            assert int(r.decode_greedy(1, pos)[-1]) == tok, ctx
            tap = r.debug_tap(tok, pos, layer)
            assert r.kv_cache_len() == pos + 1
            plan = plans[(layer, pos)] = tap["plan"]
            assert np.array_equal(tap["logits"].view(np.uint32), want.view(np.uint32)), f"{ctx}: the tapped (eager) step's logits differ from the graph's"
            flash = plan["attn_variant"] >= 16
            twin_tap = None
            if plan["path"] == 2 and plan["wo_x_only"]:  # the K body: gate | up's planes exist in LDS only -- the twin whose wo leaves them
                if planes_twin is None:
                    planes_twin = mk(flags | NO_K_NORM_IN)
                planes_twin.reset()
                assert int(planes_twin.decode_greedy(1, pos)[-1]) == tok, ctx
                twin_tap = planes_twin.debug_tap(tok, pos, layer)
                assert np.array_equal(twin_tap["logits"].view(np.uint32), want.view(np.uint32)), f"{ctx}: the NO_K_NORM_IN twin's logits differ"
            form = R.Form(defer=plan["defer_norm"] == 1, kv_f16=True, seq_cap=seq, flash_from=pos + 1 if flash else 0)
            kc, vc = r.debug_kv(layer, False, True), r.debug_kv(layer, True, True)
            res = R.check_layer(tap, kc, vc, model, layer, pos, form, ctx, twin=twin_tap, token=tok)
            for name, rr in res.items():
                print(f"{ctx} {name}: error / bound {rr.worst:.3f} excused {rr.excused}")
                fails += [f"{ctx} {name}: excused share {share:.3f} of {plane} above the cap" for plane, share in rr.excused.items()
                          if share > R.EXCUSED_CAP]
            fails += R.failures(res)
    assert not fails, "\n".join(fails)
    return plans


@pytest.mark.parametrize("shape,fmt", M.HANDOVER)
def test_every_launch_at_the_hand_over(ca, shape, fmt):
    """position 94 (95 cached: the staged one-workgroup kernel, the reference's bits), 95 and 96 (k_attn_flash, its ticket form: the
    merge inside the launch below 768 cached positions) and 200, layer 1; the Q4_K cases run the step's K-quant body"""
    plans = tapped_steps(ca, f"hand-over/{shape}/{fmt}", M.build(shape, fmt), 256, [94, 95, 96, 200], [1])
    assert [plans[(1, p)]["attn_variant"] for p in (94, 95, 96, 200)] == [0, 16 + 2, 16 + 2, 16 + 2]
    assert all((plan["path"] == 2) == (fmt == "Q4_K") for plan in plans.values())


def test_flash_attention_past_the_ticket_range(ca):
    plans = tapped_steps(ca, "past-1024/tiny-qwen2-g7/Q4_0", M.build("tiny-qwen2-g7", "Q4_0"), 1280, [1030], [0, 1])
    assert [plans[(layer, 1030)]["attn_variant"] for layer in (0, 1)] == [16 + 1, 16 + 1]  # k_attn_flash with the merge launch


# ---- 5. one step, three callers ----
def test_graph_eager_and_trait_runner_agree_over_the_switch(ca):
    model = M.build("tiny-qwen2-g7", "Q4_0")
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    graph, eager = ca.HipLlamaRunner(conf, w, dev, 128, True), ca.HipLlamaRunner(conf, w, dev, 128, True, False)
    tdev = ca.HipTensorDevice(0)
    tconf, tw = synth.to_hip(model, tdev)
    trait = ca.Llama2Runner(tconf, tw, tdev, 128, True)
    toks = [int(t) for t in np.random.default_rng(9).integers(0, 1024, size=101)]
    for i, t in enumerate(toks):
        a, b, c = graph.forward(t, i).copy(), eager.forward(t, i).copy(), np.asarray(trait.forward([t], i)).copy()
        if i >= 90:
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"graph vs eager, position {i}"
            assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), f"graph vs Llama2Runner, position {i}"
    st = tdev.lazy_stats()
    assert st["fused_tokens"] == len(toks) and st["replayed"] == 0, st  # (the runner's calls were served by the fused step)
    # decode_greedy over positions 90 .. 100 = a host arg-max loop over the eager runner's logits
    graph.reset()
    eager.reset()
    for i, t in enumerate(toks[:90]):
        graph.forward_async(t, i)
        eager.forward_async(t, i)
    ids, tok = [], toks[90]
    for i in range(90, 101):
        tok = int(ca.sample_argmax(np.asarray(eager.forward(tok, i))))
        ids.append(tok)
    assert [int(t) for t in graph.decode_greedy(toks[90], 11)] == ids


# ---- 6. the exact kernels ----
CHECK = (223, 224, 225, 300, 1023, 1024, 1025)


@pytest.mark.parametrize("shape", ["tiny-g3", "tiny-qwen2-g7"])
def test_strict_decode_equals_the_oracle_through_the_exact_long_context_kernels(ca, shape):
    model = M.build(shape, "Q4_0", n_layers=1)
    seq, n = 1040, CHECK[-1] + 1
    toks = [int(t) for t in np.random.default_rng(5).integers(0, 1024, size=n)]
    odev = o.OracleDevice(thread_num=8)
    if model.shape.arch == "qwen2":
        orr = OracleQwen2Runner(*to_oracle_qwen2(model, odev), odev, seq, True)
    else:
        orr = o.OracleLlamaRunner(*to_oracle(model, odev), odev, seq, True)
    sdev = ca.HipTensorDevice(0, False, 0, True)
    sconf, sw = synth.to_hip(model, sdev)
    plan = ca.debug_step_plan(sconf, sw, sdev, seq, True)
    assert (plan["exact_long_ok"], plan["attn_long_ok"], plan["attn_flash"], plan["attn_long_from"]) == (1, 1, 0, 224), plan
    strict_long = ca.HipLlamaRunner(sconf, sw, sdev, seq, True)                                  # the exact kernels from 224 positions
    strict_one = ca.HipLlamaRunner(sconf, sw, sdev, seq, True, extra_flags=NO_LONG_ATTENTION)    # one workgroup per head throughout
    for i, t in enumerate(toks):
        ref = orr.forward([t], i)
        if i in CHECK:
            for name, r in (("long", strict_long), ("one-wg", strict_one)):
                got = r.forward(t, i)
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"strict {name} position {i}"
        else:
            strict_long.forward_async(t, i)
            strict_one.forward_async(t, i)


@pytest.mark.parametrize("shape,fmt", [("tiny-g3", "Q4_0"), ("tiny-g5", "Q4_1"), ("tiny-qwen2-g6", "Q4_0"), ("tiny-qwen2-g7", "Q4_0")])
def test_exact_attention_switches_kernels_at_224_and_keeps_the_reference_bits(ca, shape, fmt):
    """CRABML_HIP_LLAMA_EXACT_ATTENTION on the fast device (the strict device's step is not tapped): 223 cached positions on the
    one-workgroup kernel, 224 and 300 on k_attn_scores / k_attn_softmax / k_attn_pv (group 6: k_attn_pv_split) -- the attention of
    every tapped step equals the reference's bit for bit (Form.flash_from = 0)"""
    plans = tapped_steps(ca, f"exact/{shape}/{fmt}", M.build(shape, fmt), 320, [222, 223, 300], [1], flags=EXACT_ATTENTION)
    assert [plans[(1, p)]["attn_variant"] for p in (222, 223, 300)] == [0, 1, 1]
