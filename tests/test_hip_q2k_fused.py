"""Every launch of the fast K-quant decode step over a Q2_K BODY (enqueue_segment_k<Q2_K>: k_qkv<Q2_K> with its V hand-over, attention,
k_gemv_res_nq<F, SPLIT, QIN> for wo with F the tensor's own format, k_gateup_k_lds<QOUT, false, NORMIN, Q2_K>, k_gemv_res_nq for
ffn_down, the classifier) pinned against float64, launch by launch, as tests/test_hip_q3k_fused.py and tests/test_hip_q6k_fused.py
pin their bodies: the checker is tests/q2k_step_ref.py (its derivation: that module's docstring; its own tests, and the excused
shares of the Q8_K interval check for the models below, from the reference alone: tests/test_q2k_step_ref.py, whose CASES list this
file runs).

A runner is teacher-forced greedily on its own tokens up to `pos` (from the graph), then takes ONE tapped step; the tapped (eager)
step's logits equal a graph twin's bit for bit; where gate | up normalizes and quantizes wo's row in LDS (k_norm_in, the default) a
NO_K_NORM_IN twin leaves the planes.  Every case asserts plan["path"] == 2: a Q2_K context on the per-op segments fails here.

Not pinned here (stated, not hidden): the strict-order device and tensor-parallel ranks (per-op segments, bit-exact to the oracle:
tests/test_hip_fused.py), and the Q2_K prompt pass (unchanged: tests/test_hip_prefill.py)."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import q2k_step_ref as Q
from tests import test_hip_q6k_fused as H6
from tests.helpers import check_fast, record_observed, to_oracle
from tests.test_hip_q3k_fused import FLAG_CASES, SPLIT_ALWAYS, SPLIT_NEVER
from tests.test_q2k_step_ref import CASES, build

pytestmark = pytest.mark.gpu

_OBSERVED = {}
BY_KEY = {c[0]: c for c in CASES}
Q2K, Q3K, Q4K = synth.Q2_K, synth.Q3_K, synth.Q4_K


def record(key, results):
    _OBSERVED[key] = {"error_over_bound": {k: round(r.worst, 4) for k, r in results.items()},
                      "excused_share": {k: {n: round(v, 6) for n, v in r.excused.items()} for k, r in results.items() if r.excused}}
    record_observed(_OBSERVED, "fused_q2k_launch_pins.json")


def expect_flash(model, pos):
    """k_attn_flash from 96 cached positions on, for every GQA group up to 8 (decide_attention, fused.hip).  The Q6_K file's own
    predicate names groups 1, 2, 4 and 8 only -- it never ran another group that far --, and this file runs group 7 at position 100."""
    s = model.shape
    return s.head_dim in (64, 128, 256) and 1 <= s.n_heads // s.n_kv_heads <= 8 and pos + 1 >= 96


def run_case(ca, key, model, seq, positions, layers, **kw):
    """tests/test_hip_q6k_fused.run_case (one tapped step per (layer, position), its graph and NO_K_NORM_IN twins, every launch through
    the checker, plan["path"] == 2) with this file's checker and record -> {(layer, pos): the tapped step's launch plan}"""
    saved = H6.Q, H6.record, H6.expect_flash
    H6.Q, H6.record, H6.expect_flash = Q, record, expect_flash
    try:
        return H6.run_case(ca, key, model, seq, positions, layers, **kw)
    finally:
        H6.Q, H6.record, H6.expect_flash = saved


def run_listed(ca, key, **kw):
    _, _, _, _, seq, positions, layers = BY_KEY[key]
    return run_case(ca, key, build(BY_KEY[key]), seq, positions, layers, **kw)


def layer_types(model, n_layers):
    return [tuple(model.tensors[f"blk.{l}.{n}.weight"].typ for n in ("attn_v", "attn_output", "ffn_down")) for l in range(n_layers)]


@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128", "tiny-qwen2-g7", "tiny-gemma"])
def test_default_fast_step_every_launch(ca, shape):
    """Q2_K body and classifier (tiny-hd128: a Q4_K classifier; Gemma: its tied, scaled Q2_K embedding): dim 512 (2 super-blocks per row
    = 8 pieces, most lanes dead; hidden 1024: 4), dim 1792 (7 super-blocks = 28 pieces, the partial lane round; Qwen2's biases and NEOX
    pairs), head_dim 64 / 128 / 256, Gemma's GELU; position 0 (the staged attention, wo quantizes its rhs) and 100 (k_attn_flash)"""
    plans = run_listed(ca, f"default/{shape}")
    assert {pos for _, pos in plans} == {0, 100}
    for (layer, pos), plan in plans.items():
        assert plan["path"] == 2, plan
        assert (plan["norm_epi_k"], plan["q8k_producers"], plan["k_norm_in"], plan["wo_x_only"], plan["qin"]) == (1, 1, 1, 1, 1), plan
        assert (plan["qmode_down"], plan["split_wo"]) == (2, 2), plan
        if pos == 0:
            assert plan["attn_variant"] == 0 and plan["qmode_wo"] == 1, (layer, plan)
        elif shape == "tiny-gqa":
            assert plan["attn_variant"] == 16 + 2, (layer, plan)  # k_attn_flash, GQA group 4 (as tests/test_hip_q3k_fused.py reads it)


@pytest.mark.parametrize("name", ["8b-rows", "dim8192"])
def test_real_row_lengths(ca, name):
    """dim 4096 (16 super-blocks: exactly one lane round of quads, the prologue's second round requests nothing) / hidden 14336
    (ffn_down rows of 56 super-blocks: 224 pieces, three and a half lane rounds, two workgroups per chunk) and dim 8192 (32
    super-blocks: the dim / 256 <= 32 edge of k_norm_in, two full rounds)"""
    plans = run_listed(ca, f"rows/{name}")
    for plan in plans.values():
        assert plan["path"] == 2, plan
        assert (plan["k_norm_in"], plan["wo_x_only"], plan["split_wo"]) == (1, 1, 2), plan
        assert plan["split_down"] == (2 if name == "8b-rows" else 1), plan


def test_mixed_layers_every_hand_over(ca):
    """three layers: V Q4_K / wo Q3_K / ffn_down Q3_K, all three Q3_K, all three Q2_K -- k_qkv<Q2_K>'s wave-uniform V branch in both
    formats and k_gemv_res_nq in the tensor's own instantiation, at position 0 (the staged attention, wo quantizes its rhs) and at 100
    (k_attn_flash; wo of every format behind it)"""
    model = build(BY_KEY["mix/tiny-gqa"])
    assert layer_types(model, 3) == [(Q4K, Q3K, Q3K), (Q3K,) * 3, (Q2K,) * 3]
    plans = run_listed(ca, "mix/tiny-gqa")
    for (layer, pos), plan in plans.items():
        assert plan["path"] == 2, plan
        assert (plan["norm_epi_k"], plan["q8k_producers"], plan["k_norm_in"], plan["wo_x_only"]) == (1, 1, 1, 1), plan
        assert plan["attn_variant"] == (0 if pos == 0 else 16 + 2), (layer, pos, plan)


@pytest.mark.parametrize("key,want", [("recipe-K/tiny-gqa", (Q4K, Q3K, Q3K)), ("recipe-K/tiny-mha", (Q3K, Q3K, Q3K)), ("recipe-S/tiny-hd128", None)])
def test_the_recipes(ca, key, want):
    """synth's Q2_K recipe on a group-4 shape (attn_v Q4_K) and on a group-1 shape (attn_v Q3_K), attn_output and ffn_down Q3_K; and
    Q2_K_S on eight layers (ffn_down Q4_K in layer 0 only); the recipes' Q6_K classifier"""
    model = build(BY_KEY[key])
    n = model.shape.n_layers
    assert model.tensors["output.weight"].typ == synth.Q6_K
    assert layer_types(model, n) == ([want] * n if want else [(Q2K, Q2K, Q4K)] + [(Q2K,) * 3] * 7)
    for plan in run_listed(ca, key).values():
        assert plan["path"] == 2, plan


@pytest.mark.parametrize("flag", sorted(FLAG_CASES))
def test_fallback_forms_every_launch(ca, flag):
    """the forms behind the A/B flags (and behind shapes that switch k_norm_in / the producers off), each built for the Q2_K body: the
    plan words of the Q3_K file's FLAG_CASES"""
    flags, words = FLAG_CASES[flag]
    _, _, _, _, seq, positions, layers = BY_KEY["flags/tiny-gqa"]
    plans = run_case(ca, f"{flag}/tiny-gqa", build(BY_KEY["flags/tiny-gqa"]), seq, positions, layers, flags=flags)
    for plan in plans.values():
        assert plan["path"] == 2, plan
        assert tuple(plan[k] for k in ("norm_epi_k", "q8k_producers", "wo_x_only", "qin", "qmode_wo", "qmode_down")) == words, (flag, plan)
        if flags & SPLIT_ALWAYS:
            assert (plan["split_wo"], plan["split_down"]) == (2, 2), plan
        if flags & SPLIT_NEVER:
            assert (plan["split_wo"], plan["split_down"]) == (1, 1), plan


def test_without_the_norm_epilogue_q2k_runs_per_op(ca):
    """the one form the Q2_K body is not built in: decide_step sends the context to the per-op segments, which the tap refuses"""
    model = build(BY_KEY["flags/tiny-gqa"])
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    assert ca.debug_step_plan(conf, w, dev, 64, True, norm_epilogue=False)["path"] == 0
    r = ca.HipLlamaRunner(conf, w, dev, 64, True, True, True, norm_epilogue=False)
    assert H6.error_kind(ca, lambda: r.debug_tap(1, 0, 0)) == H6.NOT_IMPLEMENTED and r.kv_cache_len() == 0


def test_block_field_edges(ca):
    """rows that carry tests/edge_blocks' Q2_K super-blocks through the fused launches (tests/test_q2k_step_ref.edge_model: quants 3 | 0
    x scale nibbles 15 | 0 x min nibbles 15 | 0 on every third super-block; d and dmin of either sign, flipped independently tensor by
    tensor; a few +-0) on the three mixed layers: the same launches, the same caps"""
    plans = run_listed(ca, "edges/tiny-gqa")
    for plan in plans.values():
        assert plan["path"] == 2, plan
        assert (plan["norm_epi_k"], plan["q8k_producers"], plan["k_norm_in"], plan["wo_x_only"], plan["qin"]) == (1, 1, 1, 1, 1), plan


def test_fast_logits_of_a_short_greedy_run(ca):
    """tiny-gqa Q2_K, a 4-token prompt + 6 decode steps: the fused step against the oracle inside the project's Q2_K row (and its
    flip-count gate), the graph against eager launches bit for bit, the reference-API runner (Llama2Runner on the default device: its
    recorded calls reach the same step) bit for bit, and on-device greedy ids equal to host arg-max over the exported logits.
    (Seed 91: on seed 90 the round-to-nearest rhs quantizer flips a quant against the oracle at step 2 on the unchanged per-op segments
    (NO_KQUANT_FUSION) and on the fused step alike, 4.8e-3 at every later step through the KV cache; 91 is the next seed whose per-op
    run carries no flip, plain and as recipe K.  On seeds 15 and 90 .. 99 the two paths show the same error to every printed digit.)"""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], Q2K, seed=91)
    toks = [1, 365, 400, 282, 3, 5, 8, 13, 21, 34]
    odev = o.OracleDevice(thread_num=4, use_avx2=False)
    oconf, ow = to_oracle(model, odev)
    orr = o.OracleLlamaRunner(oconf, ow, odev, 64, True)
    ref = [orr.forward([t], i).copy() for i, t in enumerate(toks)]
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    assert ca.debug_step_plan(conf, w, dev, 64, True)["path"] == 2
    graph, eager = ca.HipLlamaRunner(conf, w, dev, 64, True), ca.HipLlamaRunner(conf, w, dev, 64, True, False)
    trait = ca.Llama2Runner(conf, w, dev, 64, True)
    got = []
    for i, t in enumerate(toks):
        a, b, c = graph.forward(t, i).copy(), eager.forward(t, i).copy(), trait.forward([t], i).copy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"graph vs eager, step {i}"
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), f"Llama2Runner vs HipLlamaRunner, step {i}"
        got.append(a)
    err = [float(np.max(np.abs(g - r)) / np.max(np.abs(r))) for g, r in zip(got, ref)]
    print("fused/tiny-gqa/Q2_K relative errors per step:", ["%.3g" % e for e in err])
    check_fast("q2k-fused/tiny-gqa/Q2_K", "Q2_K", err)
    first = int(o.argmax_last(got[-1]))
    ids = graph.decode_greedy(first, 4)
    assert len(ids) == 4 and graph.kv_cache_len() == len(toks) + 4
    tok, pos = first, len(toks)
    for want in ids:  # the eager twin, one exported step at a time: host arg-max (last maximum) names the same token
        lg = eager.forward(tok, pos)
        tok, pos = int(o.argmax_last(lg)), pos + 1
        assert tok == int(want)


def test_prompt_then_decode_against_the_oracle(ca):
    """a 4-token prompt through the prompt pass (unchanged by the Q2_K body: its kernels are the per-format ones) followed by 6 fused
    decode steps on the Q2_K recipe, every step's logits against the oracle's inside the project's Q2_K row"""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], Q2K, seed=91, q2_k_mix="K")
    prompt, steps = [1, 365, 400, 282], [3, 5, 8, 13, 21, 34]
    odev = o.OracleDevice(thread_num=4, use_avx2=False)
    oconf, ow = to_oracle(model, odev)
    orr = o.OracleLlamaRunner(oconf, ow, odev, 64, True)
    ref = [orr.forward([t], i).copy() for i, t in enumerate(prompt + steps)]
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    assert ca.debug_step_plan(conf, w, dev, 64, True)["path"] == 2
    r = ca.HipLlamaRunner(conf, w, dev, 64, True)
    got = [r.prefill(prompt).copy()]
    for i, t in enumerate(steps):
        got.append(r.forward(t, len(prompt) + i).copy())
    err = [float(np.max(np.abs(g - rr)) / np.max(np.abs(rr))) for g, rr in zip(got, ref[len(prompt) - 1:])]
    print("prompt+decode/tiny-gqa/Q2_K-recipe-K relative errors per step:", ["%.3g" % e for e in err])
    check_fast("prompt+decode/tiny-gqa/Q2_K-recipe-K", "Q2_K", err)


def test_tap_still_refuses_what_it_does_not_serve(ca):
    """NOT_IMPLEMENTED for a strict-order Q2_K context and for a Q2_K body with a Q5_K attn_v (both on the per-op segments); a refused
    tap leaves the context as it was"""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], Q2K, seed=91)
    sdev = ca.HipTensorDevice(0, False, 0, True)
    sconf, sw = synth.to_hip(model, sdev)
    strict = ca.HipLlamaRunner(sconf, sw, sdev, 64, True)
    assert H6.error_kind(ca, lambda: strict.debug_tap(1, 0, 0)) == H6.NOT_IMPLEMENTED
    dev = ca.HipTensorDevice(0)
    other = synth.build_model(synth.SHAPES["tiny-gqa"], Q2K, seed=91, layer_types={1: {"attn_v": synth.Q5_K}})
    oconf, ow = synth.to_hip(other, dev)
    assert ca.debug_step_plan(oconf, ow, dev, 64, True)["path"] == 0
    per_op = ca.HipLlamaRunner(oconf, ow, dev, 64, True)
    assert H6.error_kind(ca, lambda: per_op.debug_tap(1, 0, 0)) == H6.NOT_IMPLEMENTED
    assert strict.kv_cache_len() == per_op.kv_cache_len() == 0
