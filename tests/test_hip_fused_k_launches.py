"""Every launch of the fast K-QUANT decode step (enqueue_segment_k: k_qkv<Q4_K>, attention, k_gemv_res_nq<Q4_K, SPLIT, QIN> for wo,
k_gateup_k_lds<QOUT, false, NORMIN>, k_gemv_res_nq for ffn_down, the classifier; k_gemv_res / k_gateup with the stand-alone norm and
quantizer launches without the norm epilogue and for Q4_1 layers in front of a classifier of another format) pinned against float64,
launch by launch: tests/test_hip_fused_launches.py for the other body of the step, with the K forms of tests/fused_step_ref.py (their
derivations: that module's docstring; the checker's own tests: tests/test_fused_step_ref.py).

A runner is teacher-forced greedily on its own tokens up to `pos` (from the graph), then takes ONE tapped step.  The form every launch
is checked in comes from the plan words the enqueue code wrote where it decided, and is then held against what the case is named for.
Where gate | up normalizes and quantizes wo's row in LDS (k_norm_in, the default), a twin context with NO_K_NORM_IN takes the same
tokens and leaves the planes: its wo.x must equal this step's bit for bit, its planes pass the interval check, and h is held to them.
The tapped step's logits equal, bit for bit, those of a twin that took the same tokens from the graph (the tap moves nothing).

Not pinned here (stated, not hidden): the ordered (strict-device) K forms, which are bit-exact to the oracle (tests/test_hip_fused.py),
tensor-parallel ranks, and the K-quant prompt pass.  What the cases left of their bounds on a device: profiles/fused_k_launch_pins.md
(evidence only; the gates are the derived bounds)."""
import numpy as np
import pytest

from crabml_amd import synth
from tests import fused_step_ref as R
from tests.helpers import record_observed
from tests.test_hip_fused_launches import SHAPE_8B, SHAPE_WIDE

pytestmark = pytest.mark.gpu

SPLIT_ALWAYS, NO_RHS_PROLOGUE, NO_Q8K_PRODUCERS, Q8K_ATTN_PRODUCER, NO_K_NORM_IN, Q4_1_SEGMENTS = 16, 1024, 32768, 65536, 16777216, 512
_OBSERVED = {}


def record(key, results):
    _OBSERVED[key] = {"error_over_bound": {k: round(r.worst, 4) for k, r in results.items()},
                      "excused_share": {k: {n: round(v, 6) for n, v in r.excused.items()} for k, r in results.items() if r.excused}}
    record_observed(_OBSERVED, "fused_k_launch_pins.json")


def flip_signs(model, seed=5):
    """block scales of either sign on every K-quant tensor: Q4_K's d and dmin, Q6_K's d (the sign bit of each f16)"""
    rng = np.random.default_rng(seed)
    for t in model.tensors.values():
        at = {synth.Q4_K: (1, 3), synth.Q6_K: (209,)}.get(t.typ, ())
        blk = t.data.reshape(-1, synth.BLOCK_BYTES[t.typ]) if at else None
        for byte in at:
            blk[:, byte] ^= (rng.integers(0, 2, size=blk.shape[0], dtype=np.uint8) << 7)
    return model


def expect_flash(model, kv_f16, pos):
    s = model.shape
    return kv_f16 and s.head_dim in (64, 128, 256) and s.n_heads // s.n_kv_heads in (1, 2, 4, 8) and pos + 1 >= 96


def run_case(ca, key, model, seq, positions, layers, norm_epilogue=True, flags=0, kv_f16=True):
    """-> {(layer, pos): the tapped step's launch plan}"""
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    mk = lambda fl: ca.HipLlamaRunner(conf, w, dev, seq, kv_f16, True, True, norm_epilogue=norm_epilogue, extra_flags=fl)  # noqa: E731
    r, twin, planes_twin = mk(flags), mk(flags), None
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
            assert plan["path"] == 2, (ctx, plan)  # enqueue_segment_k
            flash = plan["attn_variant"] >= 16
            assert flash == expect_flash(model, kv_f16, pos), (ctx, plan)
            assert np.array_equal(tap["logits"].view(np.uint32), want.view(np.uint32)), f"{ctx}: the tapped (eager) step's logits differ from the graph's"
            twin_tap = None
            if plan["wo_x_only"]:  # gate | up's planes exist in LDS only: the twin whose wo leaves them
                if planes_twin is None:
                    planes_twin = mk(flags | NO_K_NORM_IN)
                planes_twin.reset()
                if pos:
                    assert int(planes_twin.decode_greedy(1, pos)[-1]) == tok, ctx
                twin_tap = planes_twin.debug_tap(tok, pos, layer)
                assert twin_tap["plan"]["wo_x_only"] == 0 and twin_tap["plan"]["norm_epi_k"] == 1, (ctx, twin_tap["plan"])
                assert np.array_equal(twin_tap["logits"].view(np.uint32), want.view(np.uint32)), f"{ctx}: the NO_K_NORM_IN twin's logits differ"
            form = R.Form(defer=False, kv_f16=kv_f16, seq_cap=seq, flash_from=pos + 1 if flash else 0)
            kc, vc = r.debug_kv(layer, False, kv_f16), r.debug_kv(layer, True, kv_f16)
            res = R.check_layer(tap, kc, vc, model, layer, pos, form, ctx, twin=twin_tap, token=tok)
            for name, rr in res.items():
                print(f"{ctx} {name}: error / bound {rr.worst:.3f} excused {rr.excused}")
            record(f"{key}/L{layer}/p{pos}", res)
            fails += R.failures(res)
    assert not fails, "\n".join(fails)
    return plans


def q4k(shape, seed, **kw):
    """Q4_K layers with a Q6_K classifier (a Gemma shape: its tied Q4_K embedding)"""
    s = synth.SHAPES[shape] if isinstance(shape, str) else shape
    if s.arch != "gemma":
        kw.setdefault("output_type", synth.Q6_K)
    return synth.build_model(s, synth.Q4_K, seed=seed, **kw)


@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128", "tiny-qwen2", "tiny-qwen2-g7", "tiny-gemma"])
def test_default_fast_step_every_launch(ca, shape):
    """wo leaves x and its chunk sums, gate | up normalizes and quantizes in LDS and emits h's planes, ffn_down copies them and runs the
    norm epilogue: dim 512 (2 super-blocks per row; hidden 1024: 4), dim 1792 (7: the ragged round), head_dim 64 / 128 / 256, Qwen2's
    biases and NEOX pairs, Gemma's GELU and tied classifier"""
    plans = run_case(ca, f"default/{shape}", q4k(shape, 41), 64, [0, 1, 40], [0, 1])
    for plan in plans.values():
        assert (plan["norm_epi_k"], plan["q8k_producers"], plan["k_norm_in"], plan["wo_x_only"], plan["qin"]) == (1, 1, 1, 1, 1), plan
        assert (plan["qmode_wo"], plan["qmode_down"], plan["aq8"], plan["split_wo"]) == (1, 2, 0, 2), plan


# flag form -> (norm_epilogue, flags, the plan words that show it: norm_epi_k, q8k_producers, wo_x_only, qin, qmode_wo, qmode_down, aq8)
FLAG_CASES = {
    "no-k-norm-in": (True, NO_K_NORM_IN, (1, 1, 0, 1, 1, 2, 0)),
    "split-chunks": (True, SPLIT_ALWAYS, (1, 1, 0, 1, 1, 2, 0)),
    "no-rhs-prologue": (True, NO_RHS_PROLOGUE, (1, 0, 0, 0, 0, 0, 0)),
    "no-rhs-prologue+split": (True, NO_RHS_PROLOGUE + SPLIT_ALWAYS, (1, 0, 0, 0, 0, 0, 0)),
    "no-q8k-producers": (True, NO_Q8K_PRODUCERS, (1, 0, 0, 1, 1, 1, 0)),
    "no-q8k-producers+split": (True, NO_Q8K_PRODUCERS + SPLIT_ALWAYS, (1, 0, 0, 1, 1, 1, 0)),
    "attn-producer": (True, Q8K_ATTN_PRODUCER, (1, 1, 1, 1, 2, 2, 1)),
    "attn-producer+split": (True, Q8K_ATTN_PRODUCER + SPLIT_ALWAYS, (1, 1, 0, 1, 2, 2, 1)),
    "separate-norm": (False, 0, (0, 0, 0, 0, 0, 0, 0)),
}


@pytest.mark.parametrize("flag", sorted(FLAG_CASES))
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-qwen2-g7"])
def test_flag_forms_every_launch(ca, shape, flag):
    """the forms behind the A/B flags; `separate-norm`: k_gemv_res<Q4_K> with the stand-alone norm and quantizer launches"""
    ne, flags, words = FLAG_CASES[flag]
    plans = run_case(ca, f"{flag}/{shape}", q4k(shape, 42), 64, [0, 7], [0, 1], norm_epilogue=ne, flags=flags)
    for plan in plans.values():
        got = tuple(plan[k] for k in ("norm_epi_k", "q8k_producers", "wo_x_only", "qin", "qmode_wo", "qmode_down", "aq8"))
        assert got == words, (flag, plan)
        if flags & SPLIT_ALWAYS:
            assert (plan["split_wo"], plan["split_down"]) == (2, 2), plan
        elif words[0]:
            assert (plan["split_wo"], plan["split_down"]) == (2 if words[2] else 1, 1), plan


@pytest.mark.parametrize("flags", [0, SPLIT_ALWAYS, NO_RHS_PROLOGUE])
def test_q4_k_m_mix(ca, flags):
    """llama.cpp's Q4_K_M recipe on 8 layers (use_more_bits: 0, 3, 6, 7): layers whose attn_v / ffn_down are Q6_K and one without"""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_K, seed=43, n_layers=8, k_m_mix=True)
    plans = run_case(ca, f"k-m-mix/tiny-gqa/{flags}", model, 64, [0, 7], [3, 4, 7], flags=flags)
    for (layer, pos), plan in plans.items():  # (layer 7: its Q6_K ffn_down leaves the classifier's planes)
        assert (plan["v_q6k"], plan["down_q6k"]) == ((0, 0) if layer == 4 else (1, 1)), plan
        assert plan["qin"] == (0 if flags & NO_RHS_PROLOGUE else 1) and plan["norm_epi_k"] == 1, plan


@pytest.mark.parametrize("flags", [0, Q4_1_SEGMENTS])
def test_q4_1_layers_on_this_body(ca, flags):
    """k_qkv<Q4_1>, k_gemv_res<Q4_1>, k_gateup<Q4_1> and the Q8_1 quantizer launches: a Q4_1 model in front of a Q6_K classifier, and a
    plain one under Q4_1_SEGMENTS"""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_1, seed=44, output_type=None if flags else synth.Q6_K)
    plans = run_case(ca, f"q4_1/tiny-gqa/{flags}", model, 64, [0, 7], [0, 1], flags=flags)
    for plan in plans.values():
        assert (plan["norm_epi_k"], plan["qin"], plan["qmode_wo"], plan["qmode_down"], plan["split_wo"]) == (0, 0, 0, 0, 0), plan


def test_attention_switch_positions(ca):
    """94 / 95 cached positions on the staged one-workgroup kernel (the reference's arithmetic, bit for bit), k_attn_flash from 96"""
    plans = run_case(ca, "switch/tiny-gqa", q4k("tiny-gqa", 45), 256, [94, 95, 96, 200], [0, 1])
    for layer in (0, 1):
        assert [plans[(layer, p)]["attn_variant"] for p in (94, 95, 96, 200)] == [0, 16 + 2, 16 + 2, 16 + 2]


@pytest.mark.parametrize("name", ["8b-rows", "dim8192"])
def test_real_row_lengths(ca, name):
    """dim 4096 / hidden 14336 (ffn_down rows of 56 super-blocks, two workgroups per chunk) and dim 8192 (32 super-blocks: the
    dim / 256 <= 32 edge of k_norm_in, and dim / 32 == the compute units of this part)"""
    model = q4k(SHAPE_8B if name == "8b-rows" else SHAPE_WIDE, 46)
    plans = run_case(ca, f"rows/{name}", model, 128, [0, 3], [0, 1])
    for plan in plans.values():
        assert (plan["k_norm_in"], plan["wo_x_only"], plan["split_wo"]) == (1, 1, 2), plan
        assert plan["split_down"] == (2 if name == "8b-rows" else 1), plan


def test_block_scales_of_either_sign(ca):
    run_case(ca, "signs/tiny-gqa", flip_signs(q4k("tiny-gqa", 47)), 64, [0, 5], [0, 1])
    run_case(ca, "signs/tiny-gqa/k-m-mix", flip_signs(synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_K, seed=47, k_m_mix=True)), 64, [5], [0, 1])


@pytest.mark.parametrize("shape,mix", [("tiny-gqa", False), ("tiny-gqa", True), ("tiny-hd128", False)])
def test_mixed_sign_block_fields(ca, shape, mix):
    """d / dmin flipped independently and a few d = +-0 (tests/edge_blocks.flip_scale_signs), Q4_K and the Q4_K_M mix: the default
    forms, as the plain models take them"""
    from tests import edge_blocks as eb
    kw = {"k_m_mix": True} if mix else {"output_type": synth.Q6_K}
    model = eb.mixed_sign_model(shape, synth.Q4_K, eb.MIXED_SIGN_SEEDS["fused_k"], **kw)
    plans = run_case(ca, f"mixed-signs/{shape}/{'k-m-mix' if mix else 'Q4_K'}", model, 64, [0, 5], [0, 1])
    for plan in plans.values():
        assert plan["qin"] == 1 and plan["norm_epi_k"] == 1, plan
        if not mix:
            assert (plan["norm_epi_k"], plan["q8k_producers"], plan["k_norm_in"], plan["wo_x_only"], plan["qin"]) == (1, 1, 1, 1, 1), plan
            assert (plan["qmode_wo"], plan["qmode_down"], plan["aq8"], plan["split_wo"]) == (1, 2, 0, 2), plan


@pytest.mark.parametrize("mix", [False, True])
def test_shrunk_residual_stream(ca, mix):
    """a residual stream small enough for RMSNorm's eps to matter in every launch (fused_step_ref.shrink_residual).  By 2^-9 here: the
    synthetic K-quant weights are larger per element than the Q4_0 ones (6-bit sub-block scales on top of d), and 2^-7 leaves a mean
    square of 0.09, above the 2e-2 the five-launch test asks for.  The block scales d / dmin become f16 subnormals on the way."""
    model = R.shrink_residual(synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_K, seed=48, k_m_mix=True) if mix else q4k("tiny-gqa", 48), log2=9)
    run_case(ca, f"shrunk/tiny-gqa/{'k-m-mix' if mix else 'Q4_K'}", model, 64, [0, 5], [0, 1])
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    x = np.asarray(ca.HipLlamaRunner(conf, w, dev, 64, True).debug_tap(1, 0, 1)["wo.x"], dtype=np.float64)
    assert np.mean(x * x) < 2e-2, np.mean(x * x)


def error_kind(ca, call):
    with pytest.raises(ca.CrabmlError) as e:
        call()
    return int(str(e.value).split("ErrorKind(")[1].split(")")[0])


def test_tap_still_refuses_what_it_does_not_serve(ca):
    """NOT_IMPLEMENTED for the ordered K forms of a strict-order device and for a tensor-parallel rank; a refused tap leaves the context
    as it was.  (A context on the runner's own KV cache is refused by the same test of the hook; the recorded-op queue owns those and
    no HipLlamaRunner does, so it cannot be tried from here.)"""
    NOT_IMPLEMENTED = 9  # crabml_hip_status
    from crabml_amd import tp as tp_mod
    model = q4k("tiny-gqa", 49)
    sdev = ca.HipTensorDevice(0, False, 0, True)
    sconf, sw = synth.to_hip(model, sdev)
    strict = ca.HipLlamaRunner(sconf, sw, sdev, 64, True)
    assert error_kind(ca, lambda: strict.debug_tap(1, 0, 0)) == NOT_IMPLEMENTED
    dev = ca.HipTensorDevice(0)
    tconf, tw = synth.to_hip(tp_mod.shard_model(model, 2, 0, True), dev)
    rank = ca.HipLlamaRunner(tconf, tw, dev, 64, True, True, True, 2, 0)
    assert error_kind(ca, lambda: rank.debug_tap(1, 0, 0)) == NOT_IMPLEMENTED
    assert strict.kv_cache_len() == rank.kv_cache_len() == 0
