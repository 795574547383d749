"""Every launch of the fast fused decode step (enqueue_segment_t: k_qkv, attention, k_gemv_res_nq for wo, k_gateup_q, k_gemv_res_nq
for ffn_down, the classifier) pinned against float64, launch by launch (tests/fused_step_ref.py; the checker's own tests:
tests/test_fused_step_ref.py).

A runner is teacher-forced greedily on its own tokens up to `pos` (from the graph), then takes ONE tapped step
(HipLlamaRunner.debug_tap: eager, the buffers of one layer copied out between its launches).  Each launch is compared with the
float64 restatement of what it computes FROM THE BYTES IT READ, within bounds derived from f32 roundings; the tapped step's logits
equal, bit for bit, those of a twin runner that took the same tokens from the graph (the tap moves nothing).

Not pinned here (stated, not hidden): attention without k_attn_flash past 1024 cached positions (f32 cache / head_dim 48): its
softmax row sum is a block tree there, not the reference's scalar loop, so "bit for bit" does not apply and no f32 bound is
derived for it yet; tensor-parallel ranks, the strict device (other kernels; see the module docstrings of
tests/test_hip_fused.py).  The step's other body, the K-quant launches of enqueue_segment_k, is pinned the same way in
tests/test_hip_fused_k_launches.py.  The other half of the fast tier, the prompt pass, is pinned the same way, row by row, in
tests/test_hip_prefill_launches.py (there the long-row kernels past 1024 cached positions are held to the hull of the reference's f16
chain over every admissible row sum: prefill_pass_ref.long_row_hull)."""
import numpy as np
import pytest

from crabml_amd import synth
from tests import fused_step_ref as R
from tests.helpers import EXACT_NORM, record_observed

pytestmark = pytest.mark.gpu

SPLIT_ALWAYS, NO_STAGED = 16, 8192
_OBSERVED = {}

# the two one-layer-pair shapes with the 8B row lengths and a small vocabulary
SHAPE_8B = synth.ModelShape("8b-rows", 4096, 14336, 2, 32, 8, 1024, 128, 1e-5, None)
SHAPE_WIDE = synth.ModelShape("dim8192", 8192, 1024, 2, 64, 8, 1024, 128, 1e-5, None)


def record(key, results):
    _OBSERVED[key] = {"error_over_bound": {k: round(r.worst, 4) for k, r in results.items()},
                      "excused_share": {k: {n: round(v, 4) for n, v in r.excused.items()} for k, r in results.items() if r.excused}}
    record_observed(_OBSERVED, "fused_launch_pins.json")


def flip_signs(model, seed=5):
    """block scales d of either sign on every Q4_0 / Q8_0 / Q4_1 tensor (synth.flip_scale_signs does Q4_0): no common-mode
    component for a wrong kernel to hide behind"""
    rng = np.random.default_rng(seed)
    for t in model.tensors.values():
        if t.typ in (synth.Q4_0, synth.Q8_0, synth.Q4_1):
            blk = t.data.reshape(-1, synth.BLOCK_BYTES[t.typ])
            blk[:, 1] ^= (rng.integers(0, 2, size=blk.shape[0], dtype=np.uint8) << 7)
    return model


def expect_defer(model, norm_epilogue, flags, n_cu):
    """the hop-free norm where a case names it: Q4_0 / Q8_0 layers with the norm epilogue and without EXACT_NORM, every chunk's workgroup
    resident (n_cu: the device's own count, from the tap's launch plan)"""
    return model.wtype in (synth.Q4_0, synth.Q8_0) and norm_epilogue and not (flags & EXACT_NORM) and model.shape.dim // 32 <= n_cu


def expect_flash(model, kv_f16, pos):
    """k_attn_flash where a case names it: f16 cache, head_dim 64 / 128, group size 1 / 2 / 4 / 8, from 96 cached positions"""
    s = model.shape
    return kv_f16 and s.head_dim in (64, 128) and s.n_heads // s.n_kv_heads in (1, 2, 4, 8) and pos + 1 >= 96


def run_case(ca, key, model, seq, kv_f16, positions, layers, norm_epilogue=True, flags=0):
    """-> {(layer, pos): the tapped step's launch plan}.  The form every launch is checked in comes from the CONTEXT (the plan words the
    enqueue code wrote where it decided), and is then held against what the case is named for."""
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    mk = lambda: ca.HipLlamaRunner(conf, w, dev, seq, kv_f16, True, True, norm_epilogue=norm_epilogue, extra_flags=flags)
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
            defer, flash = plan["defer_norm"] == 1, plan["attn_variant"] >= 16
            # the path the case names is the path taken
            assert defer == expect_defer(model, norm_epilogue, flags, plan["n_cu"]), (ctx, plan)
            assert ("wo.rsums" in tap) == defer, (ctx, plan)  # (the buffer exists only in a hop-free context)
            assert plan["norm_epilogue"] == (1 if norm_epilogue and model.shape.dim // 32 <= plan["n_cu"] else 0), (ctx, plan)
            assert flash == expect_flash(model, kv_f16, pos), (ctx, plan)
            assert np.array_equal(tap["logits"].view(np.uint32), want.view(np.uint32)), f"{ctx}: the tapped (eager) step's logits differ from the graph's"
            form = R.Form(defer=defer, kv_f16=kv_f16, seq_cap=seq, flash_from=pos + 1 if flash else 0)
            kc, vc = r.debug_kv(layer, False, kv_f16), r.debug_kv(layer, True, kv_f16)
            res = R.check_layer(tap, kc, vc, model, layer, pos, form, ctx)
            for name, rr in res.items():
                print(f"{ctx} {name}: error / bound {rr.worst:.3f} excused {rr.excused}")
            record(f"{key}/L{layer}/p{pos}", res)
            fails += R.failures(res)
    assert not fails, "\n".join(fails)
    return plans


SMALL = ["15m", "tiny-gqa", "tiny-hd128", "tiny-qwen2", "tiny-qwen2-g7"]


@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0", "Q4_1"])
@pytest.mark.parametrize("shape", SMALL)
def test_default_step_every_launch(ca, shape, fmt):
    """the default step (hop-free for Q4_0 / Q8_0, exact-norm launches with Q8_1 planes for Q4_1), f16 cache: layers 0, 1 and the
    last, positions 0, 1 and 40 (the reference's attention arithmetic, bit for bit)"""
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=31)
    L = model.shape.n_layers
    run_case(ca, f"default/{shape}/{fmt}", model, 64, True, [0, 1, 40], sorted({0, 1, L - 1}))


FLAG_CASES = {"exact-norm": (True, EXACT_NORM), "split-chunks+exact-norm": (True, SPLIT_ALWAYS + EXACT_NORM), "split-chunks": (True, SPLIT_ALWAYS),
              "separate-norm": (False, 0), "no-staged-attention": (True, NO_STAGED)}


@pytest.mark.parametrize("kv_f16", [True, False])
@pytest.mark.parametrize("flag", sorted(FLAG_CASES))
@pytest.mark.parametrize("shape,fmt", [("tiny-gqa", "Q4_0"), ("15m", "Q8_0"), ("tiny-qwen2", "Q4_0"), ("tiny-hd128", "Q4_1")])
def test_flag_forms_every_launch(ca, shape, fmt, flag, kv_f16):
    ne, flags = FLAG_CASES[flag]
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=32)
    run_case(ca, f"{flag}/{shape}/{fmt}/kv{'16' if kv_f16 else '32'}", model, 64, kv_f16, [0, 7], [0, 1], norm_epilogue=ne, flags=flags)


@pytest.mark.parametrize("shape,fmt,kv_f16", [("tiny-gqa", "Q4_0", True), ("tiny-hd128", "Q8_0", True), ("tiny-qwen2", "Q4_0", True),
                                              ("15m", "Q4_0", True), ("tiny-gqa", "Q8_0", False), ("tiny-hd128", "Q4_1", True)])
def test_attention_switch_positions(ca, shape, fmt, kv_f16):
    """95 / 96 / 97 cached positions around attn_long_from (k_attn_flash takes over where the geometry has it; the 15m model's
    head_dim of 48 and an f32 cache stay on the one-workgroup kernel) and 200; the Q4_1 body runs k_attn_flash's own instantiation, which
    writes Q8_1 planes"""
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=33)
    plans = run_case(ca, f"switch/{shape}/{fmt}/kv{'16' if kv_f16 else '32'}", model, 256, kv_f16, [94, 95, 96, 200], [1])
    flash = kv_f16 and shape != "15m"
    # 2: below 768 cached positions the merge runs inside the k_attn_flash launch
    assert [plans[(1, p)]["attn_variant"] for p in (94, 95, 96, 200)] == ([0, 16 + 2, 16 + 2, 16 + 2] if flash else [0, 0, 0, 0])


def test_flash_attention_past_1024_positions(ca):
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=34)
    plans = run_case(ca, "past-1024/tiny-gqa/Q4_0", model, 1280, True, [1030], [0, 1])
    assert plans[(0, 1030)]["attn_variant"] == 16 + 1  # k_attn_flash with the merge launch


@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0", "Q4_1"])
def test_block_scales_of_either_sign(ca, fmt):
    model = flip_signs(synth.build_model(synth.SHAPES["tiny-gqa"], synth.TYPE_BY_NAME[fmt], seed=35))
    run_case(ca, f"signs/tiny-gqa/{fmt}", model, 64, True, [0, 5], [0, 1])


@pytest.mark.parametrize("shape,fmt", [("tiny-gqa", "Q4_0"), ("tiny-gqa", "Q8_0"), ("tiny-gqa", "Q4_1"), ("tiny-hd128", "Q4_1")])
def test_mixed_sign_block_fields(ca, shape, fmt):
    """d and Q4_1's m flipped INDEPENDENTLY (flip_signs above moves d alone, so m stays tied to it), and a few blocks with d = +-0
    (tests/edge_blocks.flip_scale_signs).  run_case holds the plan words against the case: the same launches as the plain model's."""
    from tests import edge_blocks as eb
    model = eb.mixed_sign_model(shape, synth.TYPE_BY_NAME[fmt], eb.MIXED_SIGN_SEEDS["fused"])
    run_case(ca, f"mixed-signs/{shape}/{fmt}", model, 64, True, [0, 5], [0, 1])


def test_q4_0_body_with_a_q6_k_classifier(ca):
    """out_qt != qt: the classifier reads Q8_K planes of its own (k_norm_f32 + the quantizer launch); the layers stay hop-free"""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=36, output_type=synth.Q6_K)
    run_case(ca, "q6k-classifier/tiny-gqa/Q4_0", model, 64, True, [0, 5], [0, 1])


def test_shrunk_residual_stream(ca):
    """a residual stream small enough for RMSNorm's eps to matter in every launch (fused_step_ref.shrink_residual): on the plain
    synthetic models the wrong eps moves 1 / rms by 1.3e-5 at most and, from a mean square of ~75 on, not at all"""
    for fmt in ("Q4_0", "Q8_0"):
        model = R.shrink_residual(synth.build_model(synth.SHAPES["tiny-gqa"], synth.TYPE_BY_NAME[fmt], seed=37))
        run_case(ca, f"shrunk/tiny-gqa/{fmt}", model, 64, True, [0, 5], [0, 1])
        x = np.asarray(_last_x(ca, model), dtype=np.float64)
        assert np.mean(x * x) < 2e-2, np.mean(x * x)


def _last_x(ca, model):
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    return ca.HipLlamaRunner(conf, w, dev, 64, True).debug_tap(1, 0, 1)["wo.x"]


@pytest.mark.parametrize("name,fmt,flags", [("8b-rows", "Q4_0", 0), ("8b-rows", "Q8_0", 0), ("8b-rows", "Q4_0", EXACT_NORM), ("dim8192", "Q4_0", 0),
                                            ("dim8192", "Q8_0", EXACT_NORM)])
def test_real_row_lengths(ca, name, fmt, flags):
    """two layers with the 8B row lengths (dim 4096, hidden 14336, 32 heads / 8 kv: ffn_down rows of 448 blocks) and two with dim
    8192 / hidden 1024 (wo rows of 256 blocks, the long-row norm launch): split_of(k) == 2, and with Q4_0 at dim 4096 the 128-unit form
    of the deferred q|k|v loader (rows_partial_rms_128) -- each asserted from the launch plan the context wrote while it enqueued the step"""
    shape = SHAPE_8B if name == "8b-rows" else SHAPE_WIDE
    model = synth.build_model(shape, synth.TYPE_BY_NAME[fmt], seed=38)
    plans = run_case(ca, f"rows/{name}/{fmt}/{'exact-norm' if flags else 'default'}", model, 128, True, [0, 3], [0, 1], flags=flags)
    for (layer, pos), plan in plans.items():
        assert plan["defer_norm"] == (0 if flags else 1), plan
        # two workgroups per 32-row chunk where the rhs is long: ffn_down at hidden 14336, wo at dim 8192
        assert (plan["split_wo"], plan["split_down"]) == ((1, 2) if name == "8b-rows" else (2, 1)), plan
        # layer 0 reads the planes of its own norm launch (rows past 4096 elements: k_norm_quant<12>); layer 1 those of layer 0's ffn_down
        assert plan["norm_nit"] == ((4 if name == "8b-rows" else 12) if layer == 0 else 0), plan
        if layer == 1 and not flags:  # the deferred loader; its 128-unit form at dim 4096 with Q4_0 (one unit per block)
            assert plan["qkv_loader"] == (4 if name == "8b-rows" and fmt == "Q4_0" else 3), plan
        else:
            assert plan["qkv_loader"] in (1, 2), plan
