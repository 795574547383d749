"""Every launch of one chunk pass of the fast prompt path over Q8_K ROWS (K-quant layers: Q4_K, Q5_K, Q6_K and the Q4_K_M / Q5_K_M
mixes) pinned against float64, launch by launch and ROW BY ROW: the two norm arms (k_res_epi + k_norm_f32_rows + the quantizer below
192 rows, k_norm_quant_rows_k from 192), B' in either k-slot order, k_gemm_f16w on Q4_K / Q6_K operands, the int8 matrix-core GEMMs
k_gemm_mfma_q4k / _q6k, the wave-per-row GEMVs (short passes; every Q5_K matrix), k_gateup_epi, the tail.

The cases go through tests/test_hip_prefill_launches.run_case (one tapped pass per layer, compared by tests/prefill_pass_ref.py; the
tapped logits and every layer's cache bit-equal to a plain prefill of the same tokens) and assert from the launch plan -- one word per
matrix for the kernel it took, written by the enqueue code where it decides -- that the path they are named for ran.  The checker's
own tests: tests/test_prefill_pass_ref.py.  What the cases were seen to leave of their bounds: profiles/prefill_k_launch_pins.md and
tests/golden/prefill_k_launch_pins_observed.json (evidence only; the gates are the derived bounds).

Not pinned here (stated, not hidden): Gemma passes, tensor-parallel ranks, the strict device, Q8_K / Q2_K / Q3_K weights, the
per-(head, row) attention past 1024 positions."""
import numpy as np
import pytest

from crabml_amd import synth
from tests import fused_step_ref as R
from tests import prefill_pass_ref as P
from tests import q5k_step_ref as Q5
from tests.helpers import record_observed
from tests.test_hip_fused_k_launches import flip_signs
from tests.test_hip_fused_launches import SHAPE_8B, SHAPE_WIDE
from tests.test_hip_prefill_launches import (INT8_GEMM, NO_GU_EPILOGUE, NO_ROW_FUSION, NORM_SEPARATE, POS0_CASES, SEPARATE_F16_ROWS, expect_attn,
                                             run_case)

pytestmark = pytest.mark.gpu

NORM_ROWS_K = 4  # CRABML_HIP_PFPLAN_NORM_KERNEL: k_norm_quant_rows_k
F16W, INT8, GEMV = P.KERNEL_F16W, P.KERNEL_INT8, P.KERNEL_GEMV
MATS = {"q": "attn_q", "k": "attn_k", "v": "attn_v", "wo": "attn_output", "gate": "ffn_gate", "up": "ffn_up", "down": "ffn_down"}
XH = ("n1.xh", "n1.xh.v", "attn.xh", "n2.xh", "hid.xh")
FMTS = {"Q4_K": (synth.Q4_K, False), "Q4_K_M": (synth.Q4_K, True), "Q6_K": (synth.Q6_K, False), "Q5_K": (synth.Q5_K, False),
        "Q5_K_M": (synth.Q5_K, True)}
_OBSERVED = {}


def record(key, results):
    _OBSERVED[key] = {"error_over_bound": {k: round(r.worst, 4) for k, r in results.items()},
                      "excused_share": {k: {n: round(v, 4) for n, v in r.excused.items()} for k, r in results.items() if r.excused}}
    record_observed(_OBSERVED, "prefill_k_launch_pins.json")


def k_model(shape, fmt, seed):
    wtype, mix = FMTS[fmt]
    return synth.build_model(synth.SHAPES[shape] if isinstance(shape, str) else shape, wtype, seed=seed, k_m_mix=mix)


def case(ca, key, model, seq, n, layers, **kw):
    return run_case(ca, key, model, seq, kw.pop("kv_f16", True), n, layers, rec=record, **kw)


def expect_kernels(plan, model, layer, default):
    """every matrix of the layer on the kernel its format takes in this pass: a Q5_K matrix on the row-by-row GEMV whatever the pass
    allows, a Q4_K / Q6_K matrix on `default`"""
    for m, nm in MATS.items():
        typ = model.tensors[f"blk.{layer}.{nm}.weight"].typ
        assert plan["kernel_" + m] == (GEMV if typ == synth.Q5_K else default), (m, plan)


def expect_norm(plan, n, fused=True):
    assert plan["norm_kernel"] == (NORM_ROWS_K if fused and n >= 192 else NORM_SEPARATE), plan
    assert {"n1.xn", "n2.xn", "cls.xn", "n1.act.qp", "attn.act.qp", "n2.act.qp", "hid.act.qp", "cls.act.qp"} <= plan["fields"], plan


def expect_f16_layer(plan, model, layer, n):
    """the default pass from 32 rows: k_gemm_f16w on every Q4_K / Q6_K matrix; q | k | v one launch where the three share a format, else
    three, with v re-making B' in Q6_K's k-slot order"""
    assert plan["f16w"] == 1 and plan["recomputed"] == 0, plan
    expect_kernels(plan, model, layer, F16W)
    expect_norm(plan, n)
    typ = {m: model.tensors[f"blk.{layer}.{nm}.weight"].typ for m, nm in MATS.items()}
    if typ["q"] == typ["k"] == typ["v"] != synth.Q5_K:
        assert plan["qkv_one"] == 1 and "n1.xh" in plan["fields"] and "n1.xh.v" not in plan["fields"], plan
    else:
        assert plan["qkv_one"] == 0 and plan["kernel_v"] == F16W and "n1.xh.v" in plan["fields"], plan
    assert plan["gu_one"] == (0 if typ["gate"] == synth.Q5_K else 1), plan


SMALL = ["tiny-gqa", "tiny-hd128", "tiny-qwen2", "tiny-qwen2-g7"]
ROWS_SEPARATE, ROWS_FUSED = [40, 77, 130], [192, 200, 384]


@pytest.mark.parametrize("fmt", ["Q4_K", "Q4_K_M", "Q6_K"])
@pytest.mark.parametrize("shape", SMALL)
def test_default_pass_every_launch(ca, shape, fmt):
    """the default pass from an empty cache: one row count of either norm arm per (model, format) -- between them 40, 77, 130 (separate
    launches) and 192, 200, 384 (k_norm_quant_rows_k) on every model and format --, layers 0, 1 and the last (the two-layer shapes:
    layer 1 of a *_K_M mix holds the Q6_K attn_v and ffn_down)"""
    model = k_model(shape, fmt, 61)
    L = model.shape.n_layers
    i = SMALL.index(shape) + ["Q4_K", "Q4_K_M", "Q6_K"].index(fmt)
    mixed = 0
    for n in (ROWS_SEPARATE[i % 3], ROWS_FUSED[i % 3]):
        plans = case(ca, f"default/{shape}/{fmt}", model, 400, n, sorted({0, 1, L - 1}))
        for layer, plan in plans.items():
            expect_f16_layer(plan, model, layer, n)
            assert plan["attn_kernel"] == expect_attn(model, n), plan
            assert plan["h_done"] in (0, 1) and ("hid.h" in plan["fields"]) == (plan["h_done"] == 0), plan  # (the launcher's choice)
            mixed += plan["qkv_one"] == 0
    assert mixed == (2 if fmt == "Q4_K_M" else 0)  # (layer 1 at both row counts)


def test_the_switch_between_the_norm_arms(ca):
    """the same model and tokens at 191 and 192 rows: the four separate launches, then k_norm_quant_rows_k"""
    model = k_model("tiny-gqa", "Q4_K_M", 62)
    for n, kernel in ((191, NORM_SEPARATE), (192, NORM_ROWS_K)):
        plans = case(ca, "switch/tiny-gqa/Q4_K_M", model, 256, n, [0, 1])
        for layer, plan in plans.items():
            assert plan["norm_kernel"] == kernel, plan
            expect_f16_layer(plan, model, layer, n)


@pytest.mark.parametrize("n", [40, 200])
@pytest.mark.parametrize("fmt", ["Q5_K", "Q5_K_M"])
def test_q5_k_bodies_run_row_by_row(ca, fmt, n):
    """a Q5_K matrix takes no matrix-core GEMM: launch_gemv row by row, whatever the pass allows; the Q6_K matrices of the mix (layer 1:
    attn_v, ffn_down) still take k_gemm_f16w, with B' made for them alone.  (200 rows: the GEMV checks look at a sample of prompt rows
    and weight rows, chosen before any device value is seen; the row kernels have no column tile to straddle)"""
    model = k_model("tiny-gqa", fmt, 63)
    plans = case(ca, f"q5k/tiny-gqa/{fmt}", model, 256, n, [0, 1], sample=P.Sample(extra=8, col_tile=16) if n == 200 else None)
    for layer, plan in plans.items():
        assert plan["f16w"] == 1 and plan["qkv_one"] == 0 and plan["gu_one"] == 0 and plan["h_done"] == 0, plan  # (f16w: what the pass allows)
        expect_kernels(plan, model, layer, F16W)
        expect_norm(plan, n)
        q6 = [m for m, nm in MATS.items() if model.tensors[f"blk.{layer}.{nm}.weight"].typ == synth.Q6_K]
        assert q6 == (["v", "down"] if fmt == "Q5_K_M" and layer == 1 else []), q6
        assert ("n1.xh.v" in plan["fields"]) == ("hid.xh" in plan["fields"]) == bool(q6), plan
        assert not {"n1.xh", "attn.xh", "n2.xh"} & plan["fields"], plan


@pytest.mark.parametrize("n", [1, 5, 15, 16, 23, 31])
@pytest.mark.parametrize("fmt", ["Q4_K", "Q6_K"])
def test_short_passes(ca, fmt, n):
    """below 32 rows: the wave-per-row GEMV under 16 rows, k_gemm_mfma_q4k / _q6k from 16; no B' anywhere"""
    model = k_model("tiny-gqa", fmt, 64)
    plans = case(ca, f"short/tiny-gqa/{fmt}", model, 64, n, [0, 1])
    for layer, plan in plans.items():
        assert plan["f16w"] == 0 and plan["qkv_one"] == 0 and plan["gu_one"] == 0 and plan["h_done"] == 0, plan
        expect_kernels(plan, model, layer, GEMV if n < 16 else INT8)
        expect_norm(plan, n)
        assert not set(XH) & plan["fields"] and plan["attn_kernel"] == P.ATTN_TILE, plan


@pytest.mark.parametrize("fmt", ["Q4_K", "Q4_K_M"])
def test_int8_gemm_flag_at_200_rows(ca, fmt):
    model = k_model("tiny-gqa", fmt, 65)
    plans = case(ca, f"int8-flag/tiny-gqa/{fmt}", model, 256, 200, [0, 1], flags=INT8_GEMM)
    for layer, plan in plans.items():
        assert plan["f16w"] == 0 and not set(XH) & plan["fields"], plan
        expect_kernels(plan, model, layer, INT8)
        expect_norm(plan, 200)


@pytest.mark.parametrize("flag", ["no-row-fusion", "separate-f16-rows", "no-gu-epilogue"])
def test_flag_forms_at_200_rows(ca, flag):
    flags = {"no-row-fusion": NO_ROW_FUSION, "separate-f16-rows": SEPARATE_F16_ROWS, "no-gu-epilogue": NO_GU_EPILOGUE}[flag]
    model = k_model("tiny-gqa", "Q4_K", 66)
    plans = case(ca, f"{flag}/tiny-gqa/Q4_K", model, 256, 200, [0, 1], flags=flags)
    for layer, plan in plans.items():
        assert plan["f16w"] == 1, plan
        expect_kernels(plan, model, layer, F16W)
        expect_norm(plan, 200, fused=flag != "no-row-fusion")
        if flag != "no-gu-epilogue":
            assert plan["wo_parts"] == 0 and plan["down_parts"] == 0, plan  # (no norm launch takes pieces: every GEMM reduces its own)
        else:
            assert plan["h_done"] == 0 and plan["gu_one"] == 1, plan
        assert {"n1.xh", "attn.xh", "n2.xh", "hid.xh"} <= plan["fields"], plan  # (no mirror: every GEMM makes B' itself)


@pytest.mark.parametrize("fmt", ["Q4_K", "Q4_K_M"])
def test_k_pieces_left_to_the_norm_launch(ca, fmt):
    """the two-layer tiny-wide shape (hidden 4096): ffn_down's GEMM of layer 0 is cut into k pieces whose sum is left to layer 1's
    k_norm_quant_rows_k"""
    model = k_model(synth.ModelShape("tiny-wide", 512, 4096, 2, 4, 2, 512, 256, 1e-5, None), fmt, 67)
    plans = case(ca, f"k-pieces/tiny-wide/{fmt}", model, 256, 200, [0, 1])
    assert plans[0]["down_parts"] > 0 and plans[0]["down_ksplit"] == plans[0]["down_parts"] + 1, plans[0]
    assert plans[1]["in_parts"] == plans[0]["down_parts"] and plans[1]["norm_kernel"] == NORM_ROWS_K, plans[1]
    assert plans[1]["down_parts"] == 0, plans[1]
    for layer, plan in plans.items():
        expect_f16_layer(plan, model, layer, 200)


def test_gate_up_epilogue_stores_h(ca):
    """the wide-ffn shape (hidden 12288): SiLU * mul is the gate | up GEMM's epilogue; with Q8_K rows h leaves as f32 (h_done == 1) and the
    row quantizer keeps its own launch"""
    model = k_model(synth.ModelShape("wide-ffn", 512, 12288, 1, 4, 2, 512, 256, 1e-5, None), "Q4_K", 68)
    plans = case(ca, "gu-epilogue/wide-ffn/Q4_K", model, 256, 200, [0])
    assert plans[0]["h_done"] == 1 and plans[0]["gu_one"] == 1 and "hid.h" not in plans[0]["fields"], plans[0]
    expect_f16_layer(plans[0], model, 0, 200)


@pytest.mark.parametrize("name,fmt", [("8b-rows", "Q4_K_M"), ("dim8192", "Q4_K")])
def test_real_row_lengths(ca, name, fmt):
    """two layers with the 8B row lengths (dim 4096, hidden 14336: 16 and 56 super-blocks) and two with dim 8192 at 200 rows: both
    instantiations of k_norm_quant_rows_k (norm_nit 4 and 12), ffn_down's k pieces at hidden 14336; the GEMM checks look at
    prefill_pass_ref.Sample's rows"""
    model = k_model(SHAPE_8B if name == "8b-rows" else SHAPE_WIDE, fmt, 69)
    plans = case(ca, f"rows/{name}/{fmt}", model, 256, 200, [0, 1], sample=P.Sample())
    for layer, plan in plans.items():
        expect_f16_layer(plan, model, layer, 200)
    if name == "8b-rows":
        assert plans[0]["down_parts"] > 0 and plans[1]["in_parts"] == plans[0]["down_parts"], plans


@pytest.mark.parametrize("name", ["after-decode", "second-chunk", "across-the-switch"])
def test_passes_that_start_inside_the_cache(ca, name):
    setup, seq, kv_f16, chunk, alf, n, attn = POS0_CASES[name]
    model = k_model("tiny-gqa", "Q4_K", 70)
    plans = case(ca, f"pos0/{name}/tiny-gqa/Q4_K", model, seq, n, [0, 1], kv_f16=kv_f16, setup=setup, chunk=chunk, attn_long_from=alf)
    for layer, plan in plans.items():
        assert plan["pos0"] > 0 and plan["attn_kernel"] == attn, plan
        expect_f16_layer(plan, model, layer, n)


@pytest.mark.parametrize("n", [77, 200])
def test_super_block_scales_of_either_sign(ca, n):
    model = flip_signs(k_model("tiny-gqa", "Q4_K_M", 71))
    plans = case(ca, "signs/tiny-gqa/Q4_K_M", model, 256, n, [0, 1])
    for layer, plan in plans.items():
        expect_f16_layer(plan, model, layer, n)


@pytest.mark.parametrize("fmt", ["Q4_K", "Q4_K_M"])
def test_mixed_sign_block_fields(ca, fmt):
    """d / dmin flipped independently and a few d = +-0 (tests/edge_blocks.flip_scale_signs): the default pass at 77 rows"""
    from tests import edge_blocks as eb
    wtype, mix = FMTS[fmt]
    model = eb.mixed_sign_model("tiny-gqa", wtype, eb.MIXED_SIGN_SEEDS["prefill_k"], k_m_mix=mix)
    plans = case(ca, f"mixed-signs/tiny-gqa/{fmt}", model, 256, 77, [0, 1])
    for layer, plan in plans.items():
        expect_f16_layer(plan, model, layer, 77)


@pytest.mark.parametrize("n", [77, 200])
@pytest.mark.parametrize("fmt", ["Q4_K_M", "Q5_K_M"])
def test_shrunk_residual_stream(ca, fmt, n):
    """a residual stream small enough for RMSNorm's eps to matter in every norm launch of either arm (by 2^-9, as the decode pins'
    device case: fused_step_ref.shrink_residual / q5k_step_ref.shrink_residual)"""
    shrink = Q5.shrink_residual if fmt == "Q5_K_M" else R.shrink_residual
    model = shrink(k_model("tiny-gqa", fmt, 72), 9)
    plans = case(ca, f"shrunk/tiny-gqa/{fmt}", model, 256, n, [0, 1], sample=P.Sample(extra=8, col_tile=16) if (fmt, n) == ("Q5_K_M", 200) else None)
    for layer, plan in plans.items():
        expect_kernels(plan, model, layer, F16W)
        expect_norm(plan, n)


def test_overflow_recomputation_is_the_int8_pass(ca):
    """the massive-channel Q4_K model of test_fast_prompt_pass_recomputes_a_chunk_whose_f16_rows_overflow (two elements of every ffn_norm
    weight x 2^16): B' overflows f16, the chunk is computed again on the int8 kernels, and the tapped buffers are the recomputation's"""
    model = k_model("tiny-gqa", "Q4_K", 5)
    s = model.shape
    for l in range(s.n_layers):
        t = model.tensors[f"blk.{l}.ffn_norm.weight"]
        w = t.data.view(np.float32).copy()
        w[[3, s.dim // 2 + 1]] *= np.float32(2.0 ** 16)
        t.data = w.view(np.uint8)
    plans = case(ca, "overflow/tiny-gqa/Q4_K", model, 80, 64, [0, 1])
    for layer, plan in plans.items():
        assert plan["recomputed"] == 1 and plan["f16w"] == 0 and plan["qkv_F"] == 0, plan
        expect_kernels(plan, model, layer, INT8)
        assert not set(XH) & plan["fields"], plan
