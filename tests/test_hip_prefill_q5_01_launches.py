"""Every launch of one chunk pass of the fast prompt path over Q5_0 / Q5_1 BODIES pinned against float64, launch by launch and ROW BY
ROW, through tests/test_hip_prefill_launches.run_case and tests/prefill_pass_ref.check_pass, which reads the two formats inside
q5_01_f16w_ref.q5_01_pass (the checker's own tests for them: tests/test_q5_01_pass_ref.py).  From 32 rows every layer matrix runs on
k_gemm_f16w (gemm_f16w.hip: WF_Q5_0 / WF_Q5_1, B' shared with Q4_0 / Q4_1 in slot order 0); a shorter pass, the PREFILL_INT8_GEMM form
and the recomputation of a chunk whose B' overflowed keep the wave-per-row GEMV -- the int8 matrix-core GEMM does not take the two
formats, so their plan words say 3 and never 2.

run_case asserts that the tapped pass's logits and every layer's caches equal a plain prefill's bit for bit and that the tapped layer
passes check_pass; every case here also asserts from the plan that it took the path it is named for.  Gates: GEMV_REL sum |A' B'| (the
f16 GEMM, A' = f16((q5 - 16) d) / f16(q5 d + m) restated by tests/q5_01_f16w_ref.py), row_dots' (nb + C_DOT) U sum |t_b| (the GEMV and the
classifier: Q4_0's derivation for Q5_0, Q4_1's for Q5_1, tests/q5_01_step_ref.py), the interval checks with EXCUSED_CAP, FLASH_ROWS_REL,
bit equality.  No bound is this file's own.

Also here, for every format: a pass in which the range check (f16w_range_ok) refuses ONE matrix of a body whose other matrices take the
GEMM.  The two formats reach it with a block whose weights are all exactly zero (q5_01_f16w_ref.refuse_matrix), so nothing downstream
moves: the one-launch sites for q | k | v and gate | up fall apart, the refused reader gets no B', the next reader still finds one, and
the plan says 3 for exactly that matrix.

Observed error / bound ratios: tests/golden/prefill_q5_01_launch_pins_observed.json and profiles/prefill_q5_01_launch_pins.md (evidence
only).  Not pinned for the two formats (stated, not hidden): the strict device and tensor-parallel ranks (the tap refuses them; the strict
device is bit-exact against the oracle in tests/test_hip_prefill_q5_01.py), Gemma passes."""
import numpy as np
import pytest

from crabml_amd import synth
from tests import edge_blocks as eb
from tests import prefill_pass_ref as P
from tests import q5_01_f16w_ref as Q
from tests import q5_01_step_ref as S
from tests.helpers import record_observed
from tests.test_hip_fused_launches import SHAPE_8B, SHAPE_WIDE
from tests.test_hip_prefill_launches import (EXACT_ATTENTION, FLAG_CASES, INT8_GEMM, NORM_ROWS, NORM_ROWS_H, NORM_ROWS_W, NORM_SEPARATE,
                                             POS0_CASES, ROWS, SEPARATE_F16_ROWS, SMALL, expect_attn, expect_f16, run_case, tokens_of)
from tests.test_q5_01_pass_ref import OVERFLOW_LOG2, REFUSED, XH, XH_WITH, overflow_model, refused_model

pytestmark = pytest.mark.gpu

FMTS = list(Q.FMTS)
WORDS = tuple(P.KERNEL_WORD.values())
F16W, GEMV = P.KERNEL_F16W, P.KERNEL_GEMV
_OBSERVED = {}


def record(key, results):
    _OBSERVED[key] = {"error_over_bound": {k: round(r.worst, 4) for k, r in results.items()},
                      "excused_share": {k: {n: round(v, 4) for n, v in r.excused.items()} for k, r in results.items() if r.excused}}
    record_observed(_OBSERVED, "prefill_q5_01_launch_pins.json")


def build(shape, fmt, seed):
    return synth.build_model(synth.SHAPES[shape] if isinstance(shape, str) else shape, synth.TYPE_BY_NAME[fmt], seed=seed)


def case(ca, key, model, seq, n, layers, kv_f16=True, **kw):
    with Q.q5_01_pass():
        return run_case(ca, key, model, seq, kv_f16, n, layers, rec=record, **kw)


def all_words(plan, kernel):
    assert [plan[w] for w in WORDS] == [kernel] * 7, plan


def expect_gemm(plan, model):
    """the default pass from 32 rows: expect_f16 and all seven matrices on k_gemm_f16w"""
    expect_f16(plan, model)
    all_words(plan, F16W)
    assert XH - {"n1.xh.v"} <= plan["fields"] and "n1.xh.v" not in plan["fields"], plan


def expect_row_dots(plan):
    """a pass without the f16 GEMM: every matrix row by row on the GEMV (3; the int8 matrix-core GEMM, 2, does not take the formats,
    though gemm() asks it first from 16 rows), no B' anywhere"""
    assert plan["f16w"] == 0 and plan["qkv_one"] == 0 and plan["gu_one"] == 0 and plan["h_done"] == 0, plan
    all_words(plan, GEMV)
    assert not XH & plan["fields"], plan
    assert plan["qkv_F"] == plan["down_F"] == 0, plan


# ---- case 1 ----
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", SMALL)
def test_default_pass_every_launch(ca, shape, fmt):
    """the default pass from an empty cache, f16 cache: two row counts per (model, format) -- between them every count of ROWS for each
    format, ragged row and column tiles throughout --, layers 0, 1 and the last"""
    model = build(shape, fmt, 41)
    L = model.shape.n_layers
    i = SMALL.index(shape) + FMTS.index(fmt)
    for n in (ROWS[i % 5], ROWS[(i + 2) % 5]):
        plans = case(ca, f"default/{shape}/{fmt}", model, 400, n, sorted({0, 1, L - 1}))
        for layer, plan in plans.items():
            expect_gemm(plan, model)
            assert plan["attn_kernel"] == expect_attn(model, n), plan
            assert plan["in_parts"] == (plans[layer - 1]["down_parts"] if layer - 1 in plans else plan["in_parts"]), plan


# ---- case 2 ----
@pytest.mark.parametrize("n", [1, 15, 16, 23, 31, 32])
@pytest.mark.parametrize("fmt", FMTS)
def test_the_32_row_edge_and_the_short_passes(ca, fmt, n):
    """below 32 rows: the GEMV for every matrix (also from 16 rows, where gemm() asks the int8 matrix-core GEMM first and it declines),
    k_norm_quant_rows without f16 planes, the exact tile attention; at 32 rows the f16 GEMM"""
    model = build("tiny-gqa", fmt, 42)
    plans = case(ca, f"short/tiny-gqa/{fmt}", model, 64, n, [0, 1])
    for plan in plans.values():
        if n < 32:
            expect_row_dots(plan)
            assert plan["norm_kernel"] == NORM_ROWS and plan["attn_kernel"] == P.ATTN_TILE, plan
        else:
            expect_gemm(plan, model)
            assert plan["attn_kernel"] == P.ATTN_TILE, plan


# ---- case 3 ----
@pytest.mark.parametrize("name", sorted(POS0_CASES))
@pytest.mark.parametrize("shape,fmt", [("tiny-gqa", "Q5_0"), ("tiny-hd128", "Q5_1")])
def test_passes_that_start_inside_the_cache(ca, shape, fmt, name):
    """pos0 > 0: rope positions, the causal mask and the appended cache rows all start at pos0; the attention kernel the table names"""
    setup, seq, kv_f16, chunk, alf, n, attn = POS0_CASES[name]
    model = build(shape, fmt, 44)
    plans = case(ca, f"pos0/{name}/{shape}/{fmt}", model, seq, n, [0, 1], kv_f16=kv_f16, setup=setup, chunk=chunk, attn_long_from=alf)
    for plan in plans.values():
        assert plan["pos0"] > 0 and plan["attn_kernel"] == attn, plan
        assert plan["f16w"] == 1, plan
        all_words(plan, F16W)


@pytest.mark.parametrize("fmt,flags,attn", [("Q5_0", 0, P.ATTN_FLASH_ROWS), ("Q5_1", EXACT_ATTENTION, P.ATTN_LONG_ROWS)])
def test_pass_past_1024_cached_positions(ca, fmt, flags, attn):
    """1000 cached positions, then 40 rows: k_attn_flash_rows on its float64 bound (Q5_0); with EXACT_ATTENTION the exact long-row kernels,
    bit for bit up to 1024 cached positions and inside prefill_pass_ref.long_row_hull beyond (Q5_1)"""
    model = build("tiny-gqa", fmt, 52)
    plans = case(ca, f"past-1024/tiny-gqa/{fmt}", model, 1104, 40, [0, 1], setup=lambda r: r.prefill(tokens_of(model, 1000, salt=1)), flags=flags)
    for plan in plans.values():
        assert plan["pos0"] == 1000 and plan["attn_kernel"] == attn and plan["f16w"] == 1, plan
        all_words(plan, F16W)


# ---- case 4 ----
@pytest.mark.parametrize("flag", sorted(FLAG_CASES))
@pytest.mark.parametrize("shape,fmt", [("tiny-gqa", "Q5_0"), ("tiny-qwen2", "Q5_1")])
def test_flag_forms_every_launch(ca, shape, fmt, flag):
    model = build(shape, fmt, 45)
    plans = case(ca, f"{flag}/{shape}/{fmt}", model, 160, 130, [0, 1], flags=FLAG_CASES[flag])
    for plan in plans.values():
        assert plan["f16w"] == 1, plan
        all_words(plan, F16W)
        if flag == "no-row-fusion":
            assert plan["norm_kernel"] == NORM_SEPARATE and plan["wo_parts"] == 0 and plan["down_parts"] == 0 and plan["h_done"] in (0, 1), plan
        elif flag == "separate-f16-rows":
            assert plan["norm_kernel"] == NORM_ROWS and plan["wo_parts"] == 0 and plan["down_parts"] == 0 and plan["h_done"] in (0, 1), plan
        elif flag == "no-gu-epilogue":
            assert plan["h_done"] == 0 and plan["gu_one"] == 1, plan
        elif flag == "no-tile-attention":
            assert plan["attn_kernel"] == P.ATTN_PER_ROW, plan
        else:
            assert plan["attn_kernel"] == P.ATTN_TILE, plan


# ---- case 5 ----
@pytest.mark.parametrize("fmt", FMTS)
def test_int8_gemm_flag_at_200_rows(ca, fmt):
    """PREFILL_INT8_GEMM stays the A/B (the end-to-end test of tests/test_hip_prefill_q5_01.py leans on it): no f16 GEMM, no B', every
    matrix row by row.  (The GEMM checks look at a Sample of rows: 200 rows x every weight row of float64 row dots is the host's cost,
    not the device's)"""
    model = build("tiny-gqa", fmt, 43)
    plans = case(ca, f"int8-flag/tiny-gqa/{fmt}", model, 256, 200, [0, 1], flags=INT8_GEMM, sample=P.Sample(extra=8, col_tile=16))
    for plan in plans.values():
        expect_row_dots(plan)
        assert plan["norm_kernel"] == NORM_ROWS and plan["attn_kernel"] == P.ATTN_FLASH_ROWS, plan


# ---- case 6 ----
@pytest.mark.parametrize("fmt,n", [("Q5_0", 40), ("Q5_1", 136)])
def test_k_pieces_left_to_the_norm_launch(ca, fmt, n):
    """two layers of the tiny-wide shape (hidden 4096): ffn_down's GEMM is cut into k pieces and their sum is left to the next layer's
    norm launch, which the plan of layer 1 confirms it added"""
    model = build(synth.ModelShape("tiny-wide", 512, 4096, 2, 4, 2, 512, 256, 1e-5, None), fmt, 46)
    plans = case(ca, f"k-pieces/tiny-wide/{fmt}", model, 160, n, [0, 1])
    assert plans[0]["down_parts"] > 0 and plans[0]["down_ksplit"] == plans[0]["down_parts"] + 1, plans[0]
    assert plans[1]["in_parts"] == plans[0]["down_parts"] and plans[1]["norm_kernel"] == NORM_ROWS_H, plans[1]
    assert plans[1]["down_parts"] == 0, plans[1]  # (the last layer's residual is added by k_res_epi: the GEMM reduces its own pieces)
    for plan in plans.values():
        all_words(plan, F16W)


# ---- case 7 ----
WIDE_FFN = synth.ModelShape("wide-ffn", 512, 12288, 1, 4, 2, 512, 256, 1e-5, None)


@pytest.mark.parametrize("fmt", FMTS)
def test_gate_up_epilogue_with_and_without_the_row_quantizer(ca, fmt):
    """the wide-ffn shape (hidden 12288): SiLU * mul is the gate | up GEMM's epilogue -- with the row quantizer behind it (h_done == 2: h is
    taken from the SEPARATE_F16_ROWS twin) and, in that twin form itself, storing h (h_done == 1)"""
    model = build(WIDE_FFN, fmt, 47)
    plans = case(ca, f"gu-epilogue/wide-ffn/{fmt}", model, 160, 136, [0])
    assert plans[0]["h_done"] == 2 and plans[0]["gu_F"] == 2, plans[0]
    all_words(plans[0], F16W)
    plans = case(ca, f"gu-epilogue-h/wide-ffn/{fmt}", model, 160, 136, [0], flags=SEPARATE_F16_ROWS)
    assert plans[0]["h_done"] == 1, plans[0]
    all_words(plans[0], F16W)


# ---- case 8 ----
@pytest.mark.parametrize("name,fmt,n", [("8b-rows", "Q5_0", 40), ("dim8192", "Q5_1", 136)])
def test_real_row_lengths(ca, name, fmt, n):
    """two layers with the 8B row lengths (dim 4096, hidden 14336) and two with dim 8192: the 256-thread norm kernel (k_norm_quant_rows_w),
    ffn_down's k pieces at hidden 14336; the GEMM checks look at prefill_pass_ref.Sample's rows"""
    model = build(SHAPE_8B if name == "8b-rows" else SHAPE_WIDE, fmt, 48)
    plans = case(ca, f"rows/{name}/{fmt}", model, 160, n, [0, 1], sample=P.Sample())
    for plan in plans.values():
        expect_gemm(plan, model)
        assert plan["norm_kernel"] == NORM_ROWS_W, plan
    if name == "8b-rows":
        assert plans[0]["down_parts"] > 0 and plans[1]["in_parts"] == plans[0]["down_parts"], plans


# ---- case 9 ----
def expect_refused(plans, model, nm):
    """layer 0 with matrix nm refused by the range check, layer 1 the control"""
    p = plans[0]
    assert p["f16w"] == 1 and p["recomputed"] == 0, p
    assert {k: p[w] for k, w in P.KERNEL_WORD.items()} == {k: (GEMV if k == nm else F16W) for k in P.KERNEL_WORD}, p
    assert p["qkv_one"] == (0 if nm in ("attn_q", "attn_k") else 1) and p["gu_one"] == (0 if nm == "ffn_up" else 1), p
    # B' is written for a reader that takes the GEMM and for no other.  Behind a refused attn_q the norm launch writes none, attn_k's
    # GEMM makes it (gemm() taps no field for k) and attn_v FINDS it: made == false with xh_if_made, so n1.xh.v is absent too
    assert XH & p["fields"] == XH_WITH[nm], (nm, sorted(XH & p["fields"]))
    if nm == "ffn_up":
        assert p["h_done"] == 0, p  # (no one-launch gate | up, no epilogue: g and u are stored)
    if nm == "attn_q" and model.shape.dim not in (4096, 8192):
        assert p["norm_kernel"] == NORM_ROWS, p  # (no f16 planes and nothing pending in layer 0: the plain row kernel)
    expect_gemm(plans[1], model)


@pytest.mark.parametrize("nm,n", [(m, 77) for m in REFUSED] + [("attn_k", 200), ("ffn_up", 200)])
@pytest.mark.parametrize("fmt", FMTS)
def test_one_matrix_refused_by_the_range_check(ca, fmt, nm, n):
    """the very models tests/test_q5_01_pass_ref.test_mixed_kernel_taps_are_built_and_accepted builds: one block of layer 0's matrix nm
    out of the f16 GEMM's range with all its weights exactly zero.  That matrix alone takes the GEMV; the logits stay finite (run_case)"""
    model, _ = refused_model(fmt, nm)
    plans = case(ca, f"refused/{nm}/tiny-gqa/{fmt}", model, 256, n, [0, 1])
    expect_refused(plans, model, nm)


def test_refused_ffn_down_behind_the_row_quantizer(ca):
    """wide-ffn (hidden 12288), where gate | up quantize h themselves (h_done == 2): with ffn_down refused the launch writes planes and NO
    B' (F16wHQuant.xh == nullptr), and ffn_down's GEMV reads the planes"""
    model = Q.refuse_matrix(build(WIDE_FFN, "Q5_0", 47), "blk.0.ffn_down.weight")
    plans = case(ca, "refused/ffn_down/wide-ffn/Q5_0", model, 160, 136, [0], sample=P.Sample(extra=8, col_tile=16))
    p = plans[0]
    assert p["h_done"] == 2 and p["kernel_down"] == GEMV and "hid.xh" not in p["fields"] and p["f16w"] == 1 and p["recomputed"] == 0, p
    assert [p[w] for w in WORDS if w != "kernel_down"] == [F16W] * 6, p


# ---- case 10 ----
@pytest.mark.parametrize("fmt", FMTS)
def test_block_scales_of_either_sign(ca, fmt):
    model = S.flip_signs(build("tiny-gqa", fmt, 49))
    for plan in case(ca, f"signs/tiny-gqa/{fmt}", model, 128, 77, [0, 1]).values():
        expect_gemm(plan, model)


@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128"])
@pytest.mark.parametrize("fmt", FMTS)
def test_mixed_sign_block_fields(ca, shape, fmt):
    """d and Q5_1's m flipped independently, a few d = +-0 (edge_blocks.flip_scale_signs); the caps were evaluated on these very bytes by
    tests/test_edge_blocks.py"""
    model = eb.mixed_sign_model(shape, synth.TYPE_BY_NAME[fmt], eb.MIXED_SIGN_SEEDS["prefill"])
    for plan in case(ca, f"mixed-signs/{shape}/{fmt}", model, 128, 77, [0, 1]).values():
        expect_gemm(plan, model)


@pytest.mark.parametrize("fmt", FMTS)
def test_shrunk_residual_stream(ca, fmt):
    """a residual stream small enough for RMSNorm's eps to matter in every norm launch, on the GEMM (77 rows) and row by row (23)"""
    model = S.shrink_residual(build("tiny-gqa", fmt, 50))
    for plan in case(ca, f"shrunk/tiny-gqa/{fmt}", model, 128, 77, [0, 1]).values():
        expect_gemm(plan, model)
    for plan in case(ca, f"shrunk-row-dots/tiny-gqa/{fmt}", model, 128, 23, [0, 1]).values():
        expect_row_dots(plan)


# ---- case 11 ----
def test_overflow_recomputation_is_the_row_by_row_pass(ca):
    """The massive-channel model of tests/test_hip_prefill_launches.test_overflow_recomputation_is_the_int8_pass, Q5_0 (Q8_0 rows) with
    Q4_0's factor: two elements of every ffn_norm weight x 2^12.  ffn_down's B' overflows f16 and its writer raises the flag; the chunk
    is computed again without the f16 GEMM -- for these formats that is the GEMV row by row, NOT the int8 matrix-core pass the test's
    ancestor is named for -- and the tapped buffers are the recomputation's.  From the oracle's ops on these 64 tokens
    (tests/test_q5_01_pass_ref.py) max |h| is 2.417e+06 in layer 0 and 1.201e+06 in layer 1: past 65504, below 127 * 65504 = 8.3e6"""
    assert OVERFLOW_LOG2["Q5_0"] == 12
    model = overflow_model("Q5_0")
    plans = case(ca, "overflow/tiny-gqa/Q5_0", model, 80, 64, [0, 1], sample=P.Sample(extra=8, col_tile=16))
    for plan in plans.values():
        assert plan["recomputed"] == 1, plan
        expect_row_dots(plan)


def test_overflow_recomputation_of_a_q5_1_pass_up_to_h(ca):
    """Q5_1 with Q8_0's factor, 2^11: max |h| is 2.824e+05 on the oracle, inside (65504, 127 * 65504) -- but Q5_1's rows are Q8_1 blocks
    whose f16 field s = d * sum q overflows with h, in the reference's own quantizer too, so NO path finishes this pass with finite
    numbers (tests/test_q5_01_pass_ref.test_q5_1_rows_cannot_hold_an_h_that_overflows_f16: no factor does; Q4_1 has no such case either).
    What exists is pinned: the chunk is recomputed row by row (the plan), the tapped buffers are the recomputation's, the tap moves
    nothing (the logits' bits equal a plain prefill's, NaN payloads included), and every launch of layer 0 in front of h -- both norm
    launches, q | k | v, k_qkv_epi_rows, attention, wo, the gate and up GEMVs -- passes its check"""
    model = overflow_model("Q5_1")
    n, seq, layer = 64, 80, 0
    toks = tokens_of(model, n)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    want = np.array(ca.HipLlamaRunner(conf, w, dev, seq, True).prefill(toks))
    r = ca.HipLlamaRunner(conf, w, dev, seq, True)
    before = (r.debug_kv(layer, False, True), r.debug_kv(layer, True, True))
    tap = r.debug_prefill_tap(toks, layer)
    after = (r.debug_kv(layer, False, True), r.debug_kv(layer, True, True))
    plan = dict(tap["plan"], fields=frozenset(k for k in tap if k not in ("plan", "qtype", "logits")))
    assert plan["recomputed"] == 1 and (plan["rows"], plan["pos0"]) == (n, 0), plan
    expect_row_dots(plan)
    assert np.array_equal(tap["logits"].view(np.uint32), want.view(np.uint32))
    form, ctx, sample = P.Form(kv_f16=True, seq_cap=seq), "overflow/tiny-gqa/Q5_1 layer 0", P.Sample(extra=8, col_tile=16)
    with Q.q5_01_pass():
        res = {"embedding": P.check_embedding(tap, model, toks, ctx), "norm n1": P.check_norm(tap, model, layer, "n1", ctx),
               "q|k|v gemm": P.check_qkv_gemm(tap, model, layer, ctx, sample), "k_qkv_epi_rows": P.check_epi(tap, before, after, model, layer, form, ctx),
               "attention": P.check_attention(tap, after, model, layer, form, ctx), "wo": P.check_wo(tap, model, layer, ctx, sample),
               "norm n2": P.check_norm(tap, model, layer, "n2", ctx)}
        gu = res["gate, up gemv"] = P.Result("gate, up gemv")
        for nm, wn in (("g", "ffn_gate"), ("u", "ffn_up")):
            P.check_gemm(gu, tap, model, f"blk.{layer}.{wn}.weight", "n2.act", nm, None, nm, ctx, sample)
    record(f"overflow/tiny-gqa/Q5_1/L{layer}/n{n}/p0", res)
    assert not P.failures(res), "\n".join(P.failures(res)[:40])
    h = np.abs(np.asarray(tap["g"], dtype=np.float64))  # (g, not h: SiLU * mul happens inside the quantizer launch)
    assert np.all(np.isfinite(h)) and not np.all(np.isfinite(np.asarray(tap["down.tmp"]))), "the case no longer overflows Q8_1's s"
