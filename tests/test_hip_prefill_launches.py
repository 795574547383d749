"""Every launch of one chunk pass of the fast prompt path (prefill_chunk_pass: the norm-row kernels, the f16 / int8 GEMMs, k_qkv_epi_rows,
attention, SiLU * mul, the residual hand-off, the final norm and the classifier) pinned against float64, launch by launch and ROW BY
ROW (tests/prefill_pass_ref.py; the checker's own tests: tests/test_prefill_pass_ref.py).

A runner is brought to the case's starting state (empty, after decode steps, after an earlier prefill), then takes ONE tapped pass
(HipLlamaRunner.debug_prefill_tap: the row buffers of one layer copied out between its launches).  Each launch is compared with the
float64 restatement of what it computes FROM THE BYTES IT READ, within bounds derived from roundings; the tapped pass's logits and the
K / V caches of every layer equal, bit for bit, those of a twin runner's plain prefill of the same tokens (the tap moves nothing); and
each case asserts from the launch plan -- written by the enqueue code where it decides -- that the path it is named for was taken.

K-quant (Q8_K row) passes -- Q4_K, Q5_K, Q6_K layers and the Q4_K_M / Q5_K_M mixes -- are pinned the same way, through this file's
run_case, in tests/test_hip_prefill_k_launches.py; Q2_K / Q3_K bodies in tests/test_hip_prefill_q23k_launches.py; Q5_0 / Q5_1 bodies in
tests/test_hip_prefill_q5_01_launches.py.  Not pinned here (stated, not hidden): Gemma passes, Q8_K / F32 weights, tensor-parallel ranks and the strict device (bit-exact against the oracle: tests/test_hip_prefill.py).  What the cases were seen to leave of their bounds on a device: profiles/prefill_launch_pins.md and
tests/golden/prefill_launch_pins_observed.json (evidence only; the gates are the derived bounds)."""
import numpy as np
import pytest

from crabml_amd import synth
from tests import fused_step_ref as R
from tests import prefill_pass_ref as P
from tests.helpers import record_observed
from tests.test_hip_fused_launches import SHAPE_8B, SHAPE_WIDE, flip_signs

pytestmark = pytest.mark.gpu

NO_ROW_FUSION, INT8_GEMM, SEPARATE_F16_ROWS, NO_GU_EPILOGUE, NO_TILE_ATTENTION, EXACT_ATTENTION = 262144, 524288, 33554432, 67108864, 2048, 4194304
NORM_SEPARATE, NORM_ROWS, NORM_ROWS_H, NORM_ROWS_W = 0, 1, 2, 3  # CRABML_HIP_PFPLAN_NORM_KERNEL
_OBSERVED = {}


def record(key, results):
    _OBSERVED[key] = {"error_over_bound": {k: round(r.worst, 4) for k, r in results.items()},
                      "excused_share": {k: {n: round(v, 4) for n, v in r.excused.items()} for k, r in results.items() if r.excused}}
    record_observed(_OBSERVED, "prefill_launch_pins.json")


def tokens_of(model, n, salt=0):
    return [(7 * i + 3 + 13 * salt) % model.shape.vocab for i in range(n)]


def run_case(ca, key, model, seq, kv_f16, n, layers, setup=None, flags=0, chunk=0, attn_long_from=0, sample=None, rec=None):
    """-> {layer: the tapped pass's launch plan, with the names of the fields the tap returned under "fields"}.  rec: where the observed
    ratios go (default: this file's record)"""
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    mk = lambda extra=0: ca.HipLlamaRunner(conf, w, dev, seq, kv_f16, extra_flags=flags | extra, attn_long_from=attn_long_from, prefill_chunk=chunk)
    s = model.shape
    toks = tokens_of(model, n)
    form = P.Form(kv_f16=kv_f16, seq_cap=seq)
    fails, plans = [], {}
    twin = mk()
    if setup:
        setup(twin)
    pos0 = twin.kv_cache_len()
    want = np.array(twin.prefill(toks))
    assert np.all(np.isfinite(want)), key
    for layer in layers:
        ctx = f"{key} layer {layer} rows {n} pos0 {pos0}"
        # a runner of its own per tapped layer, on the weights uploaded once above (a context refers to them, it holds no copy): a cache
        # that an earlier tap of the same tokens had filled would already hold the rows this pass has to write
        r = mk()
        if setup:
            setup(r)
        assert r.kv_cache_len() == pos0, ctx
        before = (r.debug_kv(layer, False, kv_f16), r.debug_kv(layer, True, kv_f16))
        tap = r.debug_prefill_tap(toks, layer)
        assert r.kv_cache_len() == pos0 + n == twin.kv_cache_len(), ctx
        plan = plans[layer] = dict(tap["plan"], fields=frozenset(k for k in tap if k not in ("plan", "qtype", "logits")))
        assert (plan["rows"], plan["pos0"]) == (n, pos0), (ctx, plan)
        # the tap moves nothing: logits and every layer's cache are the plain prefill's, bit for bit
        assert np.array_equal(tap["logits"].view(np.uint32), want.view(np.uint32)), f"{ctx}: the tapped pass's logits differ from prefill's"
        for l in range(s.n_layers):  # (the live positions: what lies behind them is whatever the allocation held)
            for v in (False, True):
                mine, theirs = (P.cache_view(x.debug_kv(l, v, kv_f16), form, s.n_kv_heads, s.head_dim)[:, :pos0 + n] for x in (r, twin))
                assert np.array_equal(mine.view(np.uint8), theirs.view(np.uint8)), f"{ctx}: layer {l} {'V' if v else 'K'} cache differs from prefill's"
        after = (r.debug_kv(layer, False, kv_f16), r.debug_kv(layer, True, kv_f16))
        other = None
        if plan["h_done"] == 2:  # h never leaves the launch: the twin form that stores it (bit-identical: tests/test_hip_prefill.py)
            t2 = mk(SEPARATE_F16_ROWS)
            if setup:
                setup(t2)
            other = t2.debug_prefill_tap(toks, layer)
            assert other["plan"]["h_done"] == 1, (ctx, other["plan"])
        res = P.check_pass(tap, toks, before, after, model, layer, form, ctx, sample, other)
        for name, rr in res.items():
            print(f"{ctx} {name}: error / bound {rr.worst:.3f} excused {rr.excused}")
        (rec or record)(f"{key}/L{layer}/n{n}/p{pos0}", res)
        fails += P.failures(res)
    assert not fails, "\n".join(fails[:40])
    return plans


def expect_f16(plan, model, fused=True):
    """the default f16 pass: every GEMM on k_gemm_f16w, q | k | v and gate | up as one launch each, B' written by the row kernels"""
    assert plan["f16w"] == 1 and plan["recomputed"] == 0, plan
    assert plan["qkv_one"] == 1 and plan["gu_one"] == 1, plan
    assert all(plan[k] in (1, 2) for k in ("qkv_F", "wo_F", "gu_F", "down_F")) and all(plan[k] in (2, 4, 8) for k in ("qkv_T", "wo_T", "gu_T", "down_T")), plan
    if fused:
        assert plan["norm_kernel"] == (NORM_ROWS_W if model.shape.dim in (4096, 8192) else NORM_ROWS_H), plan


def expect_attn(model, end):
    """f16 cache: k_attn_flash_rows from attn_long_from (96) cached positions at the pass's end where the geometry has it (head_dim 64 /
    128, group size 1 / 2 / 4 / 8); below, the exact tile kernel; group sizes it does not cover: k_attn per (head, row)"""
    s = model.shape
    grp_ok = s.n_heads // s.n_kv_heads in (1, 2, 4, 8)
    if grp_ok and s.head_dim in (64, 128) and end >= 96:
        return P.ATTN_FLASH_ROWS
    return P.ATTN_TILE if grp_ok else P.ATTN_PER_ROW


SMALL = ["tiny-gqa", "15m", "tiny-hd128", "tiny-qwen2", "tiny-qwen2-g7"]
ROWS = [33, 77, 130, 200, 384]


@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0", "Q4_1"])
@pytest.mark.parametrize("shape", SMALL)
def test_default_f16_pass_every_launch(ca, shape, fmt):
    """the default pass from an empty cache, f16 cache: two row counts per (model, format) -- between them every count of ROWS on every
    model or format, ragged row and column tiles throughout --, layers 0, 1 and the last"""
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=41)
    L = model.shape.n_layers
    i = SMALL.index(shape) + ["Q4_0", "Q8_0", "Q4_1"].index(fmt)
    for n in (ROWS[i % 5], ROWS[(i + 2) % 5]):
        plans = run_case(ca, f"default/{shape}/{fmt}", model, 400, True, n, sorted({0, 1, L - 1}))
        for layer, plan in plans.items():
            expect_f16(plan, model)
            assert plan["attn_kernel"] == expect_attn(model, n), plan
            assert plan["in_parts"] == (plans[layer - 1]["down_parts"] if layer - 1 in plans else plan["in_parts"]), plan


@pytest.mark.parametrize("fmt,n", [("Q4_0", 1), ("Q8_0", 5), ("Q4_1", 16), ("Q4_0", 23), ("Q8_0", 31), ("Q4_1", 31)])
def test_short_passes_take_the_int8_kernels(ca, fmt, n):
    """below 32 rows: the GEMV (under 16 rows) and the int8 matrix-core GEMM, k_norm_quant_rows without f16 planes, the exact tile attention"""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.TYPE_BY_NAME[fmt], seed=42)
    plans = run_case(ca, f"int8/tiny-gqa/{fmt}", model, 64, True, n, [0, 1])
    for plan in plans.values():
        assert plan["f16w"] == 0 and plan["qkv_one"] == 0 and plan["gu_one"] == 0 and plan["h_done"] == 0, plan
        assert plan["norm_kernel"] == NORM_ROWS and plan["attn_kernel"] == P.ATTN_TILE, plan
        assert plan["qkv_F"] == plan["down_F"] == 0, plan


@pytest.mark.parametrize("shape,fmt", [("tiny-gqa", "Q4_0"), ("tiny-qwen2", "Q8_0"), ("tiny-hd128", "Q4_1")])
def test_int8_gemm_flag_at_200_rows(ca, shape, fmt):
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=43)
    plans = run_case(ca, f"int8-flag/{shape}/{fmt}", model, 256, True, 200, [0, 1], flags=INT8_GEMM)
    for plan in plans.values():
        assert plan["f16w"] == 0 and plan["norm_kernel"] == NORM_ROWS and plan["attn_kernel"] == P.ATTN_FLASH_ROWS, plan


POS0_CASES = {
    "after-decode": (lambda r: r.decode_greedy(1, 9), 256, True, 0, 0, 40, P.ATTN_TILE),
    "after-prefill": (lambda r: r.prefill([5, 6, 7, 8, 9, 10, 11]), 256, True, 0, 0, 77, P.ATTN_TILE),
    "second-chunk": (lambda r: r.prefill(list(range(3, 43))), 256, True, 48, 0, 45, P.ATTN_TILE),
    "below-the-switch": (lambda r: r.prefill(list(range(3, 23))), 256, True, 0, 0, 70, P.ATTN_TILE),
    "across-the-switch": (lambda r: r.prefill(list(range(3, 23))), 256, True, 0, 0, 90, P.ATTN_FLASH_ROWS),
    "f32-cache": (lambda r: r.prefill(list(range(3, 23))), 256, False, 0, 0, 90, P.ATTN_TILE),
    "short-after-long": (lambda r: r.prefill(list(range(3, 203))), 256, True, 0, 0, 33, P.ATTN_FLASH_ROWS),
}


@pytest.mark.parametrize("case", sorted(POS0_CASES))
@pytest.mark.parametrize("shape,fmt", [("tiny-gqa", "Q4_0"), ("tiny-qwen2", "Q8_0"), ("tiny-hd128", "Q4_1")])
def test_passes_that_start_inside_the_cache(ca, shape, fmt, case):
    """pos0 > 0: rope positions, the causal mask and the appended cache rows all start at pos0.  The exact tile kernel below
    attn_long_from (96) cached positions at the pass's end, k_attn_flash_rows from there on (f16 cache) -- asserted from the plan"""
    setup, seq, kv_f16, chunk, alf, n, attn = POS0_CASES[case]
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=44)
    plans = run_case(ca, f"pos0/{case}/{shape}/{fmt}", model, seq, kv_f16, n, [0, 1], setup=setup, chunk=chunk, attn_long_from=alf)
    for plan in plans.values():
        assert plan["pos0"] > 0 and plan["attn_kernel"] == attn, plan
        assert plan["f16w"] == 1, plan


def test_pass_past_1024_cached_positions(ca):
    """1000 cached positions, then 40 rows: the pass ends past 1024, where the exact tile kernel no longer applies -- k_attn_flash_rows on
    its float64 bound, rope and cache rows at positions 1000 .. 1039"""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=52)
    plans = run_case(ca, "past-1024/tiny-gqa/Q4_0", model, 1104, True, 40, [0, 1], setup=lambda r: r.prefill(tokens_of(model, 1000, salt=1)))
    for plan in plans.values():
        assert plan["pos0"] == 1000 and plan["attn_kernel"] == P.ATTN_FLASH_ROWS and plan["f16w"] == 1, plan


def test_pass_past_1024_on_the_exact_long_row_kernels(ca):
    """the same pass with EXACT_ATTENTION: k_attn_scores / k_attn_softmax / k_attn_pv_rows, rows in grid.y.  Rows of up to 1024 cached
    positions (0 .. 23) are the reference's attention bit for bit; beyond, the softmax row sum is a block tree and the row must lie in
    the hull of the reference's f16 chain over every admissible sum (prefill_pass_ref.long_row_hull).  Every other launch as usual."""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=52)
    plans = run_case(ca, "past-1024-exact/tiny-gqa/Q4_0", model, 1104, True, 40, [0, 1], setup=lambda r: r.prefill(tokens_of(model, 1000, salt=1)),
                     flags=EXACT_ATTENTION)
    for plan in plans.values():
        assert plan["pos0"] == 1000 and plan["attn_kernel"] == P.ATTN_LONG_ROWS and plan["f16w"] == 1, plan


FLAG_CASES = {"no-row-fusion": NO_ROW_FUSION, "separate-f16-rows": SEPARATE_F16_ROWS, "no-gu-epilogue": NO_GU_EPILOGUE,
              "no-tile-attention": NO_TILE_ATTENTION | EXACT_ATTENTION, "exact-attention": EXACT_ATTENTION}


@pytest.mark.parametrize("flag", sorted(FLAG_CASES))
@pytest.mark.parametrize("shape,fmt", [("tiny-gqa", "Q4_0"), ("15m", "Q8_0"), ("tiny-qwen2", "Q4_1")])
def test_flag_forms_every_launch(ca, shape, fmt, flag):
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=45)
    plans = run_case(ca, f"{flag}/{shape}/{fmt}", model, 160, True, 130, [0, 1], flags=FLAG_CASES[flag])
    for plan in plans.values():
        assert plan["f16w"] == 1, plan
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


@pytest.mark.parametrize("fmt,n", [("Q4_0", 40), ("Q8_0", 136), ("Q4_1", 77)])
def test_k_pieces_left_to_the_norm_launch(ca, fmt, n):
    """the tiny-wide shape of tests/test_hip_prefill.py (hidden 4096, two layers here): ffn_down's GEMM is cut into k pieces and their sum is
    left to the next layer's norm launch, which the plan of layer 1 confirms it added"""
    model = synth.build_model(synth.ModelShape("tiny-wide", 512, 4096, 2, 4, 2, 512, 256, 1e-5, None), synth.TYPE_BY_NAME[fmt], seed=46)
    plans = run_case(ca, f"k-pieces/tiny-wide/{fmt}", model, 160, True, n, [0, 1])
    assert plans[0]["down_parts"] > 0 and plans[0]["down_ksplit"] == plans[0]["down_parts"] + 1, plans[0]
    assert plans[1]["in_parts"] == plans[0]["down_parts"] and plans[1]["norm_kernel"] == NORM_ROWS_H, plans[1]
    assert plans[1]["down_parts"] == 0, plans[1]  # (the last layer's residual is added by k_res_epi: the GEMM reduces its own pieces)


@pytest.mark.parametrize("fmt", ["Q4_0", "Q4_1"])
def test_gate_up_epilogue_with_and_without_the_row_quantizer(ca, fmt):
    """the wide-ffn shape (hidden 12288): 64-row tiles of gate and up cover the chip, so SiLU * mul is the GEMM's epilogue -- with the row
    quantizer behind it (h_done == 2: h is taken from the SEPARATE_F16_ROWS twin) and, in that twin form itself, storing h (h_done == 1)"""
    model = synth.build_model(synth.ModelShape("wide-ffn", 512, 12288, 1, 4, 2, 512, 256, 1e-5, None), synth.TYPE_BY_NAME[fmt], seed=47)
    plans = run_case(ca, f"gu-epilogue/wide-ffn/{fmt}", model, 160, True, 136, [0])
    assert plans[0]["h_done"] == 2 and plans[0]["gu_F"] == 2, plans[0]
    plans = run_case(ca, f"gu-epilogue-h/wide-ffn/{fmt}", model, 160, True, 136, [0], flags=SEPARATE_F16_ROWS)
    assert plans[0]["h_done"] == 1, plans[0]


@pytest.mark.parametrize("name,fmt,n", [("8b-rows", "Q4_0", 136), ("8b-rows", "Q8_0", 40), ("dim8192", "Q4_0", 40), ("dim8192", "Q4_1", 136)])
def test_real_row_lengths(ca, name, fmt, n):
    """two layers with the 8B row lengths (dim 4096, hidden 14336) and two with dim 8192: the 256-thread norm kernel (k_norm_quant_rows_w),
    ffn_down's k pieces at hidden 14336; the GEMM checks look at a fixed sample of weight rows and prompt rows (prefill_pass_ref.Sample:
    the first and last 64-row tile of every matrix, the first and last column tile of the pass, the row at pos0)"""
    shape = SHAPE_8B if name == "8b-rows" else SHAPE_WIDE
    model = synth.build_model(shape, synth.TYPE_BY_NAME[fmt], seed=48)
    plans = run_case(ca, f"rows/{name}/{fmt}", model, 160, True, n, [0, 1], sample=P.Sample())
    for layer, plan in plans.items():
        expect_f16(plan, model)
        assert plan["norm_kernel"] == NORM_ROWS_W, plan
    if name == "8b-rows":
        assert plans[0]["down_parts"] > 0 and plans[1]["in_parts"] == plans[0]["down_parts"], plans


@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0", "Q4_1"])
def test_block_scales_of_either_sign(ca, fmt):
    model = flip_signs(synth.build_model(synth.SHAPES["tiny-gqa"], synth.TYPE_BY_NAME[fmt], seed=49))
    plans = run_case(ca, f"signs/tiny-gqa/{fmt}", model, 128, True, 77, [0, 1])
    for plan in plans.values():
        expect_f16(plan, model)


@pytest.mark.parametrize("shape,fmt", [("tiny-gqa", "Q4_0"), ("tiny-gqa", "Q8_0"), ("tiny-gqa", "Q4_1"), ("tiny-hd128", "Q4_1")])
def test_mixed_sign_block_fields(ca, shape, fmt):
    """d and Q4_1's m flipped independently, a few d = +-0 (tests/edge_blocks.flip_scale_signs): the default f16 pass, as for the
    plain model"""
    from tests import edge_blocks as eb
    model = eb.mixed_sign_model(shape, synth.TYPE_BY_NAME[fmt], eb.MIXED_SIGN_SEEDS["prefill"])
    plans = run_case(ca, f"mixed-signs/{shape}/{fmt}", model, 128, True, 77, [0, 1])
    for plan in plans.values():
        expect_f16(plan, model)


def test_shrunk_residual_stream(ca):
    """a residual stream small enough for RMSNorm's eps to matter in every norm launch (fused_step_ref.shrink_residual)"""
    for fmt in ("Q4_0", "Q8_0"):
        model = R.shrink_residual(synth.build_model(synth.SHAPES["tiny-gqa"], synth.TYPE_BY_NAME[fmt], seed=50))
        run_case(ca, f"shrunk/tiny-gqa/{fmt}", model, 128, True, 77, [0, 1])
        run_case(ca, f"shrunk-int8/tiny-gqa/{fmt}", model, 128, True, 23, [0, 1])


@pytest.mark.parametrize("fmt,log2", [("Q4_0", 12), ("Q8_0", 11)])
def test_overflow_recomputation_is_the_int8_pass(ca, fmt, log2):
    """The massive-channel model of test_fast_prompt_pass_recomputes_a_chunk_whose_f16_rows_overflow with Q8_0 rows: two elements of
    every ffn_norm weight x 2^log2.  h = silu(g) * u then reaches 1e5 .. 2e6: past 65504, so ffn_down's B' = f16(q d) is +-inf and its
    writer raises the flag, but below 127 * 65504 = 8.3e6, so the blocks' f16 scales -- the reference's own format -- stay finite and so
    does the int8 pass (2^16, the Q4_K test's factor, puts h past that: Q8_0 rows cannot hold it on any path).  The chunk is computed
    again with the int8 kernels; the tapped buffers are the recomputation's (the plan says so) and satisfy the int8 checks, the cache rows
    are the recomputation's, everything is finite."""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.TYPE_BY_NAME[fmt], seed=5)
    s = model.shape
    for l in range(s.n_layers):
        t = model.tensors[f"blk.{l}.ffn_norm.weight"]
        w = t.data.view(np.float32).copy()
        w[[3, s.dim // 2 + 1]] *= np.float32(2.0 ** log2)
        t.data = w.view(np.uint8)
    plans = run_case(ca, f"overflow/tiny-gqa/{fmt}", model, 80, True, 64, [0, 1])
    for plan in plans.values():
        assert plan["recomputed"] == 1 and plan["f16w"] == 0 and plan["qkv_F"] == 0, plan


def error_kind(ca, call):
    with pytest.raises(ca.CrabmlError) as e:
        call()
    return int(str(e.value).split("ErrorKind(")[1].split(")")[0])


def test_tap_rejects_what_it_does_not_serve(ca):
    """BAD_INPUT for a pass longer than one chunk and for a layer the model does not have; NOT_IMPLEMENTED on the strict device, on a
    tensor-parallel rank and for formats it does not serve (Q2_K layers: Q8_K rows, but no restated kernel).  A Q4_K runner's tap
    succeeds and advances the cache by the pass.  (An ext_kv context is refused by the same test of the hook; no
    HipLlamaRunner owns one, so it is not tried here.)  A refused tap leaves the context as it was."""
    BAD_INPUT, NOT_IMPLEMENTED = 5, 9  # crabml_hip_status
    from crabml_amd import tp as tp_mod
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=51)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    r = ca.HipLlamaRunner(conf, w, dev, 64, True, prefill_chunk=16)
    assert error_kind(ca, lambda: r.debug_prefill_tap(tokens_of(model, 17), 0)) == BAD_INPUT  # longer than one chunk pass
    assert error_kind(ca, lambda: r.debug_prefill_tap(tokens_of(model, 8), model.shape.n_layers)) == BAD_INPUT
    assert error_kind(ca, lambda: r.debug_prefill_tap([], 0)) == BAD_INPUT
    assert r.kv_cache_len() == 0
    sdev = ca.HipTensorDevice(0, False, 0, True)
    sconf, sw = synth.to_hip(model, sdev)
    strict = ca.HipLlamaRunner(sconf, sw, sdev, 64, True)
    assert error_kind(ca, lambda: strict.debug_prefill_tap(tokens_of(model, 8), 0)) == NOT_IMPLEMENTED  # the strict device
    tconf, tw = synth.to_hip(tp_mod.shard_model(model, 2, 0, True), dev)
    rank = ca.HipLlamaRunner(tconf, tw, dev, 64, True, True, True, 2, 0)
    assert error_kind(ca, lambda: rank.debug_prefill_tap(tokens_of(model, 8), 0)) == NOT_IMPLEMENTED  # a tensor-parallel rank
    kq = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q2_K, seed=51)
    kconf, kw = synth.to_hip(kq, dev)
    kr = ca.HipLlamaRunner(kconf, kw, dev, 64, True)
    assert error_kind(ca, lambda: kr.debug_prefill_tap(tokens_of(kq, 40), 0)) == NOT_IMPLEMENTED  # a format the tap does not serve
    assert strict.kv_cache_len() == rank.kv_cache_len() == kr.kv_cache_len() == 0
    k4 = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_K, seed=51)
    k4conf, k4w = synth.to_hip(k4, dev)
    k4r = ca.HipLlamaRunner(k4conf, k4w, dev, 64, True)
    tap = k4r.debug_prefill_tap(tokens_of(k4, 40), 0)  # K-quant layers are served
    assert tap["plan"]["rows"] == 40 and k4r.kv_cache_len() == 40
