"""tests/prefill_pass_ref.check_pass reading Q5_0 / Q5_1 bodies (inside q5_01_f16w_ref.q5_01_pass) decides what
tests/test_hip_prefill_q5_01_launches.py can see, so it is tested first, without a device, in the form of
tests/test_prefill_pass_ref.py: oracle-made taps of both arms -- every matrix on the f16 GEMM (h stored, or only its planes), every
matrix on the row-by-row GEMV -- must be ACCEPTED with every excused share under the cap, then every mutation of
test_prefill_pass_ref.MUTATIONS and every one of the six subtly wrong loaders of q5_01_step_ref.WRONG must be REJECTED, on every model.

Also here, before any device value exists: the taps of a pass in which the range check refuses ONE matrix (its neighbours keep the GEMM)
are built and accepted, field presence included; the models of the GPU file's interval-check cases (flipped scale signs, a shrunk
residual stream) stay under EXCUSED_CAP from the reference alone; the massive-channel model of its overflow case puts h past 65504
and below 127 * 65504 (Q5_0) -- and, a finding, no such model gives a Q5_1 pass that the reference itself can finish: Q8_1's f16 field
s = d * sum q overflows with h.

Seeds.  Every model here is the first seed tried: 21 (the checker's own tests), 49 / 50 (flip_signs / shrink_residual, the seeds of the
Q4_0 / Q8_0 cases they mirror), 5 (the overflow model), 53 (the refused-matrix models)."""
import contextlib

import numpy as np
import pytest

from crabml_amd import synth
from tests import fused_step_ref as R
from tests import prefill_pass_ref as P
from tests import q5_01_f16w_ref as Q
from tests import q5_01_step_ref as S
from tests import test_hip_f16w_gemm as G
from tests import test_prefill_pass_ref as TP
from tests.test_prefill_pass_ref import CHECK, MUTATIONS, PASS_TOKS, Case, oracle_pass

FMTS = Q.FMTS
N = len(PASS_TOKS)


@contextlib.contextmanager
def q5_pass():
    """q5_01_pass for the checker, and the oracle-pass builder's own weight_operands through the same dispatch"""
    saved = TP.weight_operands
    with Q.q5_01_pass():
        TP.weight_operands = G.weight_operands
        try:
            yield
        finally:
            TP.weight_operands = saved


def all_on(kernel):
    return lambda nm, t, l: kernel


def build(shape, fmt, seed=21, **kw):
    return synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=seed, **kw)


def accept(tap, kvb, kva, model, layer, form, ctx, twin=None):
    res = P.check_pass(tap, PASS_TOKS[:tap["plan"]["rows"]], kvb, kva, model, layer, form, ctx, None, twin)
    assert not P.failures(res), P.failures(res)
    for r in res.values():
        for name, share in r.excused.items():
            assert share <= R.EXCUSED_CAP, (ctx, r.launch, name, share)
    return res


# (model kind, f16 GEMM arm, h_done): the row-dot arm leaves g and u; the f16 arm stores h or, with the row quantizer, only planes
FORMS = [("plain", False, 0), ("plain", True, 1), ("shrunk", True, 2)]


@pytest.mark.parametrize("pos0", [0, 5])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128", "tiny-qwen2"])
def test_checker_accepts_the_oracle_pass_and_rejects_every_mutation(oracle, shape, fmt, pos0):
    models = {"plain": build(shape, fmt, n_layers=2), "shrunk": S.shrink_residual(build(shape, fmt, n_layers=2))}
    applied = set()
    with q5_pass():
        for kind, f16w, h_done in FORMS:
            model, small = models[kind], kind == "shrunk"
            for layer in (0, 1):
                kv_f16 = (pos0 + layer) % 2 == 0
                ctx = f"{shape} ({kind}) {fmt} {'f16' if f16w else 'row dots'} h_done={h_done} kv_f16={kv_f16} layer {layer} pos0 {pos0}"
                tap, kvb, kva, form, aux = oracle_pass(model, pos0, N, layer, kv_f16, f16w, h_done,
                                                       kernel_of=all_on(P.KERNEL_F16W if f16w else P.KERNEL_GEMV))
                want = P.KERNEL_F16W if f16w else P.KERNEL_GEMV
                assert all(tap["plan"][w] == want for w in P.KERNEL_WORD.values()), tap["plan"]
                base = Case(model, layer, tap, kvb, kva, form, aux, small)
                accept(tap, kvb, kva, model, layer, form, ctx, base.twin)
                for m in MUTATIONS:
                    c = base.fork()
                    launch = m(c)
                    if launch is None:
                        continue
                    applied.add(m.__name__)
                    got = CHECK[launch](c, ctx)
                    assert got.fails, f"{ctx}: the checker let {m.__name__} through at {launch} (worst error / bound {got.worst:.3g}, excused {got.excused})"
    skipped = {m.__name__ for m in MUTATIONS} - applied
    allowed = set()
    if synth.SHAPES[shape].arch != "qwen2":
        allowed |= {"m_qwen2_bias_missing_on_k"}
    if fmt != "Q5_1":
        allowed |= {"m_one_s_code"}
    if pos0 == 0:
        allowed |= {"m_rope_ignores_pos0", "m_k_rope_ignores_pos0"}
    assert skipped <= allowed, skipped


# ---- the six wrong loaders, on q, wo and ffn_down, on both arms ----
SITES = [("attn_q", "n1.act", "q", None, "q|k|v gemm"), ("attn_output", "attn.act", "wo.tmp", "wo.parts", "wo"),
         ("ffn_down", "hid.act", "down.tmp", "down.parts", "ffn_down")]


def wrong_output(c, nm, act_name, wrong):
    """the f32 output a kernel whose loader is wrong in the named way leaves for this matrix: the f16 arm's f32 sum of the WRONG A' times
    B', the row-dot arm's exact dot of the wrongly loaded rows rounded once"""
    wname = f"blk.{c.layer}.{nm}.weight"
    t = c.model.tensors[wname]
    m, k = t.shape
    acts = P.act_rows(c.tap, act_name)
    if P.kernel_of(c.tap, wname) == P.KERNEL_F16W:
        raw = np.ascontiguousarray(t.data).view(np.uint8).reshape(-1)
        ap = Q.weight_operands(raw, synth.TYPE_NAMES[t.typ], list(range(m)), k, wrong)[0].astype(np.float32)
        return P.b_prime(acts)[1].astype(np.float32) @ ap.T
    with S.q5_rows(wrong):
        return R.row_dots_many(t, acts, np.arange(m))[0].astype(np.float32)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128", "tiny-qwen2"])
def test_every_wrong_loader_lands_outside_the_bound_on_both_arms(oracle, shape, fmt):
    model = build(shape, fmt, n_layers=2)
    let_through = []
    with q5_pass():
        for f16w, h_done in ((True, 1), (False, 0)):
            for layer in (0, 1):
                ctx = f"{shape} {fmt} {'f16' if f16w else 'row dots'} layer {layer}"
                tap, kvb, kva, form, aux = oracle_pass(model, 0, N, layer, True, f16w, h_done, kernel_of=all_on(P.KERNEL_F16W if f16w else P.KERNEL_GEMV))
                base = Case(model, layer, tap, kvb, kva, form, aux, False)
                for wrong in S.WRONG:
                    for nm, act_name, out_name, parts_name, launch in SITES:
                        c = base.fork()
                        out = wrong_output(c, nm, act_name, wrong)
                        if parts_name in c.tap:  # (the pieces left to the norm launch stay; piece 0 carries the difference)
                            out = out - np.asarray(c.tap[parts_name], dtype=np.float32).reshape(-1, *out.shape).sum(axis=0)
                        assert not np.array_equal(out.reshape(-1), np.asarray(c.tap[out_name])), (ctx, wrong, nm)
                        c.tap[out_name] = np.ascontiguousarray(out, dtype=np.float32).reshape(-1)
                        got = CHECK[launch](c, ctx)
                        if not got.fails:
                            let_through.append((ctx, wrong, nm, round(got.worst, 3)))
    assert not let_through, let_through


# ---- a matrix the range check refuses inside a pass that otherwise takes the GEMM ----
REFUSED = ["attn_q", "attn_k", "attn_output", "ffn_up", "ffn_down"]
XH = {"n1.xh", "n1.xh.v", "attn.xh", "n2.xh", "hid.xh"}
# the B' fields a tapped layer 0 holds with that matrix refused (prefill_chunk_pass: a refused reader gets no B' from the kernel that
# quantizes its rows; behind a refused attn_q, attn_k's GEMM makes B' -- untapped -- and attn_v finds it, so n1.xh.v stays absent)
XH_WITH = {"attn_q": {"attn.xh", "n2.xh", "hid.xh"}, "attn_k": XH - {"n1.xh.v"}, "attn_output": {"n1.xh", "n2.xh", "hid.xh"},
           "ffn_up": XH - {"n1.xh.v"}, "ffn_down": {"n1.xh", "attn.xh", "n2.xh"}}


def refused_model(fmt, nm, shape="tiny-gqa"):
    """(the model whose layer-0 matrix nm the range check refuses, the kernel each matrix then takes)"""
    model = Q.refuse_matrix(build(shape, fmt, seed=53), f"blk.0.{nm}.weight")
    return model, (lambda name, t, l: P.KERNEL_GEMV if (l == 0 and name == nm) else P.KERNEL_F16W)


@pytest.mark.parametrize("nm", REFUSED)
@pytest.mark.parametrize("fmt", FMTS)
def test_mixed_kernel_taps_are_built_and_accepted(oracle, fmt, nm):
    model, kernel_of = refused_model(fmt, nm)
    h_done = 0 if nm == "ffn_up" else 1  # (gate | up fall apart: g and u are stored)
    with q5_pass():
        for layer in (0, 1):
            ctx = f"tiny-gqa {fmt} refused {nm} layer {layer}"
            tap, kvb, kva, form, aux = oracle_pass(model, 0, N, layer, True, True, h_done, kernel_of=kernel_of)
            plan = tap["plan"]
            accept(tap, kvb, kva, model, layer, form, ctx)
            took = {k: plan[w] for k, w in P.KERNEL_WORD.items()}
            if layer == 1:  # the control: the default plan
                assert set(took.values()) == {P.KERNEL_F16W} and plan["qkv_one"] == plan["gu_one"] == 1 and XH & set(tap) == XH - {"n1.xh.v"}, plan
                continue
            assert took == {k: (P.KERNEL_GEMV if k == nm else P.KERNEL_F16W) for k in P.KERNEL_WORD}, plan
            assert plan["qkv_one"] == (0 if nm in ("attn_q", "attn_k") else 1) and plan["gu_one"] == (0 if nm == "ffn_up" else 1), plan
            assert XH & set(tap) == XH_WITH[nm], (nm, XH & set(tap))


# ---- the caps are conditions on the reference: evaluated before any device value ----
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind", ["signs", "shrunk", "shrunk-row-dots"])
def test_interval_check_models_of_the_gpu_cases_stay_under_the_cap(oracle, kind, fmt):
    """the models tests/test_hip_prefill_q5_01_launches.py builds for its flipped-sign and shrunk-residual cases (tiny-gqa; seeds 49 and
    50, the first tried): oracle-made taps of layers 0 and 1 are accepted with every excused share of the Q8_0 / Q8_1 interval checks
    under EXCUSED_CAP"""
    model = S.flip_signs(build("tiny-gqa", fmt, seed=49)) if kind == "signs" else S.shrink_residual(build("tiny-gqa", fmt, seed=50))
    f16w = kind != "shrunk-row-dots"
    with q5_pass():
        for layer in (0, 1):
            ctx = f"{kind} tiny-gqa {fmt} layer {layer}"
            tap, kvb, kva, form, aux = oracle_pass(model, 0, N, layer, True, f16w, 1 if f16w else 0, kernel_of=all_on(P.KERNEL_F16W if f16w else P.KERNEL_GEMV))
            accept(tap, kvb, kva, model, layer, form, ctx)


# ---- the overflow case's model: h past 65504 (B' of ffn_down overflows f16), below 127 * 65504 (the rows' f16 scales stay finite) ----
OVERFLOW_LOG2 = {"Q5_0": 12, "Q5_1": 11}  # Q4_0's / Q8_0's factors (tests/test_hip_prefill_launches.py)


def overflow_model(fmt, log2=None):
    """the massive-channel model of test_overflow_recomputation_is_the_int8_pass: two elements of every ffn_norm weight x 2^log2"""
    model = build("tiny-gqa", fmt, seed=5)
    s = model.shape
    for l in range(s.n_layers):
        t = model.tensors[f"blk.{l}.ffn_norm.weight"]
        w = t.data.view(np.float32).copy()
        w[[3, s.dim // 2 + 1]] *= np.float32(2.0 ** (OVERFLOW_LOG2[fmt] if log2 is None else log2))
        t.data = w.view(np.uint8)
    return model


def overflow_tokens(model, n=64):
    return [(7 * i + 3) % model.shape.vocab for i in range(n)]  # (test_hip_prefill_launches.tokens_of)


def overflow_pass(fmt, log2=None):
    """the oracle's ops on the 64 tokens the GPU case runs, row by row (what the recomputation runs), layer 0 tapped"""
    model = overflow_model(fmt, log2)
    with q5_pass():
        return oracle_pass(model, 0, 64, 0, True, False, 0, kernel_of=all_on(P.KERNEL_GEMV), toks=overflow_tokens(model), seq=80)


def test_q5_0_overflow_model_puts_h_past_f16_and_below_the_rows_scale_range(oracle):
    """some layer's max |silu(g) * u| passes 65504 and none reaches 127 * 65504; the reference's own pass stays finite"""
    tap, _, _, _, aux = overflow_pass("Q5_0")
    top = aux["h_absmax"]
    print(f"overflow model Q5_0 x 2^{OVERFLOW_LOG2['Q5_0']}: max |h| per layer {[f'{v:.4g}' for v in top]}")
    assert len(top) == 2 and max(top) > 65504.0 and max(top) < 127 * 65504.0, top
    assert np.all(np.isfinite(tap["down.tmp"])) and np.all(np.isfinite(tap["logits"]))


@pytest.mark.parametrize("log2", [9, 10, 11])
def test_q5_1_rows_cannot_hold_an_h_that_overflows_f16(oracle, log2):
    """A finding about the case, from the reference alone.  Q5_1's rows are Q8_1 blocks, whose field s = d * sum q is an f16.  In the
    block that holds a massive element the other quants are near zero, so s is about that element: once h passes 65504 -- which is what
    makes ffn_down's B' overflow -- s is inf in the REFERENCE's own planes and its ffn_down output is not finite.  2^11 (Q8_0's factor)
    and 2^10 put max |h| at 2.824e+05 / 7.061e+04, inside (65504, 127 * 65504) as the overflow case asks, and the reference cannot finish
    the pass; 2^9 leaves it at 1.766e+04 and nothing overflows.  No factor gives a Q5_1 pass that is recomputed AND finite, on any path
    (the same holds for Q4_1, which tests/test_hip_prefill_launches.py's overflow case leaves out): the GPU file pins the plan of the
    recomputed Q5_1 pass and its launches in front of h, and says so"""
    tap, _, _, _, aux = overflow_pass("Q5_1", log2)
    top = max(aux["h_absmax"])
    s_field = np.stack([a["s"] for a in P.act_rows(tap, "hid.act")])
    print(f"overflow model Q5_1 x 2^{log2}: max |h| {top:.4g}, s finite {bool(np.all(np.isfinite(s_field)))}, ffn_down finite {bool(np.all(np.isfinite(tap['down.tmp'])))}")
    if log2 == 9:
        assert top < 65504.0 and np.all(np.isfinite(s_field)) and np.all(np.isfinite(tap["down.tmp"]))
    else:
        assert 65504.0 < top < 127 * 65504.0
        assert not np.all(np.isfinite(s_field)) and not np.all(np.isfinite(tap["down.tmp"]))
