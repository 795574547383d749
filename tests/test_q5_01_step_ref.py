"""The Q5_0 / Q5_1 checker (tests/q5_01_step_ref.py) checked on the CPU: its unpack against the reference's dequantizer bit for bit
(random blocks and tests/edge_blocks.py's: every qh bit set, none, levels at both ends), its bound against an f32 emulation of the
kernels' terms in permuted add orders, every subtly wrong loader it must reject, and -- from the reference alone, an oracle-built
tap of the step (tests/test_fused_step_ref.oracle_tap) -- that it accepts the reference's own order, rejects every mutation of
test_fused_step_ref.MUTATIONS that applies, and that the interval checks excuse no more than EXCUSED_CAP of any plane set for the
models, seeds and positions tests/test_hip_q5_01_fused.py runs (CASES below is that file's list: it imports it)."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import edge_blocks as eb
from tests import fused_step_ref as R
from tests import q5_01_step_ref as Q
from tests import test_fused_step_ref as T
from tests.helpers import EXACT_NORM, GEMV_REL
from tests.test_q5k_step_ref import oracle_tokens

SPLIT_ALWAYS = 16
# one layer whose ffn_down rows hold 130 blocks: three 64-unit steps, two live lanes in the last -- with two workgroups per chunk
# (SPLIT_CHUNKS_ALWAYS: one row per wave) the pipelined loop of rows_partial_deep and its clamped tail
SHAPE_FFN130 = synth.ModelShape("ffn130", 512, 4160, 1, 8, 2, 1024, 128, 1e-5, None)
FMT = {"Q5_0": synth.Q5_0, "Q5_1": synth.Q5_1}

# (key, shape, format, seed, build_model keywords, flags, seq, positions, layers, the plan's path)
CASES = []
for _shape in ("tiny-gqa", "tiny-hd128", "15m", "tiny-qwen2"):
    for _fmt in ("Q5_0", "Q5_1"):
        CASES.append((f"default/{_shape}/{_fmt}", _shape, _fmt, 81, {}, 0, 128, [0, 7, 100], [0, 1], 1))
    CASES.append((f"exact-norm/{_shape}/Q5_0", _shape, "Q5_0", 82, {}, EXACT_NORM, 128, [0, 7, 100], [0, 1], 1))
for _fmt in ("Q5_0", "Q5_1"):
    CASES.append((f"ffn130/{_fmt}", "ffn130", _fmt, 83, {}, SPLIT_ALWAYS, 128, [0, 7, 100], [0], 1))
    CASES.append((f"signs/tiny-gqa/{_fmt}", "tiny-gqa", _fmt, 84, {}, 0, 128, [0, 7, 100], [0, 1], 1))
CASES.append(("shrunk/tiny-gqa/Q5_0", "tiny-gqa", "Q5_0", 85, {}, 0, 128, [0, 7, 100], [0, 1], 1))
CASES.append(("q6k-classifier/tiny-gqa/Q5_0", "tiny-gqa", "Q5_0", 86, {"output_type": synth.Q6_K}, 0, 128, [0, 7, 100], [0, 1], 1))
CASES.append(("q6k-classifier/tiny-gqa/Q5_1", "tiny-gqa", "Q5_1", 86, {"output_type": synth.Q6_K}, 0, 128, [0, 7, 100], [0, 1], 2))


def shape_of(name):
    return SHAPE_FFN130 if name == "ffn130" else synth.SHAPES[name]


def build(case):
    key, shape, fmt, seed, kw = case[:5]
    model = synth.build_model(shape_of(shape), FMT[fmt], seed=seed, **kw)
    if key.startswith("signs/"):
        Q.flip_signs(model)
    if key.startswith("shrunk/"):
        Q.shrink_residual(model)
    return model


def tensor(rng, typ, rows, k):
    return synth.RawTensor(synth.random_blocks(rng, rows * k, typ), [rows, k], typ)


def rhs(rng, typ, k):
    qt = o.rhs_dtype(typ)
    return R.parse_act(o.quantize((rng.standard_normal(k) * rng.uniform(0.2, 3.0)).astype(np.float32), qt), qt)


def restated_f32(t):
    """the dequantized elements as the restatement gives them, in the reference's own f32 steps: (level - 16) as f32 times d
    (buf_q5_0.rs:22-37), level as f32 times d plus m (buf_q5_1.rs:20-36)"""
    w = Q.weight_rows(t, 0, t.shape[0])
    f = np.float32
    if t.typ == synth.Q5_0:
        return (w["q"].astype(f) * w["d"].astype(f)[:, :, None]).reshape(-1)
    return ((w["q"].astype(f) * w["d"].astype(f)[:, :, None]).astype(f) + w["m"].astype(f)[:, :, None]).reshape(-1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
def test_restated_rows_equal_the_reference_dequantizer(oracle, fmt):
    """random blocks, and edge_blocks' "saturated" kind: per block the nibbles all 15 or all 0 times the qh bits all set or all clear
    -- levels 0, 15, 16 and 31, i.e. -16 .. 15 for Q5_0 --, plus a block of alternating qh bits planted here; "sign" and "mixed" too"""
    typ = FMT[fmt]
    rng = np.random.default_rng(4)
    t = tensor(rng, typ, 8, 512)
    assert same_bits(restated_f32(t), o.dequantize(t.data, typ))
    w = Q.weight_rows(t, 0, 8)
    assert w["q"].max() == (15 if fmt == "Q5_0" else 31) and w["q"].min() == (-16 if fmt == "Q5_0" else 0)
    assert np.any(Q.levels(w["qs"], w["qh"]) != Q.levels(w["qs"], w["qh"], "qh_bits_dropped"))
    for kind in ("saturated", "sign", "mixed"):
        raw = eb.edge_blocks(rng, fmt, 8, 512, kind)
        if kind == "saturated":  # alternating fifth bits, both phases
            blk = raw.reshape(-1, synth.BLOCK_BYTES[typ])
            h = 2 if fmt == "Q5_0" else 4
            blk[0, h:h + 4] = 0x55
            blk[1, h:h + 4] = 0xAA
        te = synth.RawTensor(raw, [8, 512], typ)
        assert same_bits(restated_f32(te), o.dequantize(te.data, typ)), kind
        if kind == "saturated":
            lv = Q.levels(Q.weight_rows(te, 0, 8)["qs"], Q.weight_rows(te, 0, 8)["qh"])
            assert {0, 15, 16, 31} <= set(np.unique(lv).tolist())


@pytest.mark.parametrize("k", [288, 512, 4160, 14336])
@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
def test_bound_holds_an_f32_emulation_in_permuted_orders(oracle, fmt, k):
    """the kernels' terms evaluated in f32 from integers formed HERE in int64 -- Q5_0: ((float)sumi * d_w) * d_x; Q5_1: (float)sumi *
    f16(d_w d_x) + f16(m s) -- and the nb terms added in f32 in ascending, reversed and random orders: inside the bound on every row;
    the reference's own scalar vec_dot too; and the bound is never above the project's 8 GEMV_REL sum |w x|"""
    typ = FMT[fmt]
    rng = np.random.default_rng(k)
    rows = 48
    t = tensor(rng, typ, rows, k)
    act = rhs(rng, typ, k)
    exact, bound = Q.row_dots(t, act)
    w = Q.weight_rows(t, 0, rows)
    f = np.float32
    lv = Q.levels(w["qs"], w["qh"])
    sumi = np.einsum("rbi,bi->rb", lv - (16 if fmt == "Q5_0" else 0), act["q"].astype(np.int64))
    assert np.abs(sumi).max() < 2 ** 24
    if fmt == "Q5_0":
        terms = ((sumi.astype(f) * w["d"].astype(f)).astype(f) * act["d"].astype(f)[None]).astype(f)
    else:
        P = (w["d"] * act["d"][None]).astype(np.float16).astype(f)
        M = (w["m"] * act["s"][None]).astype(np.float16).astype(f)
        terms = ((sumi.astype(f) * P).astype(f) + M).astype(f)
    n = terms.shape[1]
    for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n), rng.permutation(n)):
        acc = np.zeros(rows, dtype=f)
        for j in order:
            acc = (acc + terms[:, j]).astype(f)
        assert np.all(np.abs(acc.astype(np.float64) - exact) <= bound), (k, float(np.max(np.abs(acc - exact) / bound)))
    planes = o.quantize(np.zeros(k, np.float32), o.rhs_dtype(typ))  # (the reference's vec_dot on the same activation blocks)
    ref = T.mv(t, _blocks_of(act, planes))
    assert np.all(np.abs(ref.astype(np.float64) - exact) <= bound)
    deq = eb.dequant_f64(t.data, fmt).reshape(rows, k)
    proj = GEMV_REL * (np.abs(deq) @ np.abs(R.act_values(act)))
    assert np.all(bound <= 8 * proj * (1 + 1e-12)), (k, float(np.max(bound / proj)))


def _blocks_of(act, like):
    """the raw activation blocks `act` was parsed from (test helper: rebuilt from its fields)"""
    qt = act["qt"]
    bb = 34 if qt == o.Q8_0 else 36
    b = np.zeros((act["q"].shape[0], bb), np.uint8)
    b[:, 0:2] = act["d_bits"].astype(np.uint16).reshape(-1, 1).view(np.uint8)
    if qt == o.Q8_1:
        b[:, 2:4] = act["s_bits"].astype(np.uint16).reshape(-1, 1).view(np.uint8)
    b[:, bb - 32:] = act["q"].astype(np.int8).view(np.uint8)
    return b.reshape(-1).view(like.dtype)


@pytest.mark.parametrize("wrong", list(Q.WRONG) + ["last_block_dropped"])
@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
def test_every_wrong_loader_is_rejected(oracle, fmt, wrong):
    typ = FMT[fmt]
    rng = np.random.default_rng(11)
    for k in (288, 4160):
        t = tensor(rng, typ, 64, k)
        act = rhs(rng, typ, k)
        exact, bound = Q.row_dots(t, act)
        if wrong == "last_block_dropped":
            got, _ = Q.row_dots(t, act, drop_last_block=True)
        else:
            got, _ = Q.row_dots(t, act, wrong=wrong)
        out = np.abs(got.astype(np.float32).astype(np.float64) - exact) > bound
        assert out.mean() > 0.9, (fmt, wrong, k, float(out.mean()))


def _tap(model, pos, layer, hop_free, path=1):
    if path == 2:  # a Q5_1 body in front of a classifier of another format: the stand-alone norm and quantizer launches
        return T.oracle_tap_k(model, pos, layer, True, "separate-norm")
    cls = model.tensors.get("output.weight")
    if cls is not None and cls.typ != model.wtype:
        # oracle_tap hands the classifier the layers' planes.  What is evaluated from such a model here are the layers' launches and
        # their excused shares, which do not read the classifier: a stand-in of the body's format (the embedding's bytes)
        import copy
        model = copy.copy(model)
        model.tensors = dict(model.tensors, **{"output.weight": model.tensors["token_embd.weight"]})
    return T.oracle_tap(model, pos, layer, True, hop_free)


@pytest.mark.parametrize("pos", [0, 7])
@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
@pytest.mark.parametrize("shape", ["15m", "tiny-gqa", "tiny-hd128", "tiny-qwen2"])
def test_checker_accepts_the_oracle_step_and_rejects_every_mutation(oracle, shape, fmt, pos):
    """tests/test_fused_step_ref.py's own test with the two formats: Q5_0 in the exact-norm and the hop-free form (and on the shrunk
    residual stream, where a wrong eps cannot pass), Q5_1 in the exact-norm form; layers 0 and 1"""
    typ = FMT[fmt]
    plain = synth.build_model(synth.SHAPES[shape], typ, seed=21, n_layers=2)
    shrunk = Q.shrink_residual(synth.build_model(synth.SHAPES[shape], typ, seed=21, n_layers=2))
    applied = set()
    forms = [(plain, False, False)] + ([(plain, True, False), (shrunk, True, True)] if fmt == "Q5_0" else [])
    with Q.q5_rows():
        for model, hop_free, small in forms:
            for layer in (0, 1):
                kv_f16 = (pos + layer) % 2 == 0
                ctx = f"{shape}{' (shrunk residual)' if small else ''} {fmt} {'hop-free' if hop_free else 'exact-norm'} kv_f16={kv_f16} layer {layer} pos {pos}"
                tap, kc, vc, form, aux = T.oracle_tap(model, pos, layer, kv_f16, hop_free)
                res = R.check_layer(tap, kc, vc, model, layer, pos, form, ctx)
                assert not R.failures(res), R.failures(res)
                for r in res.values():
                    for name, share in r.excused.items():
                        assert share <= R.EXCUSED_CAP, (ctx, r.launch, name, share)
                base = T.Case(model, layer, pos, tap, kc, vc, form, aux, small)
                for m in T.MUTATIONS:
                    c = base.fork()
                    launch = m(c)
                    if launch is None:
                        continue
                    applied.add(m.__name__)
                    got = T.CHECK[launch](c, ctx)
                    assert got.fails, f"{ctx}: the checker let {m.__name__} through at {launch} (worst error / bound {got.worst:.3g}, excused {got.excused})"
    skipped = {m.__name__ for m in T.MUTATIONS} - applied
    allowed = set()
    if synth.SHAPES[shape].arch != "qwen2":
        allowed |= {"m_rope_adjacent_pairs", "m_bias_before_multiply"}
    if synth.SHAPES[shape].n_kv_heads == synth.SHAPES[shape].n_heads:
        allowed |= {"m_wrong_kv_head"}
    if fmt == "Q5_0":
        allowed |= {"m_hid_s_code"}
    else:
        allowed |= {"m_inv_rms_gateup_1e4", "m_inv_rms_qkv_1e4", "m_eps_gateup", "m_eps_qkv", "m_bias_before_multiply", "m_rsums_chunk"}
    if pos == 0:
        allowed |= {"m_rope_adjacent_pairs"}
    assert skipped <= allowed, skipped


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
def test_wrong_rows_fail_in_the_launch_that_owns_them(oracle, fmt):
    """through check_layer: wo's x built from each wrong loader's dots fails at `wo`"""
    model = Q.flip_signs(synth.build_model(synth.SHAPES["tiny-gqa"], FMT[fmt], seed=22, n_layers=2))
    tap, kc, vc, form, _ = T.oracle_tap(model, 7, 1, True, fmt == "Q5_0")
    assert not Q.failures(Q.check_layer(tap, kc, vc, model, 1, 7, form, "oracle"))
    act = R.parse_act(tap["attn.act_attn"], tap["qtype"]["attn.act_attn"])
    for wrong in list(Q.WRONG) + [True]:
        dots = Q.row_dots(model.tensors["blk.1.attn_output.weight"], act, drop_last_block=wrong is True, wrong=None if wrong is True else wrong)[0]
        bad = dict(tap)
        bad["wo.x"] = (np.asarray(tap["qkv_in.x"], dtype=np.float64) + dots).astype(np.float32)
        got = Q.check_layer(bad, kc, vc, model, 1, 7, form, "mutant")["wo"]
        assert any("x row" in f for f in got.fails), (wrong, got.fails, got.worst)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_oracle_step_passes_and_excused_shares_stay_under_the_cap(oracle, case):
    """the reference's own step passes the checker on every model the GPU file runs, and the excused share of every interval check
    -- a property of the reference's values alone -- is at most EXCUSED_CAP, at every position and layer that file taps"""
    key, _, fmt, _, _, flags, seq, positions, layers, path = case
    model = build(case)
    hop_free = fmt == "Q5_0" and not (flags & EXACT_NORM)
    shares = []
    with oracle_tokens(seq, max(positions) + 1):
        for pos in positions:
            for layer in layers:
                tap, kc, vc, form, _ = _tap(model, pos, layer, hop_free, path)
                ctx = f"{key} layer {layer} pos {pos}"
                cls_stand_in = path == 1 and "output.weight" in model.tensors and model.tensors["output.weight"].typ != model.wtype
                if cls_stand_in:
                    tap = {k: v for k, v in tap.items() if k != "logits"}
                with Q.q5_rows():
                    res = {k: v for k, v in _check(tap, kc, vc, model, layer, pos, form, ctx, cls_stand_in).items()}
                assert not Q.failures(res), Q.failures(res)
                for r in res.values():
                    for name, share in r.excused.items():
                        shares.append(share)
                        assert share <= Q.EXCUSED_CAP, (ctx, r.launch, name, share)
    assert shares or path == 2  # (the stand-alone quantizer launches of path 2 are held byte for byte: nothing to excuse)
    if shares:
        print(f"{key}: excused shares: max {max(shares):.3f}, mean {np.mean(shares):.3f} over {len(shares)} plane sets")


def _check(tap, kc, vc, model, layer, pos, form, ctx, without_classifier):
    if not without_classifier:
        return R.check_layer(tap, kc, vc, model, layer, pos, form, ctx)
    out = {}
    if layer == 0:
        out["norm+quantize"] = R.check_planes_in_front(tap, model, layer, form, ctx)
    out["q|k|v"] = R.check_qkv(tap, kc, vc, model, layer, pos, form, ctx)
    out["attention"] = R.check_attention(tap, kc, vc, model, layer, pos, form, ctx)
    out["wo"] = R.check_gemv_out(tap, model, layer, "wo", form, ctx)
    out["gate|up"] = R.check_gateup(tap, model, layer, form, ctx)
    out["ffn_down"] = R.check_gemv_out(tap, model, layer, "down", form, ctx)
    return out
