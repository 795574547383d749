"""tests/edge_blocks.py on the CPU: the float64 restatement IS the reference's dequantization, and the generator reaches the field
values it promises (the GPU comparisons of test_hip_weight_edges.py are only as sharp as these inputs)."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import edge_blocks as eb
from tests.test_hip_kquant_ints import scale_min_k4

M, K = 16, 1024  # 64 super-blocks: a quarter of them (the "mixed" kind's share per kind) still covers the 16 combinations of Q5_K
ALL_KINDS = ["random"] + eb.KINDS


def blocks(fmt, kind, seed=0):
    rng = np.random.default_rng([seed, eb.FORMATS.index(fmt), ALL_KINDS.index(kind)])
    if kind == "random":
        return synth.random_blocks(rng, M * K, synth.TYPE_BY_NAME[fmt])
    return eb.edge_blocks(rng, fmt, M, K, kind)


@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("fmt", eb.FORMATS)
def test_float64_restatement_is_the_reference_dequantization(fmt, kind):
    """dequant_f64 rounded ONCE to f32 equals o.dequantize bit for bit (signs of zero included), and its float64 dot with the
    dequantized quantized row is o.vec_dot of the same blocks within the reference's own roundings: f32 accumulation (1e-5 of
    sum |w||x|, as test_restated_operands_are_the_reference_dot allows) plus, for Q4_1 / Q5_1, its f16 products."""
    typ = synth.TYPE_BY_NAME[fmt]
    raw = blocks(fmt, kind)
    w = eb.dequant_f64(raw, fmt)
    assert np.all(np.isfinite(w)), "no dequantized element may leave f32"
    with np.errstate(over="raise"):
        w32 = w.astype(np.float32)
    ref = eb.reference_dequantize(raw, fmt)
    assert np.all(np.isfinite(ref))
    assert np.array_equal(w32.view(np.uint32), ref.view(np.uint32)), (fmt, kind, np.flatnonzero(w32.view(np.uint32) != ref.view(np.uint32))[:4])
    rng = np.random.default_rng(7)
    x = eb.edge_rows(rng, K, "normal")
    qt = o.rhs_dtype(typ)
    xq = o.quantize(x, qt)
    x64 = eb.dequant_rows_f64(xq, qt)
    rb = K // o.BLOCK_ELEMS[typ] * o.BLOCK_BYTES[typ]
    slack = eb.f16_product_slack(raw, fmt, xq, M, K)
    w = w.reshape(M, K)
    for r in range(M):
        got = o.vec_dot(raw[r * rb:(r + 1) * rb], typ, xq, K)
        assert np.isfinite(got)
        tol = 1e-5 * float(np.abs(w[r]) @ np.abs(x64)) + slack[r] + 1e-30
        assert abs(float(w[r] @ x64) - got) <= tol, (fmt, kind, r, float(w[r] @ x64), got, tol)


def _signs(v):
    return bool(np.any(np.signbit(v))), bool(np.any(~np.signbit(v)))


@pytest.mark.parametrize("fmt", eb.FORMATS)
def test_sign_and_range_kinds_carry_both_signs_of_every_scale(fmt):
    for kind in ("sign", "range", "mixed"):
        f = eb.scale_fields(blocks(fmt, kind), fmt)
        for name, v in f.items():
            assert _signs(v) == (True, True), (fmt, kind, name)
    f = eb.scale_fields(blocks(fmt, "sign"), fmt)
    if fmt != "Q8_K":  # d = +0 and d = -0
        z = f["d"][f["d"] == 0]
        assert _signs(z) == (True, True), fmt
    # "sign" leaves the magnitudes of the blocks it does not zero as random_blocks drew them: the same generator state, so the same
    # base blocks, is what edge_blocks starts from
    rng = np.random.default_rng(3)
    a = synth.random_blocks(np.random.default_rng(3), M * K, synth.TYPE_BY_NAME[fmt])
    b = eb.edge_blocks(rng, fmt, M, K, "sign")
    fa, fb = eb.scale_fields(a, fmt), eb.scale_fields(b, fmt)
    for name in fa:
        keep = fb[name] != 0
        assert np.array_equal(np.abs(fa[name][keep]), np.abs(fb[name][keep])), (fmt, name)
    assert np.array_equal(np.abs(eb.dequant_f64(eb.negate_scales(b, fmt), fmt)), np.abs(eb.dequant_f64(b, fmt)))
    assert np.array_equal(eb.dequant_f64(eb.negate_scales(b, fmt), fmt), -eb.dequant_f64(b, fmt)), "negate_scales is -W exactly"
    # "range": every magnitude of the set, with both signs
    f = eb.scale_fields(blocks(fmt, "range"), fmt)
    for i, (name, v) in enumerate(f.items()):
        for mag in eb.range_magnitudes(fmt, i).astype(np.float64):
            assert np.any(v == mag) and np.any(v == -mag), (fmt, name, mag)


def _k4_all(raw_scales):
    sc, mn = zip(*(scale_min_k4(s) for s in raw_scales))
    return np.array(sc), np.array(mn)


def _ends(v, lo, hi, what):
    """some block has the field at `lo` everywhere and some block at `hi` everywhere; no block in between"""
    v = np.asarray(v).reshape(len(v), -1)
    all_lo, all_hi = np.all(v == lo, axis=1), np.all(v == hi, axis=1)
    assert all_lo.any() and all_hi.any(), what
    return all_lo, all_hi


@pytest.mark.parametrize("fmt", eb.FORMATS)
def test_saturated_kind_reaches_every_named_extreme(fmt):
    typ = synth.TYPE_BY_NAME[fmt]
    for kind in ("saturated", "mixed"):
        blk = blocks(fmt, kind).reshape(-1, o.BLOCK_BYTES[typ])
        if fmt in ("Q4_0", "Q4_1"):
            qs = blk[:, (2 if fmt == "Q4_0" else 4):]
            _ends(qs, 0x00, 0xFF, (fmt, kind, "nibbles 0 / 15"))
        elif fmt == "Q8_0":
            _ends(blk[:, 2:].view(np.int8), -128, 127, (fmt, kind))
        elif fmt in ("Q5_0", "Q5_1"):
            h = 2 if fmt == "Q5_0" else 4
            lev = eb._q5_levels(blk[:, h:h + 4], blk[:, h + 4:])
            for lo, hi in ((0, 31), (15, 16)):  # all four nibble x high-bit combinations: levels 0, 15, 16, 31
                _ends(lev, lo, hi, (fmt, kind, lo, hi))
        elif fmt == "Q8_K":
            q = blk[:, 4:260].view(np.int8)
            lo, hi = _ends(q, -128, 127, (fmt, kind))
            bs = blk[:, 260:].copy().view(np.int16)
            assert np.all(bs[lo] == -2048) and np.all(bs[hi] == 2032)
        elif fmt == "Q2_K":
            q_lo, q_hi = _ends(blk[:, 16:80], 0x00, 0xFF, (fmt, kind, "quants"))
            s_lo, s_hi = _ends(blk[:, 0:16] & 15, 0, 15, (fmt, kind, "scales"))
            m_lo, m_hi = _ends(blk[:, 0:16] >> 4, 0, 15, (fmt, kind, "mins"))
            assert (q_hi & s_hi & m_hi).any() and (q_hi & s_hi & m_lo).any() and (q_lo & s_hi & m_hi).any()
        elif fmt == "Q3_K":
            _ends(blk[:, 32:96], 0x00, 0xFF, (fmt, kind, "low bits"))
            _ends(blk[:, 0:32], 0x00, 0xFF, (fmt, kind, "hmask"))
            s_lo, s_hi = _ends(eb._q3k_scales(blk[:, 96:108]), 0, 63, (fmt, kind, "scales"))
            lev = eb.dequant_f64(blk.reshape(-1), fmt).reshape(len(blk), 256)
            d = eb.scale_fields(blk.reshape(-1), fmt)["d"][:, None]
            assert np.any(lev[s_lo] == -32 * -4 * d[s_lo]) and np.any(lev[s_hi] == 31 * 3 * d[s_hi])  # (-32)(-4) and (+31)(+3)
        elif fmt in ("Q4_K", "Q5_K"):
            sc, mn = _k4_all(blk[:, 4:16] if fmt == "Q4_K" else blk[:, 160:172])
            q_lo, q_hi = _ends(blk[:, 16:] if fmt == "Q4_K" else blk[:, 0:128], 0x00, 0xFF, (fmt, kind, "nibbles"))
            s_lo, s_hi = _ends(sc, 0, 63, (fmt, kind, "scales"))
            m_lo, m_hi = _ends(mn, 0, 63, (fmt, kind, "mins"))
            assert (q_hi & s_hi & m_hi).any() and (q_hi & s_hi & m_lo).any() and (q_lo & s_lo & m_hi).any()
            if fmt == "Q5_K":
                h_lo, h_hi = _ends(blk[:, 128:160], 0x00, 0xFF, (fmt, kind, "high bits"))
                assert (q_hi & h_hi & s_hi).any() and (q_lo & h_lo).any()
        elif fmt == "Q6_K":
            q_lo, q_hi = _ends(blk[:, 0:192], 0x00, 0xFF, (fmt, kind, "quants 0 / 63"))
            sc = blk[:, 192:208].view(np.int8)
            s_lo, s_hi = _ends(sc, -128, 127, (fmt, kind, "scales"))
            both = np.any(sc == -128, axis=1) & np.any(sc == 127, axis=1) & np.all((sc == -128) | (sc == 127), axis=1)
            assert both.any(), (fmt, kind, "mixed scales")
            assert (q_lo & s_lo).any() and (q_hi & s_hi).any() and (q_lo & s_hi).any() and (q_hi & s_lo).any()


def test_edge_rows_quantize_to_the_ends_of_the_q8_k_fields():
    rng = np.random.default_rng(11)
    for kind in eb.ROW_KINDS:
        x = eb.edge_rows(rng, K, kind)
        assert x.dtype == np.float32 and x.shape == (K,) and np.all(np.abs(x) <= eb.X_MAX)
        assert eb.edge_rows(rng, 288, kind).shape == (288,)  # a ragged tail for the 32-element formats
        blk = o.quantize(x, o.Q8_K).reshape(-1, 292)
        q = blk[:, 4:260].view(np.int8)
        bs = blk[:, 260:].copy().view(np.int16)
        assert np.array_equal(bs, q.reshape(-1, 16, 16).astype(np.int64).sum(axis=2))
        if kind == "constant":
            assert np.all((q == -128) | (q == 127))
            assert np.any(bs == -2048) and np.any(bs == 2032)
            assert np.any(np.all(bs == -2048, axis=1)), "a super-block with every 16-sum at the bottom"
            assert np.any(np.sum(bs == 2032, axis=1) == 15), "a super-block with 15 of its 16 sums at the top"
            assert _signs(blk[:, 0:4].copy().view(np.float32)) == (True, True), "both signs of the row scale d"
        elif kind == "one_hot_neg":
            assert np.all(np.sum(q == -128, axis=1) == 1) and np.all(np.sum(q == 127, axis=1) == 255)
        elif kind == "alternating":
            assert np.all(np.abs(q.astype(np.int64)) >= 127) and np.all(np.sum(q == -128, axis=1) == 1)
            assert np.all(bs[:, 1:] == 0) and np.all(bs[:, 0] == -1)
        # the 32-element quantizers: |q| at 127 in every block of the three edge kinds
        if kind != "normal":
            q0 = o.quantize(x, o.Q8_0).reshape(-1, 34)[:, 2:].view(np.int8)
            assert np.all(np.max(np.abs(q0.astype(np.int64)), axis=1) == 127)


@pytest.mark.parametrize("fmt", ["Q4_K", "Q5_K", "Q2_K"])
def test_saturated_blocks_on_constant_rows_leave_the_references_i16(fmt):
    """the reference multiplies bsums by the mins in i16 (buf_q4_k.rs:240); the backend's arithmetic is the oracle's with
    i16_wrap = 0.  On these inputs the two differ -- the counter of products that leave i16 is not zero -- so the GPU comparisons of
    test_hip_weight_edges.py run the i32 arithmetic where it matters."""
    typ = synth.TYPE_BY_NAME[fmt]
    raw = blocks(fmt, "saturated")
    x = eb.edge_rows(np.random.default_rng(5), K, "constant")
    xq = o.quantize(x, o.Q8_K)
    rb = K // 256 * o.BLOCK_BYTES[typ]
    count = {"Q4_K": o.q4k_overflow_count, "Q5_K": o.q5k_overflow_count, "Q2_K": o.q2k_overflow_count}[fmt]
    n = sum(count(raw[r * rb:(r + 1) * rb], xq, K) for r in range(M))
    assert n > 0, fmt
    if fmt != "Q2_K":  # and the wrapped arithmetic gives another number there
        fn = o.lib().co_vec_dot_q4_k_q8_k if fmt == "Q4_K" else o.lib().co_vec_dot_q5_k_q8_k
        rows = [np.ascontiguousarray(raw[r * rb:(r + 1) * rb]) for r in range(M)]
        a, b = ([fn(o._p(row), o._p(xq), K // 256, wrap, None) for row in rows] for wrap in (0, 1))
        assert a != b, fmt


def test_flip_scale_signs_touches_every_quantized_tensor_and_nothing_else():
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_K, seed=8, n_layers=1, k_m_mix=True)
    before = {n: t.data.copy() for n, t in model.tensors.items()}
    flipped = eb.flip_scale_signs(model, np.random.default_rng(2))
    for name, t in model.tensors.items():
        assert np.array_equal(t.data, before[name]), "the source model is not written"
        f = flipped.tensors[name]
        assert f.typ == t.typ and f.shape == t.shape
        fmt = synth.TYPE_NAMES[t.typ]
        if fmt not in eb.FORMATS:
            assert np.array_equal(f.data, t.data)
            continue
        a, b = eb.scale_fields(t.data, fmt), eb.scale_fields(f.data, fmt)
        for key in a:
            assert _signs(b[key]) == (True, True), (name, key)
            keep = b[key] != 0
            assert np.array_equal(np.abs(a[key][keep]), np.abs(b[key][keep]))


# ---- the mixed-sign models behind the launch pins: the checkers' excused-share caps are CONDITIONS on the reference's own values, so
# they are evaluated here, from oracle-made taps of the very models the GPU cases build (edge_blocks.mixed_sign_model), before any GPU
# run.  (The Q5_K / Q6_K bodies: the `mixed-signs` rows of tests/test_q5k_step_ref.py / test_q6k_step_ref.py.  No Gemma shape is
# among the mixed-sign cases: the oracle tap restates the Llama / Qwen2 step only.)
def _under_the_cap(res, cap, ctx, failures):
    assert not failures(res), failures(res)
    for r in res.values():
        for name, share in r.excused.items():
            assert share <= cap, (ctx, r.launch, name, share)


@pytest.mark.parametrize("shape,fmt", [("tiny-gqa", "Q4_0"), ("tiny-gqa", "Q8_0"), ("tiny-gqa", "Q4_1"), ("tiny-hd128", "Q4_1")])
def test_mixed_sign_models_stay_under_the_decode_and_prompt_caps(oracle, shape, fmt):
    from tests import fused_step_ref as R
    from tests import prefill_pass_ref as P
    from tests import test_fused_step_ref as TF
    from tests import test_prefill_pass_ref as TP
    model = eb.mixed_sign_model(shape, synth.TYPE_BY_NAME[fmt], eb.MIXED_SIGN_SEEDS["fused"])
    for pos in (0, 5):
        for layer in (0, 1):
            ctx = f"mixed-signs {shape} {fmt} layer {layer} pos {pos}"
            tap, kc, vc, form, aux = TF.oracle_tap(model, pos, layer, True, fmt != "Q4_1")  # (the default step: hop-free but for Q4_1)
            _under_the_cap(R.check_layer(tap, kc, vc, model, layer, pos, form, ctx), R.EXCUSED_CAP, ctx, R.failures)
    model = eb.mixed_sign_model(shape, synth.TYPE_BY_NAME[fmt], eb.MIXED_SIGN_SEEDS["prefill"])
    n = len(TP.PASS_TOKS)
    for layer in (0, 1):
        ctx = f"mixed-signs {shape} {fmt} f16 pass layer {layer}"
        tap, kvb, kva, form, aux = TP.oracle_pass(model, 0, n, layer, True, True, 1)
        twin = TP.Case(model, layer, tap, kvb, kva, form, aux, False).twin
        _under_the_cap(P.check_pass(tap, TP.PASS_TOKS[:n], kvb, kva, model, layer, form, ctx, None, twin), R.EXCUSED_CAP, ctx, P.failures)


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128"])
def test_mixed_sign_q5_01_models_stay_under_the_prompt_cap(oracle, shape, fmt):
    """the Q5_0 / Q5_1 models of tests/test_hip_prefill_q5_01_launches.test_mixed_sign_block_fields (the same builder, the same seed: the
    first tried), read by the prompt-pass checker inside q5_01_pass: every launch of the f16 pass accepted, every excused share of the
    Q8_0 / Q8_1 interval checks under the cap, from the reference alone"""
    from tests import fused_step_ref as R
    from tests import prefill_pass_ref as P
    from tests import test_prefill_pass_ref as TP
    from tests.test_q5_01_pass_ref import all_on, q5_pass
    model = eb.mixed_sign_model(shape, synth.TYPE_BY_NAME[fmt], eb.MIXED_SIGN_SEEDS["prefill"])
    n = len(TP.PASS_TOKS)
    with q5_pass():
        for layer in (0, 1):
            ctx = f"mixed-signs {shape} {fmt} f16 pass layer {layer}"
            tap, kvb, kva, form, aux = TP.oracle_pass(model, 0, n, layer, True, True, 1, kernel_of=all_on(P.KERNEL_F16W))
            _under_the_cap(P.check_pass(tap, TP.PASS_TOKS[:n], kvb, kva, model, layer, form, ctx, None, None), R.EXCUSED_CAP, ctx, P.failures)


@pytest.mark.parametrize("shape,mix", [("tiny-gqa", False), ("tiny-gqa", True), ("tiny-hd128", False)])
def test_mixed_sign_k_quant_models_stay_under_the_decode_and_prompt_caps(oracle, shape, mix):
    from tests import fused_step_ref as R
    from tests import prefill_pass_ref as P
    from tests import test_fused_step_ref as TF
    from tests import test_prefill_pass_ref as TP
    kw = {"k_m_mix": True} if mix else {"output_type": synth.Q6_K}
    model = eb.mixed_sign_model(shape, synth.Q4_K, eb.MIXED_SIGN_SEEDS["fused_k"], **kw)
    for pos in (0, 5):
        for layer in (0, 1):
            ctx = f"mixed-signs {shape} {'Q4_K_M' if mix else 'Q4_K'} layer {layer} pos {pos}"
            tap, kc, vc, form, aux = TF.oracle_tap_k(model, pos, layer, True, "default")
            _under_the_cap(R.check_layer(tap, kc, vc, model, layer, pos, form, ctx, twin=aux["twin"]), R.EXCUSED_CAP, ctx, R.failures)
    if shape != "tiny-gqa":
        return  # (the prompt-pass pins take the tiny-gqa models only)
    model = eb.mixed_sign_model(shape, synth.Q4_K, eb.MIXED_SIGN_SEEDS["prefill_k"], k_m_mix=mix)
    n = len(TP.PASS_TOKS)
    for layer in (0, 1):
        ctx = f"mixed-signs {shape} {'Q4_K_M' if mix else 'Q4_K'} f16 pass layer {layer}"
        tap, kvb, kva, form, aux = TP.oracle_pass(model, 0, n, layer, True, True, 0, True)
        res = P.check_pass(tap, TP.PASS_TOKS[:n], kvb, kva, model, layer, form, ctx, None, None)
        assert not P.failures(res), P.failures(res)
        assert not any(r.excused for r in res.values()), {k: r.excused for k, r in res.items()}  # (Q8_K-row passes excuse nothing)
