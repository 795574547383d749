"""The Q3_K checker (tests/q3k_step_ref.py) checked on the CPU: its unpack of the raw 110-byte block against the reference's dequantizer,
its bound against an f32 emulation of the kernel's term in permuted add orders, every subtly wrong kernel it must reject, and -- from
the reference alone, an oracle-built tap of the step -- that it accepts the reference's own order and that the Q8_K interval check
excuses no more than EXCUSED_CAP of any plane set for the shapes, seeds and positions tests/test_hip_q3k_fused.py uses (CASES below
is that file's list: it imports it)."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests import q3k_step_ref as Q
from tests.test_q5k_step_ref import _tap, oracle_tokens, q8k, shape_of

Q3K, Q4K, Q5K, Q6K = synth.Q3_K, synth.Q4_K, synth.Q5_K, synth.Q6_K
# three layers that hold every hand-over of the family: V / wo / ffn_down in Q5_K / Q4_K / Q5_K, all three in Q4_K, all three in Q3_K
MIX_LAYERS = {0: {"attn_v": Q5K, "attn_output": Q4K, "ffn_down": Q5K}, 1: {"attn_v": Q4K, "attn_output": Q4K, "ffn_down": Q4K}}
# (key, shape, seed, build_model keywords, seq, positions, layers): the models of the GPU file.  The classifier is Q3_K (Gemma: its tied
# Q3_K embedding) except where the recipe's Q6_K one or a Q4_K one stands in: other Q8_K-rhs formats behind the same step.
CASES = [
    ("default/tiny-gqa", "tiny-gqa", 81, {}, 64, [0, 1, 40], [0, 1]),
    ("default/tiny-hd128", "tiny-hd128", 81, {"output_type": Q4K}, 64, [0, 1, 40], [0, 1]),
    ("default/tiny-qwen2-g7", "tiny-qwen2-g7", 81, {}, 64, [0, 1, 40], [0, 1]),
    ("default/tiny-gemma", "tiny-gemma", 81, {}, 64, [0, 1, 40], [0, 1]),
    ("rows/8b-rows", "8b-rows", 86, {}, 128, [0, 3], [0]),
    ("rows/dim8192", "dim8192", 86, {}, 128, [0, 3], [0]),
    # positions 0 and 100: the staged one-workgroup attention, and k_attn_flash handing its Q8_K planes to a wo of each format
    ("mix/tiny-gqa", "tiny-gqa", 83, {"n_layers": 3, "layer_types": MIX_LAYERS, "output_type": Q6K}, 256, [0, 100], [0, 1, 2]),
    ("recipe-M/tiny-hd128", "tiny-hd128", 84, {"q3_k_mix": "M"}, 64, [0, 5], [0, 1]),
    ("recipe-L/tiny-qwen2-g7", "tiny-qwen2-g7", 84, {"q3_k_mix": "L"}, 64, [0, 5], [1]),
    ("flags/tiny-gqa", "tiny-gqa", 82, {}, 64, [0, 7], [0, 1]),
    # d (and the mixes' dmin) flipped independently, some d = +-0 (tests/edge_blocks.flip_scale_signs)
    ("mixed-signs/tiny-gqa", "tiny-gqa", 89, {"q3_k_mix": "M"}, 64, [0, 5], [0, 1]),
]


def build(case):
    key, shape, seed, kw, _, _, _ = case
    if key.startswith("mixed-signs/"):
        from tests import edge_blocks as eb
        return eb.mixed_sign_model(shape_of(shape), Q3K, seed, **kw)
    return synth.build_model(shape_of(shape), Q3K, seed=seed, **kw)


def q3k_tensor(rng, rows, k):
    return synth.RawTensor(synth.random_blocks(rng, rows * k, Q3K), [rows, k], Q3K)


def test_q3_k_rows_of_the_restatement_equal_the_reference_dequantizer(oracle):
    """weight_rows' Q3_K fields as this module re-derives them from the raw block (the field order, the 2-bit fields, the hmask bit as
    bit 2, the 6-bit scales) against the oracle's dequantize, in its own f32 steps (buf_q3_k.rs:62-83: d * (scale - 32) first, then
    times the level)"""
    rng = np.random.default_rng(4)
    t = q3k_tensor(rng, 8, 512)
    w = Q.weight_rows(t, 0, 8)
    f = np.float32
    lv = w["lv"].reshape(8, 2, 16, 16)
    assert lv.max() == 3 and lv.min() == -4 and 24 < w["sc"].max() <= 31 and -32 <= w["sc"].min() < -24  # (256 scales drawn: both ends' neighbourhood)
    mine = (w["d"].astype(f)[:, :, None] * w["sc"].astype(f))[:, :, :, None] * lv.astype(f)
    assert np.array_equal(mine.reshape(-1), o.dequantize(t.data, o.Q3_K))
    assert np.allclose(Q.k_values(w).reshape(-1), mine.reshape(-1).astype(np.float64), rtol=1e-6, atol=0)
    # ... and the scales are tests/edge_blocks' (an unpack written independently of this one)
    from tests import edge_blocks as eb
    assert np.array_equal(Q.scales(w["s12"]).reshape(-1, 16) + 32, eb._q3k_scales(w["s12"].reshape(-1, 12)).reshape(-1, 16) & 63)


def test_q3_k_row_dots_equal_the_reference_vec_dot(oracle):
    """the exact row dot of this module against the reference's scalar vec_dot (another association: eight f32 lanes per super-block,
    the one the bound's A is taken from), within the bound"""
    rng = np.random.default_rng(5)
    for k in (512, 1792):
        t = q3k_tensor(rng, 16, k)
        x = (rng.standard_normal(k) * 1.5).astype(np.float32)
        xq = o.quantize(x, o.Q8_K)
        exact, bound = Q.row_dots(t, R.parse_act(xq, o.Q8_K))
        rows = np.ascontiguousarray(t.data).reshape(16, -1)
        got = np.array([o.vec_dot(rows[r], o.Q3_K, xq, k) for r in range(16)], dtype=np.float64)
        assert np.all(np.abs(got - exact) <= bound), (k, float(np.max(np.abs(got - exact) / bound)))


@pytest.mark.parametrize("k", [512, 1792, 4096, 14336])
def test_bound_holds_an_f32_emulation_in_permuted_orders(oracle, k):
    """the kernel's term evaluated in f32 -- f32(d) * d8, times the exact integer converted -- and the nsb terms added in f32 in ascending,
    reversed and random orders: inside (n_terms + C_Q3K) U sum A on every row; and the bound is below the project's 8 GEMV_REL sum |w x|"""
    from tests.helpers import GEMV_REL
    rng = np.random.default_rng(k)
    rows = 48
    t = q3k_tensor(rng, rows, k)
    act = q8k(rng, k)
    exact, bound = Q.row_dots(t, act)
    w = Q.weight_rows(t, 0, rows)
    f = np.float32
    # the exact integers, formed here in int64 (not taken from k_terms): levels 0 .. 7 against q8, minus 4 bsums, times the scale - 32
    nsb = k // 256
    x = act["q"].astype(np.int64).reshape(nsb, 16, 16)
    S = np.einsum("rsgi,sgi->rsg", Q.levels(w["q2"], w["hmask"]).reshape(rows, nsb, 16, 16), x) - 4 * act["bsums"].astype(np.int64)[None]
    tot = (Q.scales(w["s12"]) * S).sum(axis=2)
    assert np.abs(tot).max() < 2 ** 24
    terms = ((w["d"].astype(f) * act["d"].astype(f)[None]).astype(f) * tot.astype(f)).astype(f)
    n = terms.shape[1]
    for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n), rng.permutation(n)):
        acc = np.zeros(rows, dtype=f)
        for j in order:
            acc = (acc + terms[:, j]).astype(f)
        assert np.all(np.abs(acc.astype(np.float64) - exact) <= bound), (k, float(np.max(np.abs(acc - exact) / bound)))
    proj = GEMV_REL * (np.abs(Q.k_values(w)) @ np.abs(R.act_values(act)))
    assert np.all(bound <= 8 * proj), (k, float(np.max(bound / proj)))


@pytest.mark.parametrize("wrong", list(Q.WRONG) + ["last_block_dropped"])
def test_every_wrong_kernel_is_rejected(oracle, wrong):
    """a kernel that drops the hmask bit, takes it from the other half's bit (off by 4) or from the twin lane's piece, drops the -4 *
    bsum offset, takes a scale's high two bits from the neighbouring byte, forgets the -32, reads a neighbouring bsums entry, or stops
    one super-block early lands outside the bound"""
    rng = np.random.default_rng(11)
    for k in (512, 1792):
        t = q3k_tensor(rng, 64, k)
        act = q8k(rng, k)
        exact, bound = Q.row_dots(t, act)
        if wrong == "last_block_dropped":
            got, _ = Q.row_dots(t, act, drop_last_block=True)
        else:
            got, _ = Q.row_dots(t, act, wrong=wrong)
        out = np.abs(got.astype(np.float32).astype(np.float64) - exact) > bound
        assert out.mean() > 0.9, (wrong, k, float(out.mean()))


def test_wrong_rows_fail_in_the_launch_that_owns_them(oracle):
    """through check_layer: wo's x built from each wrong kernel's dots fails at `wo` (the oracle's own tap passes); and on a mixed
    layer the chained wrappers read the Q5_K V rows and the Q4_K wo"""
    model = Q.flip_signs(synth.build_model(synth.SHAPES["tiny-gqa"], Q3K, seed=22, n_layers=2))
    tap, kc, vc, form, aux = _tap(model, 7, 1)
    res = Q.check_layer(tap, kc, vc, model, 1, 7, form, "oracle", twin=aux["twin"])
    assert not Q.failures(res), Q.failures(res)
    rhs = R._rhs(tap, "attn.act_attn", "attn.attn", o.Q8_K)
    for wrong in list(Q.WRONG) + [True]:
        dots = Q.row_dots(model.tensors["blk.1.attn_output.weight"], rhs, drop_last_block=wrong is True, wrong=None if wrong is True else wrong)[0]
        bad = dict(tap)
        bad["wo.x"] = (np.asarray(tap["qkv_in.x"], dtype=np.float64) + dots).astype(np.float32)
        got = Q.check_layer(bad, kc, vc, model, 1, 7, form, "mutant", twin=aux["twin"])["wo"]
        assert any("x row" in f for f in got.fails), (wrong, got.fails, got.worst)
    mixed = synth.build_model(synth.SHAPES["tiny-gqa"], Q3K, seed=23, n_layers=2, layer_types=MIX_LAYERS, output_type=Q6K)
    tap, kc, vc, form, aux = _tap(mixed, 3, 0)
    res = Q.check_layer(tap, kc, vc, mixed, 0, 3, form, "oracle mix", twin=aux["twin"])
    assert not Q.failures(res), Q.failures(res)


def test_shrink_residual_knows_the_family(oracle):
    """Q3_K's d sits at byte 108 (a mixed layer's Q4_K / Q5_K scales where those formats keep them): every f16 scale field of the
    writers of the residual stream is the old one times 2^-9 rounded to f16, no other byte of the model moves, and the Q3_K embedding
    dequantizes to 2^-9 of itself"""
    from tests import edge_blocks as eb
    kw = dict(seed=24, n_layers=2, layer_types=MIX_LAYERS, output_type=Q6K)
    a, b = synth.build_model(synth.SHAPES["tiny-gqa"], Q3K, **kw), Q.shrink_residual(synth.build_model(synth.SHAPES["tiny-gqa"], Q3K, **kw))
    for name, t in a.tensors.items():
        writer = name == "token_embd.weight" or name.endswith("attn_output.weight") or name.endswith("ffn_down.weight")
        if not writer:
            assert np.array_equal(t.data, b.tensors[name].data), name
            continue
        fmt = synth.TYPE_NAMES[t.typ]
        fa, fb = eb.scale_fields(t.data, fmt), eb.scale_fields(b.tensors[name].data, fmt)
        for k in fa:
            assert np.array_equal(fb[k], (fa[k] * 2.0 ** -9).astype(np.float16).astype(np.float64)), (name, k)
        at = [x for x in eb.SCALE_AT[fmt] if x is not None]
        keep = np.ones(synth.BLOCK_BYTES[t.typ], dtype=bool)
        for x in at:
            keep[x:x + 2] = False
        assert np.array_equal(t.data.reshape(-1, keep.size)[:, keep], b.tensors[name].data.reshape(-1, keep.size)[:, keep]), name
    emb = a.tensors["token_embd.weight"]
    va, vb = o.dequantize(emb.data, emb.typ).astype(np.float64), o.dequantize(b.tensors["token_embd.weight"].data, emb.typ).astype(np.float64)
    # (a shrunk d of ~1e-5 is an f16 subnormal: spacing 2^-24, half of it up to a percent of the value; a wrong byte is off by factors)
    assert np.allclose(vb, va * 2.0 ** -9, rtol=2e-2, atol=0)


@pytest.mark.parametrize("case", [c for c in CASES if shape_of(c[1]).arch != "gemma"], ids=lambda c: c[0])
def test_oracle_step_passes_and_excused_shares_stay_under_the_cap(oracle, case):
    """the reference's own step (oracle forward on the CPU, every form the GPU file taps) passes the checker, and the excused share of
    the Q8_K interval check -- a property of the reference's values alone -- is at most EXCUSED_CAP for every plane set.  (Gemma's
    case is not evaluated here: the oracle tap of tests/test_fused_step_ref.py restates the Llama / Qwen2 step only.)"""
    key, _, _, _, seq, positions, layers = case
    model = build(case)
    shares = []
    with oracle_tokens(seq, max(positions) + 1):
        for pos in positions:
            for layer in layers:
                for form in (("default", "no-k-norm-in", "no-rhs-prologue") if key.startswith("flags/") else ("default",)):  # (the forms that case taps)
                    tap, kc, vc, frm, aux = _tap(model, pos, layer, form)
                    ctx = f"{key} {form} layer {layer} pos {pos}"
                    res = Q.check_layer(tap, kc, vc, model, layer, pos, frm, ctx, twin=aux["twin"])
                    assert not Q.failures(res), Q.failures(res)
                    for r in res.values():
                        for name, share in r.excused.items():
                            shares.append(share)
                            assert share <= Q.EXCUSED_CAP, (ctx, r.launch, name, share)
    assert shares
    print(f"{key}: excused shares of the Q8_K interval check: max {max(shares):.2e}, mean {np.mean(shares):.2e} over {len(shares)} plane sets")
