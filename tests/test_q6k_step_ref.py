"""The Q6_K checker (tests/q6k_step_ref.py) checked on the CPU: its unpack against the reference's dequantizer, its bound against an f32
emulation of the kernel's term in permuted add orders, every subtly wrong kernel it must reject, and -- from the reference alone, an
oracle-built tap of the step -- that it accepts the reference's own order and that the Q8_K interval check excuses no more than
EXCUSED_CAP of any plane set for the shapes, seeds and positions tests/test_hip_q6k_fused.py uses (CASES below is that file's list:
it imports it)."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests import q6k_step_ref as Q
from tests.test_q5k_step_ref import _tap, oracle_tokens, q8k, shape_of

# (key, shape, seed, build_model keywords, seq, positions, layers): the models of the GPU file, every layer matrix Q6_K.  The classifier
# is Q6_K too (Gemma: its tied Q6_K embedding) except where a Q4_K one stands in: another Q8_K-rhs format behind the same step.
CASES = [
    ("default/tiny-gqa", "tiny-gqa", 61, {}, 64, [0, 1, 40], [0, 1]),
    ("default/tiny-hd128", "tiny-hd128", 61, {"output_type": synth.Q4_K}, 64, [0, 1, 40], [0, 1]),
    ("default/tiny-qwen2-g7", "tiny-qwen2-g7", 61, {}, 64, [0, 1, 40], [0, 1]),
    ("default/tiny-gemma", "tiny-gemma", 61, {}, 64, [0, 1, 40], [0, 1]),
    ("rows/8b-rows", "8b-rows", 66, {}, 128, [0, 3], [0, 1]),
    ("rows/dim8192", "dim8192", 66, {}, 128, [0, 3], [0, 1]),
    ("flags/tiny-gqa", "tiny-gqa", 62, {}, 64, [0, 7], [0, 1]),
    ("switch/tiny-gqa", "tiny-gqa", 65, {}, 256, [94, 95, 96, 200], [0, 1]),
    ("signs/tiny-gqa", "tiny-gqa", 67, {}, 64, [0, 5], [0, 1]),
    ("shrunk/tiny-gqa", "tiny-gqa", 68, {}, 64, [0, 5], [0, 1]),
    # d and dmin flipped independently, some d = +-0 (tests/edge_blocks.flip_scale_signs)
    ("mixed-signs/tiny-gqa", "tiny-gqa", 69, {}, 64, [0, 5], [0, 1]),
]


def build(case):
    key, shape, seed, kw, _, _, _ = case
    model = synth.build_model(shape_of(shape), synth.Q6_K, seed=seed, **kw)
    if key.startswith("signs/"):
        Q.flip_signs(model)
    if key.startswith("shrunk/"):
        Q.shrink_residual(model, log2=9)
    if key.startswith("mixed-signs/"):
        from tests import edge_blocks as eb
        model = eb.flip_scale_signs(model, np.random.default_rng([seed, 1]))
    return model


def q6k_tensor(rng, rows, k):
    return synth.RawTensor(synth.random_blocks(rng, rows * k, synth.Q6_K), [rows, k], synth.Q6_K)


def test_q6_k_rows_of_the_restatement_equal_the_reference_dequantizer(oracle):
    """weight_rows' Q6_K fields as this module re-derives them (the nibble order, the two-bit fields of qh, the signed scales) against the
    oracle's dequantize, in its own f32 steps (buf_q6_k.rs:21-48: d * scale first, then times the level)"""
    rng = np.random.default_rng(4)
    t = q6k_tensor(rng, 8, 512)
    w = Q.weight_rows(t, 0, 8)
    f = np.float32
    lv = (Q.levels(w["lo4"], w["qh"]) - 32).reshape(8, 2, 16, 16)
    assert lv.max() == 31 and lv.min() == -32 and np.any(Q.levels(w["lo4"], w["qh"]) != Q.levels(w["lo4"], w["qh"], drop=True))
    mine = (w["d"].astype(f)[:, :, None] * w["sc"].astype(f))[:, :, :, None] * lv.astype(f)
    assert np.array_equal(mine.reshape(-1), o.dequantize(t.data, o.Q6_K))
    assert np.allclose(R.k_values(w).reshape(-1), mine.reshape(-1).astype(np.float64), rtol=1e-6, atol=0)
    # ... and this module's pieces are fused_step_ref's
    act = q8k(rng, 512)
    for mine_, theirs in zip(Q.k_pieces(w, act), R.k_pieces(w, act)):
        assert np.array_equal(mine_, theirs)
    for mine_, theirs in zip(Q.k_pieces(w, act, "q6_scale_shift"), R.k_pieces(w, act, "q6_scale_shift")):
        assert np.array_equal(mine_, theirs)


@pytest.mark.parametrize("k", [512, 1792, 4096, 14336])
def test_bound_holds_an_f32_emulation_in_permuted_orders(oracle, k):
    """the kernel's term evaluated in f32 -- f32(d d8), the two scaled integers converted and added, the product -- and the 8 nsb terms
    added in f32 in ascending, reversed and random orders: inside (n_terms + C_K) U sum A on every row; and the bound is below the
    project's 8 GEMV_REL sum |w x|.  (The reference's scalar vec_dot -- another association altogether -- is held to it by the oracle-step
    test below.)"""
    from tests.helpers import GEMV_REL
    rng = np.random.default_rng(k)
    rows = 48
    t = q6k_tensor(rng, rows, k)
    act = q8k(rng, k)
    exact, bound = Q.row_dots(t, act)
    w = Q.weight_rows(t, 0, rows)
    f = np.float32
    # the exact integers, formed here in int64 (not taken from k_pieces): levels 0 .. 63 against q8, minus 32 bsums, times the scale
    nsb = k // 256
    x = act["q"].astype(np.int64).reshape(nsb, 16, 16)
    S = np.einsum("rsgi,sgi->rsg", Q.levels(w["lo4"], w["qh"]).reshape(rows, nsb, 16, 16), x) - 32 * act["bsums"].astype(np.int64)[None]
    G = (w["sc"].astype(np.int64) * S).reshape(rows, nsb, 2, 2, 4)
    assert np.abs(G).max() < 2 ** 31
    dd = (w["d"].astype(f) * act["d"].astype(f)[None])[:, :, None, None]
    terms = (dd * (G[:, :, :, 0].astype(f) + G[:, :, :, 1].astype(f)).astype(f)).astype(f).reshape(rows, -1)
    n = terms.shape[1]
    for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n), rng.permutation(n)):
        acc = np.zeros(rows, dtype=f)
        for j in order:
            acc = (acc + terms[:, j]).astype(f)
        assert np.all(np.abs(acc.astype(np.float64) - exact) <= bound), (k, float(np.max(np.abs(acc - exact) / bound)))
    proj = GEMV_REL * (np.abs(R.k_values(w)) @ np.abs(R.act_values(act)))
    assert np.all(bound <= 8 * proj), (k, float(np.max(bound / proj)))


@pytest.mark.parametrize("wrong", list(Q.WRONG) + ["last_block_dropped"])
def test_every_wrong_kernel_is_rejected(oracle, wrong):
    """a kernel that drops the two qh bits, takes them with the twin lane's shift, swaps the low / high scales, takes a neighbouring
    scale, drops the -32 * bsum offset, reads a neighbouring bsums entry, loses the sign of d, or stops one super-block early lands
    outside the bound"""
    rng = np.random.default_rng(11)
    for k in (512, 1792):
        t = q6k_tensor(rng, 64, k)
        if wrong == "d_sign_lost":  # (random blocks carry positive d: give half of them the other sign)
            blk = t.data.reshape(-1, 210)
            blk[::2, 209] ^= 0x80
        act = q8k(rng, k)
        exact, bound = Q.row_dots(t, act)
        if wrong == "last_block_dropped":
            got, _ = Q.row_dots(t, act, drop_last_block=True)
        else:
            got, _ = Q.row_dots(t, act, wrong=wrong)
        out = np.abs(got.astype(np.float32).astype(np.float64) - exact) > bound
        # (a neighbouring scale may equal the right one on a row)
        assert out.mean() > 0.9, (wrong, k, float(out.mean()))


def test_wrong_rows_fail_in_the_launch_that_owns_them(oracle):
    """through check_layer: wo's x built from each wrong kernel's dots fails at `wo` (the oracle's own tap passes)"""
    model = Q.flip_signs(synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q6_K, seed=22, n_layers=2))
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


@pytest.mark.parametrize("case", [c for c in CASES if shape_of(c[1]).arch != "gemma"], ids=lambda c: c[0])
def test_oracle_step_passes_and_excused_shares_stay_under_the_cap(oracle, case):
    """the reference's own step (oracle forward on the CPU, every form the GPU file taps) passes the checker, and the excused share of
    the Q8_K interval check -- a property of the reference's values alone -- is at most EXCUSED_CAP for every plane set.  (Gemma's
    case is not evaluated here: the oracle tap of tests/test_fused_step_ref.py restates the Llama / Qwen2 step only.)"""
    key, _, _, _, seq, positions, layers = case
    model = build(case)
    big = model.shape.dim >= 4096
    shares = []
    with oracle_tokens(seq, max(positions) + 1):
        for pos in positions:
            for layer in (layers[:1] if big else layers):  # (the long-row shapes: one layer's planes; the other's come from the same x)
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
