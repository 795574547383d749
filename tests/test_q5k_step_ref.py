"""The Q5_K checker (tests/q5k_step_ref.py) checked on the CPU: its unpack against the reference's dequantizer, its bound against an f32
emulation of the kernel's term in permuted add orders, every subtly wrong kernel it must reject, and -- from the reference alone, an
oracle-built tap of the step -- that it accepts the reference's own order and that the Q8_K interval check excuses no more than
EXCUSED_CAP of any plane set for the shapes, seeds and positions tests/test_hip_q5k_fused.py uses (CASES below is that file's list:
it imports it)."""
import contextlib

import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests import q5k_step_ref as Q
from tests import test_fused_step_ref as T

# (key, shape, seed, build_model keywords, seq, positions, layers): the models of the GPU file.  A Llama / Qwen2 shape gets a Q6_K
# classifier; the 8-layer recipe is llama.cpp's Q5_K_M (use_more_bits: layers 0, 3, 6, 7).
CASES = [
    ("default/tiny-gqa", "tiny-gqa", 51, {"output_type": synth.Q6_K}, 64, [0, 1, 40], [0, 1]),
    ("default/tiny-hd128", "tiny-hd128", 51, {"output_type": synth.Q6_K}, 64, [0, 1, 40], [0, 1]),
    ("default/tiny-qwen2-g7", "tiny-qwen2-g7", 51, {"output_type": synth.Q6_K}, 64, [0, 1, 40], [0, 1]),
    ("default/tiny-gemma", "tiny-gemma", 51, {}, 64, [0, 1, 40], [0, 1]),
    ("k-m-mix/tiny-gqa", "tiny-gqa", 53, {"n_layers": 8, "k_m_mix": True}, 64, [0, 7], [3, 4, 7]),
    ("rows/8b-rows", "8b-rows", 56, {"output_type": synth.Q6_K}, 128, [0, 3], [0, 1]),
    ("rows/dim8192", "dim8192", 56, {"output_type": synth.Q6_K}, 128, [0, 3], [0, 1]),
    ("flags/tiny-gqa", "tiny-gqa", 52, {"output_type": synth.Q6_K}, 64, [0, 7], [0, 1]),
    ("switch/tiny-gqa", "tiny-gqa", 55, {"output_type": synth.Q6_K}, 256, [94, 95, 96, 200], [0, 1]),
    ("signs/tiny-gqa", "tiny-gqa", 57, {"k_m_mix": True}, 64, [0, 5], [0, 1]),
    ("shrunk/tiny-gqa", "tiny-gqa", 58, {"k_m_mix": True}, 64, [0, 5], [0, 1]),
    # d and dmin flipped independently, some d = +-0 (tests/edge_blocks.flip_scale_signs)
    ("mixed-signs/tiny-gqa", "tiny-gqa", 59, {"k_m_mix": True}, 64, [0, 5], [0, 1]),
]


def shape_of(name):
    from tests.test_hip_fused_launches import SHAPE_8B, SHAPE_WIDE
    return {"8b-rows": SHAPE_8B, "dim8192": SHAPE_WIDE}.get(name) or synth.SHAPES[name]


def build(case):
    key, shape, seed, kw, _, _, _ = case
    model = synth.build_model(shape_of(shape), synth.Q5_K, seed=seed, **kw)
    if key.startswith("signs/"):
        Q.flip_signs(model)
    if key.startswith("shrunk/"):
        Q.shrink_residual(model, log2=9)
    if key.startswith("mixed-signs/"):
        from tests import edge_blocks as eb
        model = eb.flip_scale_signs(model, np.random.default_rng([seed, 1]))
    return model


@contextlib.contextmanager
def oracle_tokens(seq, n):
    """tests/test_fused_step_ref.oracle_tap_k teacher-forces its module's TOKS into a cache of SEQ positions: longer ones for this file"""
    saved = T.SEQ, T.TOKS
    T.SEQ, T.TOKS = seq, [1] + [int(t) for t in np.random.default_rng(77).integers(2, 1000, size=n)]
    try:
        yield
    finally:
        T.SEQ, T.TOKS = saved


def q5k_tensor(rng, rows, k):
    return synth.RawTensor(synth.random_blocks(rng, rows * k, synth.Q5_K), [rows, k], synth.Q5_K)


def q8k(rng, k):
    return R.parse_act(o.quantize((rng.standard_normal(k) * rng.uniform(0.2, 3.0)).astype(np.float32), o.Q8_K), o.Q8_K)


def test_q5_k_rows_of_the_restatement_equal_the_reference_dequantizer(oracle):
    """weight_rows' Q5_K fields (the field order of the block, the 6-bit unpack, the nibble order, the fifth bits) against the oracle's
    dequantize, in its own f32 steps"""
    rng = np.random.default_rng(4)
    t = q5k_tensor(rng, 8, 512)
    w = Q.weight_rows(t, 0, 8)
    f = np.float32
    d1 = (w["d"].astype(f)[:, :, None] * w["sc"].astype(f))[:, :, :, None]
    m1 = (w["dmin"].astype(f)[:, :, None] * w["mn"].astype(f))[:, :, :, None]
    mine = d1 * w["q"].reshape(8, 2, 8, 32).astype(f) - m1
    assert np.array_equal(mine.reshape(-1), o.dequantize(t.data, o.Q5_K))
    assert w["q"].max() == 31 and w["q"].min() == 0 and np.any(w["q"] != w["nib"])
    assert np.allclose(Q.k_values(w).reshape(-1), mine.reshape(-1).astype(np.float64), rtol=1e-6, atol=0)


@pytest.mark.parametrize("k", [512, 1792, 4096, 14336])
def test_bound_holds_an_f32_emulation_in_permuted_orders(oracle, k):
    """the kernel's term evaluated in f32 -- f32(d d8), f32(dmin d8), their products with the exact integers, the subtraction -- and the
    8 nsb terms added in f32 in ascending, reversed and random orders: inside (n_terms + C_K) U sum A on every row; and the bound is below the
    project's 8 GEMV_REL sum |w x|.  (The reference's scalar vec_dot -- another association altogether -- is held to it by the oracle-step
    test below.)"""
    from tests.helpers import GEMV_REL
    rng = np.random.default_rng(k)
    rows = 48
    t = q5k_tensor(rng, rows, k)
    act = q8k(rng, k)
    exact, bound = Q.row_dots(t, act)
    w = Q.weight_rows(t, 0, rows)
    f = np.float32
    # the exact integers, formed here in int64 (not taken from k_pieces)
    nsb = k // 256
    x = act["q"].astype(np.int64).reshape(nsb, 4, 2, 2, 16)
    q = w["q"].astype(np.int64).reshape(rows, nsb, 4, 2, 2, 16)
    S = np.einsum("rspghi,spghi->rspgh", q, x)
    isum = (w["sc"].astype(np.int64).reshape(rows, nsb, 4, 2)[..., None] * S).sum(axis=3)
    msum = (w["mn"].astype(np.int64).reshape(rows, nsb, 4, 2)[..., None] * act["bsums"].astype(np.int64).reshape(nsb, 4, 2, 2)[None]).sum(axis=3)
    assert np.abs(isum).max() < 2 ** 23
    dd = (w["d"].astype(f) * act["d"].astype(f)[None])[:, :, None, None]
    dm = (w["dmin"].astype(f) * act["d"].astype(f)[None])[:, :, None, None]
    terms = ((dd * isum.astype(f)).astype(f) - (dm * msum.astype(f)).astype(f)).astype(f).reshape(rows, -1)
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
    """a kernel that drops the fifth bit, swaps the low / high nibbles' fifth bits, shifts qh for the wrong pair, takes a neighbouring
    sub-block's scale or minimum, adds the minimum term, or stops one super-block early lands outside the bound"""
    rng = np.random.default_rng(11)
    for k in (512, 1792):
        t = q5k_tensor(rng, 64, k)
        act = q8k(rng, k)
        exact, bound = Q.row_dots(t, act)
        if wrong == "last_block_dropped":
            got, _ = Q.row_dots(t, act, drop_last_block=True)
        else:
            got, _ = Q.row_dots(t, act, wrong=wrong)
        out = np.abs(got.astype(np.float32).astype(np.float64) - exact) > bound
        # (a neighbouring scale / minimum may equal the right one on a row: 6-bit fields)
        assert out.mean() > 0.9, (wrong, k, float(out.mean()))


def _tap(model, pos, layer, form="default"):
    tap, kc, vc, frm, aux = T.oracle_tap_k(model, pos, layer, True, form)
    return tap, kc, vc, frm, aux


def test_wrong_rows_fail_in_the_launch_that_owns_them(oracle):
    """through check_layer: wo's x built from each wrong kernel's dots fails at `wo` (the oracle's own tap passes)"""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q5_K, seed=22, n_layers=2, output_type=synth.Q6_K)
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
