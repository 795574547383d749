"""Which launches a Q2_K decode context runs, on the record-only test device (tests/test_step_plan.py's device and read-out, through
tests/step_plan_cases.case / tests/test_q5k_step_plan.Evaluator with this file's own formats).  The Q2_K recipe family -- attn_q,
attn_k, ffn_gate and ffn_up in Q2_K in every layer; attn_v, attn_output and ffn_down each Q2_K, Q3_K or Q4_K, per layer and per
tensor: plain Q2_K and the Q2_K / Q2_K_S recipes (synth.q2_k_mix_types), with a Q6_K or Q4_K classifier or Gemma's tied embedding --
takes the K-quant fused segments (path 2, enqueue_segment_k, five launches per layer) on the fast device in the norm-epilogue form,
the only form the Q2_K body is built in.  Everything else keeps the per-op segments (path 0): the strict-order device (there is no
ordered Q2_K form), NO_KQUANT_FUSION, a tensor-parallel rank, a context without the norm epilogue, a classifier whose rhs is not
Q8_K, and a Q2_K body with any other deviation (attn_q in another type, Q5_K or Q6_K anywhere in a layer).  The forms behind the other
A/B flags are all built for Q2_K and stay on path 2 with the plan Q4_K reads under the same flag.  The Q3_K family does not grow: a
Q3_K body holding a Q2_K tensor stays per-op."""
import os

import numpy as np
import pytest

os.environ["CRABML_HIP_TEST_HOOKS"] = "1"

import crabml_amd as ca  # noqa: E402
from crabml_amd import synth  # noqa: E402
from tests import step_plan_cases as spc  # noqa: E402
from tests import test_q5k_step_plan as P5  # noqa: E402

FORMATS = {"Q2_K": (synth.Q2_K, {}), "Q2_K-recipe-K": (synth.Q2_K, {"q2_k_mix": "K"}), "Q2_K-recipe-S": (synth.Q2_K, {"q2_k_mix": "S"}),
           "Q2_K+Q4_K": (synth.Q2_K, {"output_type": synth.Q4_K}), "Q2_K+Q4_0": (synth.Q2_K, {"output_type": synth.Q4_0}),
           "Q3_K": (synth.Q3_K, {}), "Q4_K": spc.FORMATS["Q4_K"]}
Q2 = ("Q2_K", "Q2_K-recipe-K", "Q2_K-recipe-S", "Q2_K+Q4_K")
SHAPES = P5.SHAPES          # tiny-gqa, tiny-hd128, tiny-qwen2, tiny-gemma (tied: the classifier is the Q2_K embedding, or the recipe's Q6_K)
PER_OP = (0, 0, 0, 0, 0)


def _retype(model, name, typ):
    t = model.tensors[name]
    rows, cols = t.shape
    model.tensors[name] = synth.RawTensor(synth.random_blocks(np.random.default_rng(9), rows * cols, typ, 1.0), [rows, cols], typ)
    return model


def attn_q_in_q3k(model):
    """a deviation outside the family: layer 1's attn_q in Q3_K (layer 0's decides the body's format)"""
    return _retype(model, "blk.1.attn_q.weight", synth.Q3_K)


def attn_v_in_q5k(model):
    """... a Q5_K tensor where the family allows Q2_K, Q3_K or Q4_K only: layer 0's attn_v"""
    return _retype(model, "blk.0.attn_v.weight", synth.Q5_K)


def ffn_down_in_q6k(model):
    """... and a Q6_K one: layer 1's ffn_down"""
    return _retype(model, "blk.1.ffn_down.weight", synth.Q6_K)


def attn_v_in_q2k(model):
    """(on a Q3_K body) a Q2_K attn_v: not a member of the Q3_K family"""
    return _retype(model, "blk.0.attn_v.weight", synth.Q2_K)


class Evaluator(P5.Evaluator):
    """the Q5_K file's evaluator over this file's formats and edits"""
    EDITS = {"attn_q_q3k": attn_q_in_q3k, "attn_v_q5k": attn_v_in_q5k, "ffn_down_q6k": ffn_down_in_q6k, "attn_v_q2k": attn_v_in_q2k}

    def plan(self, c):
        saved = P5.FORMATS
        P5.FORMATS = FORMATS
        try:
            return super().plan(c)
        finally:
            P5.FORMATS = saved


@pytest.fixture(scope="module")
def ev():
    return Evaluator(ca, "dry")


words = P5.words


@pytest.mark.parametrize("fmt", Q2)
@pytest.mark.parametrize("shape", SHAPES)
def test_fast_q2k_takes_the_fused_k_segments(ev, shape, fmt):
    """path 2 in the default form: norm epilogue, Q8_K producers, gate | up normalizing wo's row itself; with both caches"""
    assert words(ev.plan(spc.case(shape, fmt))) == (2, 0, 1, 1, 1)
    assert words(ev.plan(spc.case(shape, fmt, kv_f16=False))) == (2, 0, 1, 1, 1)


def test_the_recipes_are_the_table():
    """synth's recipes against DESIGN.md's table on 32 layers (n_layers / 8 = 4), at GQA groups 1 and 4"""
    Q2K, Q3K, Q4K = synth.Q2_K, synth.Q3_K, synth.Q4_K
    for l in range(32):
        assert synth.q2_k_mix_types("K", l, 32, 1) == {"attn_v": Q3K, "attn_output": Q3K, "ffn_down": Q3K}
        assert synth.q2_k_mix_types("K", l, 32, 4) == {"attn_v": Q4K, "attn_output": Q3K, "ffn_down": Q3K}
        for grp in (1, 4):
            assert synth.q2_k_mix_types("S", l, 32, grp) == ({"ffn_down": Q4K} if l < 4 else {})
    # a built model: tiny-gqa has group 4, tiny-hd128 group 2; the recipes' Q6_K classifier, a Q2_K embedding
    for shape, v in (("tiny-gqa", Q4K), ("tiny-hd128", Q3K)):
        m = synth.build_model(synth.SHAPES[shape], Q2K, q2_k_mix="K")
        got = {n: t.typ for n, t in m.tensors.items() if not n.endswith("norm.weight")}
        assert all(got[f"blk.{l}.attn_v.weight"] == v and got[f"blk.{l}.attn_output.weight"] == got[f"blk.{l}.ffn_down.weight"] == Q3K
                   for l in range(2))
        assert got["output.weight"] == synth.Q6_K and got["token_embd.weight"] == Q2K
        assert all(got[f"blk.{l}.{n}.weight"] == Q2K for l in range(2) for n in ("attn_q", "attn_k", "ffn_gate", "ffn_up"))
    m = synth.build_model(synth.SHAPES["tiny-gqa"], Q2K, q2_k_mix="S", n_layers=8)
    assert [m.tensors[f"blk.{l}.ffn_down.weight"].typ for l in range(8)] == [Q4K] + [Q2K] * 7
    assert m.tensors["output.weight"].typ == synth.Q6_K


def test_defaults_leave_existing_models_byte_identical():
    """q2_k_mix = None draws nothing: a model built without it is the one build_model made before the keyword existed"""
    a = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q2_K, seed=3)
    b = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q2_K, seed=3, q2_k_mix=None)
    assert list(a.tensors) == list(b.tensors) and "output.weight" in a.tensors and a.tensors["output.weight"].typ == synth.Q2_K
    assert all(np.array_equal(a.tensors[n].data, b.tensors[n].data) for n in a.tensors)


@pytest.mark.parametrize("fmt", Q2)
@pytest.mark.parametrize("shape", SHAPES)
def test_what_stays_on_the_per_op_segments(ev, shape, fmt):
    assert words(ev.plan(spc.case(shape, fmt, strict=True))) == PER_OP             # no ordered Q2_K form
    assert words(ev.plan(spc.case(shape, fmt, flag="NO_KQUANT_FUSION"))) == PER_OP
    assert words(ev.plan(spc.case(shape, fmt, strict=True, flag="NO_KQUANT_FUSION"))) == PER_OP
    # the one form Q2_K is not built in: wo / ffn_down without the norm epilogue
    assert words(ev.plan(spc.case(shape, fmt, norm_epilogue=False))) == PER_OP


@pytest.mark.parametrize("fmt", Q2)
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128"])
def test_a_tensor_parallel_rank_stays_per_op(ev, shape, fmt):
    for strict in (False, True):
        assert words(ev.plan(spc.case(shape, fmt, strict, flag="TP_DRY_RUN", tp_size=2))) == PER_OP


@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128", "tiny-qwen2"])
def test_a_classifier_whose_rhs_is_not_q8k_stays_per_op(ev, shape):
    """a Q4_0 classifier takes Q8_0 rows: the K-quant norm epilogue leaves Q8_K planes only (Gemma's classifier is its embedding)"""
    assert words(ev.plan(spc.case(shape, "Q2_K+Q4_0"))) == PER_OP


@pytest.mark.parametrize("edit", ["attn_q_q3k", "attn_v_q5k", "ffn_down_q6k"])
@pytest.mark.parametrize("fmt", Q2)
@pytest.mark.parametrize("shape", SHAPES)
def test_a_q2k_body_with_a_deviation_outside_the_family_stays_per_op(ev, shape, fmt, edit):
    assert words(ev.plan(spc.case(shape, fmt, edit=edit))) == PER_OP


@pytest.mark.parametrize("shape", SHAPES)
def test_the_q3k_family_does_not_grow(ev, shape):
    """a Q3_K body with a Q2_K attn_v keeps the per-op segments (the plain Q3_K body of the same shape: path 2)"""
    assert words(ev.plan(spc.case(shape, "Q3_K"))) == (2, 0, 1, 1, 1)
    assert words(ev.plan(spc.case(shape, "Q3_K", edit="attn_v_q2k"))) == PER_OP


@pytest.mark.parametrize("flag", ["NO_RHS_PROLOGUE", "NO_Q8K_PRODUCERS", "NO_K_NORM_IN", "SPLIT_CHUNKS_ALWAYS", "SPLIT_CHUNKS_NEVER"])
@pytest.mark.parametrize("fmt", Q2)
def test_the_flag_forms_are_built_and_read_as_q4k_does(ev, fmt, flag):
    """every A/B form of the norm-epilogue step exists for the Q2_K body: the whole plan of the Q4_K case of the same flag"""
    for shape in SHAPES:
        got, want = ev.plan(spc.case(shape, fmt, flag=flag)), ev.plan(spc.case(shape, "Q4_K", flag=flag))
        assert got["path"] == 2 and got == want, (shape, got, want)


@pytest.mark.parametrize("fmt", Q2)
def test_a_shape_whose_head_dim_has_no_producer(ev, fmt):
    """q8k_producers off by shape (head_dim 32 is none of 64 / 128 / 256): still path 2, planes out of wo"""
    assert words(ev.plan(spc.case("q5k-hd32", fmt))) == (2, 0, 1, 0, 0)
