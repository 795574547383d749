"""Which launches a Q3_K decode context runs, on the record-only test device (tests/test_step_plan.py's device and read-out, through
tests/step_plan_cases.case / tests/test_q5k_step_plan.Evaluator with this file's own formats).  The Q3_K recipe family -- attn_q,
attn_k, ffn_gate and ffn_up in Q3_K in every layer; attn_v, attn_output and ffn_down each Q3_K, Q4_K or Q5_K, per layer and per
tensor: plain Q3_K and the Q3_K_S / Q3_K_M / Q3_K_L recipes (synth.q3_k_mix_types), with a Q6_K or Q4_K classifier or Gemma's tied
embedding -- takes the K-quant fused segments (path 2, enqueue_segment_k, five launches per layer) on the fast device in the
norm-epilogue form, the only form the Q3_K body is built in.  Everything else keeps the per-op segments (path 0): the strict-order
device (there is no ordered Q3_K form), NO_KQUANT_FUSION, a tensor-parallel rank, a context without the norm epilogue, a classifier
whose rhs is not Q8_K, and a Q3_K body with any other deviation (attn_q in another type, Q6_K anywhere in a layer).  The forms behind
the other A/B flags are all built for Q3_K and stay on path 2 with the plan Q4_K reads under the same flag."""
import os

import numpy as np
import pytest

os.environ["CRABML_HIP_TEST_HOOKS"] = "1"

import crabml_amd as ca  # noqa: E402
from crabml_amd import synth  # noqa: E402
from tests import step_plan_cases as spc  # noqa: E402
from tests import test_q5k_step_plan as P5  # noqa: E402

FORMATS = {"Q3_K": (synth.Q3_K, {}), "Q3_K_S": (synth.Q3_K, {"q3_k_mix": "S"}), "Q3_K_M": (synth.Q3_K, {"q3_k_mix": "M"}),
           "Q3_K_L": (synth.Q3_K, {"q3_k_mix": "L"}), "Q3_K+Q4_K": (synth.Q3_K, {"output_type": synth.Q4_K}),
           "Q3_K+Q4_0": (synth.Q3_K, {"output_type": synth.Q4_0}), "Q4_K": spc.FORMATS["Q4_K"]}
Q3 = ("Q3_K", "Q3_K_S", "Q3_K_M", "Q3_K_L", "Q3_K+Q4_K")
SHAPES = P5.SHAPES          # tiny-gqa, tiny-hd128, tiny-qwen2, tiny-gemma (tied: the classifier is the Q3_K embedding, or the recipe's Q6_K)
ALL_SHAPES = P5.ALL_SHAPES  # ... and the head_dim-32 shape none of the Q8_K-producing attention kernels is built for
PER_OP = (0, 0, 0, 0, 0)


def _retype(model, name, typ):
    t = model.tensors[name]
    rows, cols = t.shape
    model.tensors[name] = synth.RawTensor(synth.random_blocks(np.random.default_rng(9), rows * cols, typ, 1.0), [rows, cols], typ)
    return model


def attn_q_in_q4k(model):
    """a deviation outside the family: layer 1's attn_q in Q4_K (layer 0's decides the body's format)"""
    return _retype(model, "blk.1.attn_q.weight", synth.Q4_K)


def attn_v_in_q6k(model):
    """... and a Q6_K tensor where the family allows Q3_K, Q4_K or Q5_K only: layer 0's attn_v"""
    return _retype(model, "blk.0.attn_v.weight", synth.Q6_K)


class Evaluator(P5.Evaluator):
    """the Q5_K file's evaluator over this file's formats and edits"""
    EDITS = {"attn_q_q4k": attn_q_in_q4k, "attn_v_q6k": attn_v_in_q6k}

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


@pytest.mark.parametrize("fmt", Q3)
@pytest.mark.parametrize("shape", SHAPES)
def test_fast_q3k_takes_the_fused_k_segments(ev, shape, fmt):
    """path 2 in the default form: norm epilogue, Q8_K producers, gate | up normalizing wo's row itself; with both caches"""
    assert words(ev.plan(spc.case(shape, fmt))) == (2, 0, 1, 1, 1)
    assert words(ev.plan(spc.case(shape, fmt, kv_f16=False))) == (2, 0, 1, 1, 1)


def test_the_recipes_are_the_table():
    """synth's recipes against DESIGN.md's table, on a depth where every row of it shows (32 layers: n_layers / 16 = 2)"""
    Q3K, Q4K, Q5K = synth.Q3_K, synth.Q4_K, synth.Q5_K
    for l in range(32):
        assert synth.q3_k_mix_types("S", l, 32) == {}
        assert synth.q3_k_mix_types("L", l, 32) == {"attn_v": Q5K, "attn_output": Q5K, "ffn_down": Q5K}
        assert synth.q3_k_mix_types("M", l, 32) == {"attn_v": Q5K if l < 2 else Q4K, "attn_output": Q4K, "ffn_down": Q5K if l < 2 else Q4K}
    assert synth.q3_k_mix_types("M", 0, 2)["ffn_down"] == Q4K  # (n_layers / 16 is 0 on a test model: layer_types puts a Q5_K one there)
    m = synth.build_model(synth.SHAPES["tiny-gqa"], Q3K, q3_k_mix="M", layer_types={0: {"ffn_down": Q5K}})
    got = {n: t.typ for n, t in m.tensors.items() if not n.endswith("norm.weight")}
    assert got["blk.0.ffn_down.weight"] == Q5K and got["blk.1.ffn_down.weight"] == Q4K
    assert got["blk.0.attn_v.weight"] == got["blk.1.attn_v.weight"] == Q5K and got["blk.0.attn_output.weight"] == Q4K
    assert got["output.weight"] == synth.Q6_K and got["token_embd.weight"] == Q3K
    assert all(got[f"blk.{l}.{n}.weight"] == Q3K for l in range(2) for n in ("attn_q", "attn_k", "ffn_gate", "ffn_up"))


@pytest.mark.parametrize("fmt", Q3)
@pytest.mark.parametrize("shape", SHAPES)
def test_what_stays_on_the_per_op_segments(ev, shape, fmt):
    assert words(ev.plan(spc.case(shape, fmt, strict=True))) == PER_OP             # no ordered Q3_K form
    assert words(ev.plan(spc.case(shape, fmt, flag="NO_KQUANT_FUSION"))) == PER_OP
    assert words(ev.plan(spc.case(shape, fmt, strict=True, flag="NO_KQUANT_FUSION"))) == PER_OP
    # the one form Q3_K is not built in: wo / ffn_down without the norm epilogue
    assert words(ev.plan(spc.case(shape, fmt, norm_epilogue=False))) == PER_OP


@pytest.mark.parametrize("fmt", Q3)
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128"])
def test_a_tensor_parallel_rank_stays_per_op(ev, shape, fmt):
    for strict in (False, True):
        assert words(ev.plan(spc.case(shape, fmt, strict, flag="TP_DRY_RUN", tp_size=2))) == PER_OP


@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128", "tiny-qwen2"])
def test_a_classifier_whose_rhs_is_not_q8k_stays_per_op(ev, shape):
    """a Q4_0 classifier takes Q8_0 rows: the K-quant norm epilogue leaves Q8_K planes only (Gemma's classifier is its embedding)"""
    assert words(ev.plan(spc.case(shape, "Q3_K+Q4_0"))) == PER_OP


@pytest.mark.parametrize("edit", ["attn_q_q4k", "attn_v_q6k"])
@pytest.mark.parametrize("fmt", Q3)
@pytest.mark.parametrize("shape", SHAPES)
def test_a_q3k_body_with_a_deviation_outside_the_family_stays_per_op(ev, shape, fmt, edit):
    assert words(ev.plan(spc.case(shape, fmt, edit=edit))) == PER_OP


@pytest.mark.parametrize("flag", ["NO_RHS_PROLOGUE", "NO_Q8K_PRODUCERS", "NO_K_NORM_IN", "SPLIT_CHUNKS_ALWAYS", "SPLIT_CHUNKS_NEVER"])
@pytest.mark.parametrize("fmt", Q3)
def test_the_flag_forms_are_built_and_read_as_q4k_does(ev, fmt, flag):
    """every A/B form of the norm-epilogue step exists for the Q3_K body: the whole plan of the Q4_K case of the same flag"""
    for shape in SHAPES:
        got, want = ev.plan(spc.case(shape, fmt, flag=flag)), ev.plan(spc.case(shape, "Q4_K", flag=flag))
        assert got["path"] == 2 and got == want, (shape, got, want)


@pytest.mark.parametrize("fmt", Q3)
def test_a_shape_whose_head_dim_has_no_producer(ev, fmt):
    """q8k_producers off by shape (head_dim 32 is none of 64 / 128 / 256): still path 2, planes out of wo"""
    assert words(ev.plan(spc.case("q5k-hd32", fmt))) == (2, 0, 1, 0, 0)
