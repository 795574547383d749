"""Which launches a Q6_K decode context runs, on the record-only test device (tests/test_step_plan.py's device and read-out, through
tests/step_plan_cases.case / Evaluator with this file's own formats): a context whose layer matrices are ALL Q6_K -- with a Q6_K
classifier, with Gemma's tied Q6_K embedding, or in front of a Q4_K classifier (still a Q8_K rhs) -- takes the K-quant fused
segments (path 2, enqueue_segment_k, five launches per layer) on the fast device in the norm-epilogue form, the only form the Q6_K
body is built in.  Everything else keeps the per-op segments (path 0): the strict-order device (there is no ordered Q6_K form),
NO_KQUANT_FUSION, a tensor-parallel rank, a context without the norm epilogue, a classifier whose rhs is not Q8_K, and a Q6_K body
with any layer tensor of another type (no mix recipe has a Q6_K body).  The forms behind the other A/B flags are all built for Q6_K
and stay on path 2 with the plan Q4_K reads under the same flag."""
import os

import numpy as np
import pytest

os.environ["CRABML_HIP_TEST_HOOKS"] = "1"

import crabml_amd as ca  # noqa: E402
from crabml_amd import synth  # noqa: E402
from tests import step_plan_cases as spc  # noqa: E402
from tests import test_q5k_step_plan as P5  # noqa: E402

FORMATS = {"Q6_K": (synth.Q6_K, {}), "Q6_K+Q4_K": (synth.Q6_K, {"output_type": synth.Q4_K}), "Q6_K+Q4_0": (synth.Q6_K, {"output_type": synth.Q4_0}),
           "Q4_K": spc.FORMATS["Q4_K"]}
Q6 = ("Q6_K", "Q6_K+Q4_K")
SHAPES = P5.SHAPES        # tiny-gqa, tiny-hd128, tiny-qwen2, tiny-gemma (whose classifier is the tied embedding: Q6_K under every format)
ALL_SHAPES = P5.ALL_SHAPES  # ... and the head_dim-32 shape none of the Q8_K-producing attention kernels is built for
WORDS = P5.WORDS
PER_OP = (0, 0, 0, 0, 0)


def attn_q_in_q4k(model):
    """a Q6_K body with one layer tensor of another type: layer 0's attn_q in Q4_K"""
    t = model.tensors["blk.0.attn_q.weight"]
    rows, cols = t.shape
    model.tensors["blk.0.attn_q.weight"] = synth.RawTensor(synth.random_blocks(np.random.default_rng(9), rows * cols, synth.Q4_K, 1.0), [rows, cols], synth.Q4_K)
    return model


class Evaluator(P5.Evaluator):
    """the Q5_K file's evaluator over this file's formats and edit"""
    EDITS = {"attn_q_q4k": attn_q_in_q4k}

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


@pytest.mark.parametrize("fmt", Q6)
@pytest.mark.parametrize("shape", SHAPES)
def test_fast_q6k_takes_the_fused_k_segments(ev, shape, fmt):
    """path 2 in the default form: norm epilogue, Q8_K producers, gate | up normalizing wo's row itself; with both caches"""
    assert words(ev.plan(spc.case(shape, fmt))) == (2, 0, 1, 1, 1)
    assert words(ev.plan(spc.case(shape, fmt, kv_f16=False))) == (2, 0, 1, 1, 1)


@pytest.mark.parametrize("fmt", Q6)
@pytest.mark.parametrize("shape", SHAPES)
def test_what_stays_on_the_per_op_segments(ev, shape, fmt):
    assert words(ev.plan(spc.case(shape, fmt, strict=True))) == PER_OP             # no ordered Q6_K form
    assert words(ev.plan(spc.case(shape, fmt, flag="NO_KQUANT_FUSION"))) == PER_OP
    assert words(ev.plan(spc.case(shape, fmt, strict=True, flag="NO_KQUANT_FUSION"))) == PER_OP
    # the one form Q6_K is not built in: wo / ffn_down without the norm epilogue
    assert words(ev.plan(spc.case(shape, fmt, norm_epilogue=False))) == PER_OP


@pytest.mark.parametrize("fmt", Q6)
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128"])
def test_a_tensor_parallel_rank_stays_per_op(ev, shape, fmt):
    for strict in (False, True):
        assert words(ev.plan(spc.case(shape, fmt, strict, flag="TP_DRY_RUN", tp_size=2))) == PER_OP


@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128", "tiny-qwen2"])
def test_a_classifier_whose_rhs_is_not_q8k_stays_per_op(ev, shape):
    """a Q4_0 classifier takes Q8_0 rows: the K-quant norm epilogue leaves Q8_K planes only (Gemma's classifier is its embedding)"""
    assert words(ev.plan(spc.case(shape, "Q6_K+Q4_0"))) == PER_OP


@pytest.mark.parametrize("fmt", Q6)
@pytest.mark.parametrize("shape", SHAPES)
def test_a_q6k_body_with_a_tensor_of_another_type_stays_per_op(ev, shape, fmt):
    assert words(ev.plan(spc.case(shape, fmt, edit="attn_q_q4k"))) == PER_OP


@pytest.mark.parametrize("flag", ["NO_RHS_PROLOGUE", "NO_Q8K_PRODUCERS", "NO_K_NORM_IN", "SPLIT_CHUNKS_ALWAYS", "SPLIT_CHUNKS_NEVER"])
@pytest.mark.parametrize("fmt", Q6)
def test_the_flag_forms_are_built_and_read_as_q4k_does(ev, fmt, flag):
    """every A/B form of the norm-epilogue step exists for the Q6_K body: the whole plan of the Q4_K case of the same flag"""
    for shape in SHAPES:
        got, want = ev.plan(spc.case(shape, fmt, flag=flag)), ev.plan(spc.case(shape, "Q4_K", flag=flag))
        assert got["path"] == 2 and got == want, (shape, got, want)


def test_a_shape_whose_head_dim_has_no_producer(ev):
    """q8k_producers off by shape (head_dim 32 is none of 64 / 128 / 256): still path 2, planes out of wo"""
    assert words(ev.plan(spc.case("q5k-hd32", "Q6_K"))) == (2, 0, 1, 0, 0)
