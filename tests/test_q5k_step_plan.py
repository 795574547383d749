"""Which launches a Q5_K decode context runs, on the record-only test device (tests/test_step_plan.py's device and read-out, through
tests/step_plan_cases.case / Evaluator with this file's own formats): a Q5_K body -- plain, llama.cpp's Q5_K_M recipe (attn_v /
ffn_down in Q6_K on the use_more_bits layers, a Q6_K classifier), and Q5_K layers in front of a Q6_K classifier -- takes the K-quant
fused segments (path 2, enqueue_segment_k, five launches per layer) on the fast device in the norm-epilogue form, the only form the
Q5_K body is built in.  Everything else keeps the per-op segments (path 0): the strict-order device (there is no ordered Q5_K
form), NO_KQUANT_FUSION, a tensor-parallel rank, a mix that is not the recipe, and a context without the norm epilogue.  The forms
behind the other A/B flags are all built for Q5_K and stay on path 2 with the words Q4_K reads under the same flag."""
import os

import numpy as np
import pytest

os.environ["CRABML_HIP_TEST_HOOKS"] = "1"

import crabml_amd as ca  # noqa: E402
from crabml_amd import synth, tp  # noqa: E402
from tests import step_plan_cases as spc  # noqa: E402

FORMATS = {"Q5_K": (synth.Q5_K, {}), "Q5_K_M": (synth.Q5_K, {"k_m_mix": True}), "Q5_K+Q6_K": (synth.Q5_K, {"output_type": synth.Q6_K}),
           "Q4_K": spc.FORMATS["Q4_K"], "Q4_K_M": spc.FORMATS["Q4_K_M"]}
Q5 = ("Q5_K", "Q5_K_M", "Q5_K+Q6_K")
SHAPES = ("tiny-gqa", "tiny-hd128", "tiny-qwen2", "tiny-gemma")
# ... and one whose head_dim (32) none of the Q8_K-producing attention kernels is built for
ALL_SHAPES = dict(spc.SHAPES, **{"q5k-hd32": synth.ModelShape("q5k-hd32", 512, 1024, 2, 16, 4, 1024, 64, 1e-5, None)})
WORDS = ("path", "ordered", "norm_epi_k", "q8k_producers", "k_norm_in")


def attn_q_in_q6k(model):
    """a deviation that is not the recipe: layer 0's attn_q in Q6_K"""
    t = model.tensors["blk.0.attn_q.weight"]
    rows, cols = t.shape
    model.tensors["blk.0.attn_q.weight"] = synth.RawTensor(synth.random_blocks(np.random.default_rng(9), rows * cols, synth.Q6_K, 1.0), [rows, cols], synth.Q6_K)
    return model


class Evaluator(spc.Evaluator):
    """spc.Evaluator over this file's FORMATS; `edit` (a case keyword that never reaches create) names a change to the built model"""
    EDITS = {"attn_q_q6k": attn_q_in_q6k}

    def plan(self, c):
        kw = dict(c["kw"])
        edit = kw.pop("edit", None)
        if c["strict"] not in self.devs:
            self.devs[c["strict"]] = self.ca.HipTensorDevice(0, False, 0, c["strict"], self.mode)
        dev = self.devs[c["strict"]]
        ranks = kw.get("tp_size", 1)
        mk = (c["shape"], c["fmt"], ranks, c["kv_f16"] or ranks == 1, edit)
        if mk not in self.models:
            wtype, mkw = FORMATS[c["fmt"]]
            model = synth.build_model(ALL_SHAPES[c["shape"]], wtype, seed=3, **mkw)
            if edit:
                model = self.EDITS[edit](model)
            try:
                model = tp.shard_model(model, ranks, 0, c["kv_f16"])
            except ValueError:
                pass
            self.models[mk] = model
        if mk + (c["strict"],) not in self.hip:
            self.hip[mk + (c["strict"],)] = synth.to_hip(self.models[mk], dev)
        conf, w = self.hip[mk + (c["strict"],)]
        flags = sum(spc.FLAGS[f] for f in c["flag"].split("+")) if c["flag"] else 0
        try:
            return self.ca.debug_step_plan(conf, w, dev, c["seq_len"], c["kv_f16"], extra_flags=flags, **kw)
        except self.ca.CrabmlError as e:
            return {"error": str(e)}


@pytest.fixture(scope="module")
def ev():
    return Evaluator(ca, "dry")


def words(plan):
    assert "error" not in plan, plan
    return tuple(plan[w] for w in WORDS)


@pytest.mark.parametrize("fmt", Q5)
@pytest.mark.parametrize("shape", SHAPES)
def test_fast_q5k_takes_the_fused_k_segments(ev, shape, fmt):
    """path 2 in the default form: norm epilogue, Q8_K producers, gate | up normalizing wo's row itself"""
    assert words(ev.plan(spc.case(shape, fmt))) == (2, 0, 1, 1, 1)
    assert words(ev.plan(spc.case(shape, fmt, kv_f16=False))) == (2, 0, 1, 1, 1)


@pytest.mark.parametrize("fmt", Q5)
@pytest.mark.parametrize("shape", SHAPES)
def test_what_stays_on_the_per_op_segments(ev, shape, fmt):
    assert words(ev.plan(spc.case(shape, fmt, strict=True))) == (0, 0, 0, 0, 0)             # no ordered Q5_K form
    assert words(ev.plan(spc.case(shape, fmt, flag="NO_KQUANT_FUSION"))) == (0, 0, 0, 0, 0)
    assert words(ev.plan(spc.case(shape, fmt, strict=True, flag="NO_KQUANT_FUSION"))) == (0, 0, 0, 0, 0)
    # the one form Q5_K is not built in: wo / ffn_down without the norm epilogue (Q4_K runs k_gemv_res<Q4_K> there, still path 2)
    assert words(ev.plan(spc.case(shape, fmt, norm_epilogue=False))) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("fmt", Q5)
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128"])
def test_a_tensor_parallel_rank_stays_per_op(ev, shape, fmt):
    for strict in (False, True):
        assert words(ev.plan(spc.case(shape, fmt, strict, flag="TP_DRY_RUN", tp_size=2))) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("shape", SHAPES)
def test_a_mix_that_is_not_the_recipe_stays_per_op(ev, shape):
    for fmt in ("Q5_K", "Q5_K_M"):
        assert words(ev.plan(spc.case(shape, fmt, edit="attn_q_q6k"))) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("flag", ["NO_RHS_PROLOGUE", "NO_Q8K_PRODUCERS", "NO_K_NORM_IN", "SPLIT_CHUNKS_ALWAYS", "SPLIT_CHUNKS_NEVER"])
@pytest.mark.parametrize("fmt", Q5)
def test_the_flag_forms_are_built_and_read_as_q4k_does(ev, fmt, flag):
    """every A/B form of the norm-epilogue step exists for the Q5_K body: the same words as the Q4_K case of the same flag"""
    twin = {"Q5_K": "Q4_K", "Q5_K_M": "Q4_K_M", "Q5_K+Q6_K": "Q4_K"}[fmt]
    for shape in SHAPES:
        got, want = ev.plan(spc.case(shape, fmt, flag=flag)), ev.plan(spc.case(shape, twin, flag=flag))
        assert got["path"] == 2 and got == want, (shape, got, want)


def test_a_shape_whose_head_dim_has_no_producer(ev):
    """q8k_producers off by shape (head_dim 32 is none of 64 / 128 / 256): still path 2, planes out of wo"""
    assert words(ev.plan(spc.case("q5k-hd32", "Q5_K"))) == (2, 0, 1, 0, 0)
