"""Which launches a Q5_0 / Q5_1 decode context runs, on the record-only test device (tests/test_step_plan.py's device and read-out,
through tests/step_plan_cases.case with this file's own formats).  Q5_0 follows Q4_0 and Q5_1 follows Q4_1 in every clause of
decide_step: the five fused launches (path 1) on the fast device, their ordered form on the strict-order device, Q5_0 in front of a
Q6_K classifier still path 1 (the classifier's own rhs is quantized beside the layers'), Q5_1 in front of one the K-quant style
segments (path 2, enqueue_segment_k<Q5_1>).  The one difference: a tensor-parallel rank keeps the per-op segments (path 0) -- none
of the tensor-parallel launch forms is built for the two formats.  Every case compares the WHOLE plan with the twin format's on the
same shape and flags, so nothing here restates a rule that the twin's records (tests/golden/step_plan_*.json) already hold."""
import os

import pytest

os.environ["CRABML_HIP_TEST_HOOKS"] = "1"

import crabml_amd as ca  # noqa: E402
from crabml_amd import synth, tp  # noqa: E402
from tests import step_plan_cases as spc  # noqa: E402

FORMATS = dict(spc.FORMATS, **{"Q5_0": (synth.Q5_0, {}), "Q5_1": (synth.Q5_1, {}), "Q5_0+Q6_K": (synth.Q5_0, {"output_type": synth.Q6_K}),
                               "Q5_1+Q6_K": (synth.Q5_1, {"output_type": synth.Q6_K})})
TWIN = {"Q5_0": "Q4_0", "Q5_1": "Q4_1", "Q5_0+Q6_K": "Q4_0+Q6_K", "Q5_1+Q6_K": "Q4_1+Q6_K"}
SHAPES = ("tiny-gqa", "tiny-hd128", "tiny-qwen2")


class Evaluator(spc.Evaluator):
    """spc.Evaluator over this file's FORMATS"""

    def plan(self, c):
        if c["strict"] not in self.devs:
            self.devs[c["strict"]] = self.ca.HipTensorDevice(0, False, 0, c["strict"], self.mode)
        dev = self.devs[c["strict"]]
        ranks = c["kw"].get("tp_size", 1)
        mk = (c["shape"], c["fmt"], ranks, c["kv_f16"] or ranks == 1)
        if mk not in self.models:
            wtype, mkw = FORMATS[c["fmt"]]
            model = synth.build_model(spc.SHAPES[c["shape"]], wtype, seed=3, **mkw)
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
            return self.ca.debug_step_plan(conf, w, dev, c["seq_len"], c["kv_f16"], extra_flags=flags, **c["kw"])
        except self.ca.CrabmlError as e:
            return {"error": str(e)}


@pytest.fixture(scope="module")
def ev():
    return Evaluator(ca, "dry")


def both(ev, shape, fmt, **kw):
    """the plan of `fmt` and of its twin on the same shape and flags; the two agree in every word"""
    got, want = ev.plan(spc.case(shape, fmt, **kw)), ev.plan(spc.case(shape, TWIN[fmt], **kw))
    assert "error" not in got and "error" not in want, (got, want)
    assert got == want, (shape, fmt, kw, got, want)
    return got


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
@pytest.mark.parametrize("shape", SHAPES)
def test_fast_device_runs_the_five_fused_launches(ev, shape, fmt):
    for kv_f16 in (True, False):
        p = both(ev, shape, fmt, kv_f16=kv_f16)
        assert p["path"] == 1 and p["ordered"] == 0 and p["norm_epi"] == 1
        # the hop-free norm is Q5_0's (as Q4_0's), never Q5_1's (as Q4_1's)
        assert p["defer_norm"] == (1 if fmt == "Q5_0" else 0)


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
@pytest.mark.parametrize("shape", SHAPES)
def test_strict_device_runs_the_ordered_five(ev, shape, fmt):
    p = both(ev, shape, fmt, strict=True)
    assert p["path"] == 1 and p["ordered"] == 1 and p["defer_norm"] == 0


@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128"])
def test_a_q6k_classifier(ev, shape):
    """llama.cpp's Q5_0 / Q5_1 files carry a Q6_K output.weight"""
    assert both(ev, shape, "Q5_0+Q6_K")["path"] == 1
    p = both(ev, shape, "Q5_1+Q6_K")
    assert p["path"] == 2 and p["norm_epi"] == 0
    for fmt in ("Q5_0+Q6_K", "Q5_1+Q6_K"):  # a strict-order device: the classifier's format does not matter to the ordered five
        both(ev, shape, fmt, strict=True)


@pytest.mark.parametrize("flag,kw", [("EXACT_NORM", {}), (None, {"norm_epilogue": False}), ("SPLIT_CHUNKS_ALWAYS", {}),
                                     ("SPLIT_CHUNKS_NEVER", {}), ("NO_KQUANT_FUSION", {}), ("NO_LONG_ATTENTION", {}),
                                     ("EXACT_ATTENTION", {})])
@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1", "Q5_0+Q6_K", "Q5_1+Q6_K"])
def test_the_flag_forms_read_as_the_twin_does(ev, fmt, flag, kw):
    for shape in ("tiny-gqa", "tiny-hd128"):
        for strict in (False, True):
            p = both(ev, shape, fmt, strict=strict, flag=flag, **kw)
            if flag == "EXACT_NORM":
                assert p["defer_norm"] == 0


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
def test_q4_1_segments_is_q4_1s_alone(ev, fmt):
    """the A/B flag that sends a Q4_1 body to the K-quant style segments does nothing to either new format"""
    assert ev.plan(spc.case("tiny-gqa", fmt, flag="Q4_1_SEGMENTS")) == ev.plan(spc.case("tiny-gqa", fmt))
    assert ev.plan(spc.case("tiny-gqa", "Q4_1", flag="Q4_1_SEGMENTS"))["path"] == 2


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1", "Q5_0+Q6_K", "Q5_1+Q6_K"])
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128"])
def test_a_tensor_parallel_rank_stays_per_op(ev, shape, fmt):
    """the one clause in which the two formats leave their twins: path 0, no epilogue, nothing ordered.  The attention words do not
    depend on the weight format and still equal the twin's."""
    for strict in (False, True):
        got = ev.plan(spc.case(shape, fmt, strict, flag="TP_DRY_RUN", tp_size=2))
        want = ev.plan(spc.case(shape, TWIN[fmt], strict, flag="TP_DRY_RUN", tp_size=2))
        assert "error" not in got, got
        assert (got["path"], got["ordered"], got["norm_epi"], got["defer_norm"], got["gu_rows"]) == (0, 0, 0, 0, 0), got
        own = ("path", "ordered", "norm_epi", "defer_norm", "gu_rows", "norm_epi_k")
        assert {k: v for k, v in got.items() if k not in own} == {k: v for k, v in want.items() if k not in own}


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1"])
def test_dim_288(ev, fmt):
    """15m: 9 blocks per row, head_dim 48 -- whatever the twin gets there, on either device"""
    for strict in (False, True):
        for kv_f16 in (True, False):
            both(ev, "15m", fmt, strict=strict, kv_f16=kv_f16)


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1", "Q5_0+Q6_K", "Q5_1+Q6_K"])
def test_a_long_context_is_a_plan(ev, fmt):
    """20000 positions on tiny-hd128.  The record-only device cannot raise a kernel's LDS limit, so it has no long-context attention
    for ANY format and refuses such a cache with that reason: what is held here is that the two formats get the twin's answer word for
    word -- no refusal of their own.  That the answer is a plan on a real device is
    tests/test_hip_q5_01_fused.py::test_a_long_context_is_created."""
    got, want = ev.plan(spc.case("tiny-hd128", fmt, seq_len=20000)), ev.plan(spc.case("tiny-hd128", TWIN[fmt], seq_len=20000))
    assert got == want, (got, want)
    p = both(ev, "tiny-hd128", fmt, seq_len=16000)  # (the longest cache every plan serves)
    assert p["path"] in (1, 2)


def test_a_mixed_body_keeps_its_path(ev):
    """a Q5_0 body with one tensor in another format of the same rhs: per-op segments, as every 32-element body"""
    import numpy as np
    for own, other in ((synth.Q5_0, synth.Q4_0), (synth.Q5_1, synth.Q4_1)):
        model = synth.build_model(spc.SHAPES["tiny-gqa"], own, seed=3)
        t = model.tensors["blk.0.attn_q.weight"]
        rows, cols = t.shape
        model.tensors["blk.0.attn_q.weight"] = synth.RawTensor(synth.random_blocks(np.random.default_rng(9), rows * cols, other, 1.0),
                                                               [rows, cols], other)
        dev = ca.HipTensorDevice(0, False, 0, False, "dry")
        conf, w = synth.to_hip(model, dev)
        assert ca.debug_step_plan(conf, w, dev, 64, True)["path"] == 0
