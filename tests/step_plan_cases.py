"""The case matrix of the step-plan tests (tests/test_step_plan.py on the record-only device, tests/test_hip_step_plan.py on the GPU)
and the one function that evaluates a case.  The expected plans are RECORDS (tests/golden/step_plan_*.json, written by
tools/record_step_plan.py at the commit before the decisions were gathered into decide_step): nothing here restates a rule."""
import json
import os

from crabml_amd import synth, tp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# flag bits of include/crabml_hip.h / crabml_hip_debug.h
FLAGS = {"NO_KQUANT_FUSION": 256, "Q4_1_SEGMENTS": 512, "EXACT_NORM": 8388608, "NO_RHS_PROLOGUE": 1024, "NO_Q8K_PRODUCERS": 32768,
         "NO_K_NORM_IN": 16777216, "SPLIT_CHUNKS_ALWAYS": 16, "SPLIT_CHUNKS_NEVER": 32, "TP_DRY_RUN": 128, "EXACT_ATTENTION": 4194304,
         "NO_LONG_ATTENTION": 64, "NO_STAGED_ATTENTION": 8192, "FLASH_TICKET": 2097152, "NO_PV_PRODUCER_WAVES": 131072,
         "NO_H_CONSUMER_QUANT": 4096}

# a format = (layer type, build_model keywords)
FORMATS = {"Q4_0": (synth.Q4_0, {}), "Q8_0": (synth.Q8_0, {}), "Q4_1": (synth.Q4_1, {}), "Q4_K": (synth.Q4_K, {}),
           "Q4_K_M": (synth.Q4_K, {"k_m_mix": True}), "Q4_0+Q6_K": (synth.Q4_0, {"output_type": synth.Q6_K}),
           "Q4_1+Q6_K": (synth.Q4_1, {"output_type": synth.Q6_K}), "F16": (synth.F16, {}), "F32": (synth.F32, {})}
K_FORMATS = ("Q4_K", "Q4_K_M")
SHAPES = dict(synth.SHAPES)
# one layer whose gate / up rows, halved by tp_size = 2, give one workgroup of 16 rows per compute unit of an MI355X
SHAPES["gu-rows"] = synth.ModelShape("gu-rows", 512, 8192, 1, 8, 2, 1024, 64, 1e-5, None)


def case(shape, fmt, strict=False, kv_f16=True, seq_len=64, flag=None, **kw):
    """one case; its id names everything that differs from the defaults"""
    c = {"shape": shape, "fmt": fmt, "strict": strict, "kv_f16": kv_f16, "seq_len": seq_len, "flag": flag, "kw": kw}
    c["id"] = "/".join([shape, fmt, "strict" if strict else "fast", "kv16" if kv_f16 else "kv32", "seq%d" % seq_len] +
                       ([flag] if flag else []) + ["%s=%s" % kv for kv in sorted(kw.items())])
    return c


def cpu_cases():
    out = []
    shapes = ["tiny-gqa", "tiny-hd128", "15m", "tiny-qwen2", "tiny-gemma"]

    def fmts_of(shape, fmts):  # (dim 288 holds no 256-element super-block: such a tensor cannot even be uploaded)
        return [f for f in fmts if not (shape == "15m" and (f in K_FORMATS or f.endswith("+Q6_K")))]

    for shape in shapes:
        for strict in (False, True):
            for fmt in fmts_of(shape, FORMATS):
                for kv_f16 in (True, False):
                    out.append(case(shape, fmt, strict, kv_f16))
            # every flag on every format it can affect (f16 cache)
            per_flag = [(None, {"norm_epilogue": False}, ["Q4_0", "Q8_0", "Q4_1", "Q4_K", "Q4_K_M", "Q4_0+Q6_K", "Q4_1+Q6_K"]),
                        ("NO_KQUANT_FUSION", {}, ["Q4_1", "Q4_K", "Q4_K_M", "Q4_1+Q6_K"]),
                        ("Q4_1_SEGMENTS", {}, ["Q4_1", "Q4_1+Q6_K"]),
                        ("EXACT_NORM", {}, ["Q4_0", "Q8_0", "Q4_1", "Q4_0+Q6_K"]),
                        ("NO_RHS_PROLOGUE", {}, list(K_FORMATS)),
                        ("NO_Q8K_PRODUCERS", {}, list(K_FORMATS)),
                        ("NO_K_NORM_IN", {}, list(K_FORMATS)),
                        ("SPLIT_CHUNKS_ALWAYS", {}, ["Q4_0", "Q4_1", "Q4_K", "Q4_K_M"]),
                        ("SPLIT_CHUNKS_NEVER", {}, ["Q4_0", "Q4_1", "Q4_K", "Q4_K_M"])]
            for flag, kw, fmts in per_flag:
                for fmt in fmts_of(shape, fmts):
                    out.append(case(shape, fmt, strict, True, flag=flag, **kw))
            if shape in ("tiny-gqa", "tiny-hd128"):  # a lone tensor-parallel rank (the Llama shapes whose halves are whole blocks)
                for fmt in FORMATS:
                    out.append(case(shape, fmt, strict, True, flag="TP_DRY_RUN", tp_size=2))
    # what create refuses is recorded too
    out.append(case("15m", "Q4_0", flag="TP_DRY_RUN", tp_size=2))         # local dim 144
    out.append(case("tiny-gqa", "Q4_0", kv_f16=False, flag="TP_DRY_RUN", tp_size=2))  # GQA shards by heads only with the f16 cache
    return out


def gpu_cases():
    out = []
    for shape in ("tiny-gqa", "tiny-hd128"):
        for fmt in ("Q4_0", "Q4_1"):
            for seq in (64, 320, 1001):
                for kv_f16 in (True, False):
                    out.append(case(shape, fmt, False, kv_f16, seq))
                for flag in ("EXACT_ATTENTION", "NO_LONG_ATTENTION", "NO_STAGED_ATTENTION", "FLASH_TICKET", "NO_PV_PRODUCER_WAVES"):
                    out.append(case(shape, fmt, False, True, seq, flag))
                out.append(case(shape, fmt, False, True, seq, attn_long_from=12))
    for fmt in ("Q4_0", "Q4_K"):
        for seq in (64, 320, 1001):
            out.append(case("tiny-gemma", fmt, False, True, seq))
            out.append(case("tiny-gqa", fmt, True, True, seq))
    out.append(case("gu-rows", "Q4_0", flag="TP_DRY_RUN", tp_size=2))
    out.append(case("gu-rows", "Q4_0", flag="TP_DRY_RUN+NO_H_CONSUMER_QUANT", tp_size=2))
    return out


class Evaluator:
    """evaluates cases on one kind of device, building each model and uploading it to each device once"""

    def __init__(self, ca, mode):
        self.ca, self.mode, self.devs, self.models, self.hip = ca, mode, {}, {}, {}

    def plan(self, c):
        ca = self.ca
        if c["strict"] not in self.devs:
            self.devs[c["strict"]] = ca.HipTensorDevice(0, False, 0, c["strict"], self.mode)
        dev = self.devs[c["strict"]]
        ranks = c["kw"].get("tp_size", 1)
        mk = (c["shape"], c["fmt"], ranks, c["kv_f16"] or ranks == 1)
        if mk not in self.models:
            wtype, kw = FORMATS[c["fmt"]]
            model = synth.build_model(SHAPES[c["shape"]], wtype, seed=3, **kw)
            try:  # rank 0's shard; a shape that cannot be cut goes to create whole, which says why not
                model = tp.shard_model(model, ranks, 0, c["kv_f16"])
            except ValueError:
                pass
            self.models[mk] = model
        if mk + (c["strict"],) not in self.hip:
            self.hip[mk + (c["strict"],)] = synth.to_hip(self.models[mk], dev)
        conf, w = self.hip[mk + (c["strict"],)]
        flags = sum(FLAGS[f] for f in c["flag"].split("+")) if c["flag"] else 0
        try:
            return ca.debug_step_plan(conf, w, dev, c["seq_len"], c["kv_f16"], extra_flags=flags, **c["kw"])
        except ca.CrabmlError as e:
            return {"error": str(e)}


def load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)
