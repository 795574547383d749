"""Gemma on the fused decode step against the unchanged runner and the per-op device, in one process (synthetic weights, f16 cache).
Usage: python tools/gemma_bench.py [--runs gemma-2b:Q8_0,gemma-2b:Q4_0] [--reps 5] [--sweep] [--json out.json]

Per SHAPE:FORMAT one markdown table row; every decode figure is tok/s of a window that ends in a device synchronise, the MEDIAN of
--reps repeats after a warm-up of the same window, with (min .. max) behind it:
  fused      (i) crabml_hip_llama_decode_greedy over positions 0..127
  @1024      the same over positions 1024..1087, behind a 1024-token prompt pass; `exact`: the same window on a
  @4096      CRABML_HIP_LLAMA_EXACT_ATTENTION context (the exact long-context chain that k_attn_flash<., 256> replaces) -- the two are
             measured alternately, repeat by repeat
  unchanged  (ii) Llama2Runner<HipTensor>::forward + host arg-max per token (the recorded calls served by the fused step), 64 tokens
  per-op     (iii) the same runner -- the forward_gemma mirror -- on a CRABML_HIP_FLAG_PER_OP device: one launch per Tensor call, only
             kernels that existed before the Gemma decode step did.  The baseline: nothing else could run the model.  16 tokens
  prompt     prefill tok/s of 512 rows
--sweep: the crossover of the split-KV kernel against the staged one-workgroup-per-head kernel at this geometry -- 16 decode steps
from each start position with attn_long_from = 1 (k_attn_flash from the first position) and = seq_len (never), alternately."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import crabml_amd as ca  # noqa: E402
from crabml_amd import synth  # noqa: E402

EXACT_ATTENTION = 4194304  # CRABML_HIP_LLAMA_EXACT_ATTENTION (include/crabml_hip.h)


def timed(fn, n):
    t0 = time.perf_counter()
    fn()  # (decode_greedy / prefill / export return after a device synchronise)
    return n / (time.perf_counter() - t0)


def stats(v):
    v = sorted(v)
    return {"median": float(np.median(v)), "min": v[0], "max": v[-1]}


def fmt_stat(s):
    return "%.1f (%.1f .. %.1f)" % (s["median"], s["min"], s["max"])


def runner_rate(model, mode, n, reps):
    dev = ca.HipTensorDevice(0, False, 0, False, mode)
    conf, w = synth.to_hip(model, dev)
    r = ca.Llama2Runner(conf, w, dev, 8 + (reps + 1) * n, True)
    pos = [0]

    def loop(k):
        tok = 1
        for _ in range(k):
            tok = int(ca.sample_argmax(np.asarray(r.forward([tok], pos[0]))))
            pos[0] += 1

    loop(4)  # warm-up (the unchanged runner learns its decode context from the first token)
    return stats([timed(lambda: loop(n), n) for _ in range(reps)])


def decode_window(r, prompt, n, reps):
    """tok/s of n greedy steps behind `prompt` (already cached positions), repeated: the cache is rewound by a fresh prompt pass"""
    out = []
    for rep in range(reps + 1):
        r.reset()
        if prompt:
            r.prefill(prompt)
        v = timed(lambda: r.decode_greedy(1, n), n)
        if rep:  # (the first window is the warm-up)
            out.append(v)
    return out


def row(spec, reps):
    shape, fmt = spec.split(":")
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=1)
    out = {"GB": model.gemv_weight_bytes_per_token() / 1e9}
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    cap = 4096 + 64 + 16
    r = ca.HipLlamaRunner(conf, w, dev, cap, True)
    e = ca.HipLlamaRunner(conf, w, dev, cap, True, extra_flags=EXACT_ATTENTION)
    out["fused"] = stats(decode_window(r, [], 128, reps))
    prompt = [(11 * i + 5) % conf.vocab_size for i in range(4096)]
    r.reset()
    r.prefill(prompt[:512])
    pr = []
    for _ in range(reps):
        r.reset()
        pr.append(timed(lambda: r.prefill(prompt[:512]), 512))
    out["prompt"] = stats(pr)
    for p in (1024, 4096):
        a, b = [], []
        for rep in range(reps + 1):  # alternately: flash, exact
            for ctx, acc in ((r, a), (e, b)):
                ctx.reset()
                ctx.prefill(prompt[:p])
                v = timed(lambda: ctx.decode_greedy(1, 64), 64)
                if rep:
                    acc.append(v)
        out["@%d" % p], out["@%d exact" % p] = stats(a), stats(b)
    del r, e, w
    out["unchanged"] = runner_rate(model, "lazy", 64, reps)
    out["per-op"] = runner_rate(model, "per-op", 16, reps)
    return shape, fmt, out


def sweep(spec, reps):
    shape, fmt = spec.split(":")
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=1)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    cap = 1024
    fl = ca.HipLlamaRunner(conf, w, dev, cap, True, attn_long_from=1)
    one = ca.HipLlamaRunner(conf, w, dev, cap, True, attn_long_from=cap)
    prompt = [(11 * i + 5) % conf.vocab_size for i in range(cap)]
    print("\n| %s %s: start position | split-KV from position 0, us / step | one workgroup per head, us / step |" % (shape, fmt))
    print("|---|---|---|")
    res = {}
    for p0 in (16, 32, 48, 64, 80, 96, 128, 192, 256, 512):
        a, b = [], []
        for rep in range(reps + 1):
            for ctx, acc in ((fl, a), (one, b)):
                ctx.reset()
                ctx.prefill(prompt[:p0])
                v = timed(lambda: ctx.decode_greedy(1, 16), 16)
                if rep:
                    acc.append(1e6 / v)
        res[p0] = {"flash_us": stats(a), "one_wg_us": stats(b)}
        print("| %d | %s | %s |" % (p0, fmt_stat(stats(a)), fmt_stat(stats(b))), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="gemma-2b:Q8_0,gemma-2b:Q4_0")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    cols = ["fused", "@1024", "@1024 exact", "@4096", "@4096 exact", "unchanged", "per-op", "prompt"]
    print("| shape | format | GB / token | " + " | ".join(cols) + " | fused / per-op |")
    print("|---|---|---|" + "---|" * len(cols) + "---|")
    all_out = {}
    for spec in a.runs.split(","):
        shape, fmt, o = row(spec, a.reps)
        all_out[spec] = o
        print("| %s | %s | %.2f | " % (shape, fmt, o["GB"]) + " | ".join(fmt_stat(o[c]) for c in cols) +
              " | %.2fx |" % (o["fused"]["median"] / o["per-op"]["median"]), flush=True)
    if a.sweep:
        for spec in a.runs.split(","):
            all_out[spec + "/sweep"] = sweep(spec, a.reps)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(all_out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
