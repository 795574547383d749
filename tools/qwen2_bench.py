"""Qwen2 on the fused decode step against the per-op trait path and Llama-3-8B, in one process.
Usage: python tools/qwen2_bench.py [--runs qwen2.5-7b:Q4_0,qwen2.5-7b:Q4_K_M,llama3-8b:Q4_0,qwen2.5-3b:Q4_0] [--at 1024[,4096...]]
(FORMAT: a name of synth.TYPE_BY_NAME -- llama3-8b:Q6_K, llama3-8b:Q5_K -- or the recipes Q4_K_M / Q5_K_M / Q3_K_S / Q3_K_M / Q3_K_L / Q2_K_MIX (llama.cpp's "Q2_K"
file type; plain Q2_K is every layer matrix in Q2_K) / Q2_K_S)
Per SHAPE:FORMAT (synthetic weights, f16 KV cache), one markdown table row:
  fused      crabml_hip_llama_decode_greedy tok/s over positions 0..127 (best of 3)
  @1024      the same over positions 1024..1087, after a 1024-token prefill (--at POS[,POS...]: one such column per position)
  unchanged  Llama2Runner<HipTensor>::forward + host arg-max per token (the recorded calls served by the fused step), 64 tokens
  per-op     the same runner on a CRABML_HIP_FLAG_PER_OP device (one launch per Tensor call), 16 tokens
  strict     decode_greedy on the strict-order device, positions 0..63
  prompt     prefill tok/s of 512 rows
  GB         weight bytes one decode step streams"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import crabml_amd as ca  # noqa: E402
from crabml_amd import synth  # noqa: E402


def timed(fn, n):
    t0 = time.perf_counter()
    fn()
    return n / (time.perf_counter() - t0)


def runner_rate(model, mode, strict, n):
    dev = ca.HipTensorDevice(0, False, 0, strict, mode)
    conf, w = synth.to_hip(model, dev)
    r = ca.Llama2Runner(conf, w, dev, n + 8, True)

    def loop(p0, k):
        tok = 1
        for i in range(k):
            tok = int(ca.sample_argmax(np.asarray(r.forward([tok], p0 + i))))

    loop(0, 4)  # warm-up (the unchanged runner learns its decode context from the first token)
    return timed(lambda: loop(4, n), n)


def row(spec, steps=128, at=(1024,)):
    shape, fmt = spec.split(":")
    mix = fmt in ("Q4_K_M", "Q5_K_M")
    q3 = fmt[5:] if fmt in ("Q3_K_S", "Q3_K_M", "Q3_K_L") else None
    q2 = {"Q2_K_MIX": "K", "Q2_K_S": "S"}.get(fmt)
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt[:4]] if mix or q3 or q2 else synth.TYPE_BY_NAME[fmt], seed=1, k_m_mix=mix,
                              q3_k_mix=q3, q2_k_mix=q2)
    gb = model.gemv_weight_bytes_per_token() / 1e9
    out = {"GB": gb}
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    r = ca.HipLlamaRunner(conf, w, dev, max(at) + steps + 16, True)
    r.decode_greedy(1, 8)
    best = 0.0
    for _ in range(3):
        r.reset()
        best = max(best, timed(lambda: r.decode_greedy(1, steps), steps))
    out["fused"] = best
    prompt = [(11 * i + 5) % conf.vocab_size for i in range(max(at))]
    r.reset()
    r.prefill(prompt[:512])
    r.reset()
    out["prompt"] = timed(lambda: r.prefill(prompt[:512]), 512)
    for pos in at:
        r.reset()
        r.prefill(prompt[:pos])
        out["@%d" % pos] = timed(lambda: r.decode_greedy(1, 64), 64)
    del r, w
    out["unchanged"] = runner_rate(model, "lazy", False, 64)
    out["per-op"] = runner_rate(model, "per-op", False, 16)
    sdev = ca.HipTensorDevice(0, False, 0, True)
    sconf, sw = synth.to_hip(model, sdev)
    s = ca.HipLlamaRunner(sconf, sw, sdev, 80, True)
    s.decode_greedy(1, 8)
    s.reset()
    out["strict"] = timed(lambda: s.decode_greedy(1, 64), 64)
    return shape, fmt, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="qwen2.5-7b:Q4_0,qwen2.5-7b:Q4_K_M,llama3-8b:Q4_0,qwen2.5-3b:Q4_0")
    ap.add_argument("--at", default="1024", help="cached positions of the long-context column(s), comma-separated")
    a = ap.parse_args()
    at = tuple(int(p) for p in a.at.split(","))
    cols = ["fused"] + ["@%d" % p for p in at] + ["unchanged", "per-op", "strict", "prompt"]
    print("| shape | format | GB / token | " + " | ".join(cols) + " | fused / per-op |")
    print("|---|---|---|" + "---|" * len(cols) + "---|")
    for spec in a.runs.split(","):
        shape, fmt, o = row(spec, at=at)
        print("| %s | %s | %.2f | " % (shape, fmt, o["GB"]) + " | ".join("%.1f" % o[c] for c in cols) +
              " | %.2fx |" % (o["fused"] / o["per-op"]), flush=True)


if __name__ == "__main__":
    main()
