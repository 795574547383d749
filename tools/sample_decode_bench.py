#!/usr/bin/env python3
"""Decode rate with the CLI's default sampler (crabml-cli main.rs:39-44: --temperature 1.0 --probability 0.9) at the 8B shape,
three ways on one context each:
  greedy        crabml_hip_llama_decode_greedy (arg-max on the device)
  sample        crabml_hip_llama_decode_sample(T, topp) (sampler.hpp on the device)
  host_sample   crabml_hip_llama_forward (logits to the host) + Llama2Sampler in C++ per token (host/llama2_runner.hpp)
for the fast and the strict-order device.  Prints one JSON line per (wtype, device).
usage: python tools/sample_decode_bench.py [--wtypes Q4_0,Q4_K] [--steps 128] [--layers N] [--devices fast,strict]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crabml_amd as ca  # noqa: E402
from crabml_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="llama3-8b")
ap.add_argument("--wtypes", default="Q4_0,Q4_K")
ap.add_argument("--devices", default="fast,strict")
ap.add_argument("--layers", type=int, default=None)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--temperature", type=float, default=1.0)
ap.add_argument("--topp", type=float, default=0.9)
ap.add_argument("--reps", type=int, default=3, help="best of this many timed runs per mode")
a = ap.parse_args()

W = 8  # warm-up tokens (graph capture on first use)
coins = np.random.default_rng(0).random(a.steps + W, dtype=np.float32)
for wt in a.wtypes.split(","):
    model = synth.build_model(synth.SHAPES[a.model], synth.TYPE_BY_NAME[wt], seed=8, n_layers=a.layers)
    for kind in a.devices.split(","):
        dev = ca.HipTensorDevice(0, False, 0, kind == "strict")
        conf, w = synth.to_hip(model, dev)
        seq = a.reps * (a.steps + W) + 8
        res = {"model": a.model, "wtype": wt, "layers": a.layers or synth.SHAPES[a.model].n_layers, "device": kind, "steps": a.steps,
               "temperature": a.temperature, "topp": a.topp}
        for mode in ("greedy", "sample", "host_sample"):
            r = ca.HipLlamaRunner(conf, w, dev, seq, True)
            best, host_frac = 0.0, None
            tok = 1
            for _ in range(a.reps):
                if mode == "greedy":
                    tok = r.decode_greedy(tok, W)[-1]
                    dev.sync()
                    t0 = time.perf_counter()
                    ids = r.decode_greedy(tok, a.steps)
                    dt = time.perf_counter() - t0
                elif mode == "sample":
                    tok = r.decode_sample(tok, W, a.temperature, a.topp, coins[:W])[-1]
                    dev.sync()
                    t0 = time.perf_counter()
                    ids = r.decode_sample(tok, a.steps, a.temperature, a.topp, coins[W:])
                    dt = time.perf_counter() - t0
                else:
                    ids, _, _ = r.timed_decode_host_sample(tok, a.temperature, a.topp, coins[:W])
                    tok = ids[-1]
                    ids, dt, hs = r.timed_decode_host_sample(tok, a.temperature, a.topp, coins[W:])
                    host_frac = hs / dt
                tok = ids[-1]
                best = max(best, a.steps / dt)
            res[mode + "_tok_s"] = round(best, 1)
            if host_frac is not None:
                res["host_sampler_share"] = round(host_frac, 3)
            del r
        res["sample_vs_greedy"] = round(res["sample_tok_s"] / res["greedy_tok_s"], 4)
        res["sample_vs_host_sample"] = round(res["sample_tok_s"] / res["host_sample_tok_s"], 3)
        print(json.dumps(res), flush=True)
        del w, conf, dev
