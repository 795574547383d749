#!/usr/bin/env python3
"""Prompt-processing throughput of the batched prefill (crabml_hip_llama_prefill) against the token loop.
usage: prefill_bench.py [--model llama3-8b] [--wtype Q4_0] [--n 512] [--chunks 64,128,256,512] [--layers N]
--wtype: a name of synth.TYPE_BY_NAME or a recipe: Q4_K_M, Q5_K_M, Q3_K_S, Q3_K_M, Q3_K_L, Q2_K_MIX (llama.cpp's "Q2_K" file type), Q2_K_S.
--flags 536870912 (CRABML_HIP_LLAMA_PREFILL_Q5K_GEMM): the Q5_K matrices of Q5_K, Q5_K_M, Q3_K_M, Q3_K_L on the f16 GEMM (opt-in).
Prints one line per chunk size: prompt tokens/s (host clock around the blocking call, 2nd of 2 runs) and the int8
MFMA rate the weight GEMMs reach (2 * m * k ops per prompt row and weight element)."""
import argparse
import sys
import time

sys.path.insert(0, ".")
import crabml_amd as ca
from crabml_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="llama3-8b")
ap.add_argument("--wtype", default="Q4_0")
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--chunks", default="64,128,256,512")
ap.add_argument("--layers", type=int, default=0)
ap.add_argument("--loop", type=int, default=64, help="tokens of the token-loop baseline")
ap.add_argument("--flags", type=int, default=0, help="extra CRABML_HIP_LLAMA_* flags (A/B runs)")
a = ap.parse_args()
shape = synth.SHAPES[a.model]
wt = a.wtype.upper()
k_m = wt in ("Q4_K_M", "Q5_K_M")  # llama.cpp's mixes: Q4_K / Q5_K body, attn_v / ffn_down in Q6_K on some layers, Q6_K classifier
q3 = wt[5:] if wt in ("Q3_K_S", "Q3_K_M", "Q3_K_L") else None  # the Q3_K recipes (synth.q3_k_mix_types), named as tools/generate.py --synth names them
q2 = {"Q2_K_MIX": "K", "Q2_K_S": "S"}.get(wt)  # the Q2_K recipes (synth.q2_k_mix_types; plain Q2_K: every matrix Q2_K)
model = synth.build_model(shape, synth.TYPE_BY_NAME[wt[:4]] if k_m or q3 or q2 else synth.TYPE_BY_NAME[a.wtype], seed=8, n_layers=a.layers or None,
                          k_m_mix=k_m, q3_k_mix=q3, q2_k_mix=q2)
dev = ca.HipTensorDevice(0)
conf, w = synth.to_hip(model, dev)
L = a.layers or shape.n_layers
hd = shape.dim // shape.n_heads
ops_per_row = 2.0 * L * (shape.dim * shape.dim * 2 + 2 * shape.dim * hd * shape.n_kv_heads + 3 * shape.dim * shape.hidden)
toks = [(7 * i + 1) % shape.vocab for i in range(a.n)]
for chunk in [int(c) for c in a.chunks.split(",")]:
    r = ca.HipLlamaRunner(conf, w, dev, a.n + 8, True, prefill_chunk=chunk, extra_flags=a.flags)
    best = None
    for rep in range(2):
        r.reset()
        dev.sync()
        t0 = time.perf_counter()
        r.prefill(toks)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    print(f"prefill n={a.n} chunk={chunk:4d}: {best * 1e3:8.2f} ms  {a.n / best:9.0f} prompt tok/s  "
          f"{ops_per_row * a.n / best / 1e12:6.1f} TOP/s in the weight GEMMs", flush=True)
    del r
r = ca.HipLlamaRunner(conf, w, dev, a.n + 8, True)
r.forward(toks[0], 0)
dev.sync()
t0 = time.perf_counter()
for i in range(1, a.loop):
    r.forward_async(toks[i], i)
dev.sync()
dt = time.perf_counter() - t0
print(f"token loop ({a.loop - 1} forwards): {dt / (a.loop - 1) * 1e3:.3f} ms/token  {(a.loop - 1) / dt:.0f} prompt tok/s")
