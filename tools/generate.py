#!/usr/bin/env python3
"""Token-id level counterpart of `crabml-cli generate` for the hip backend: load a llama, qwen2 or gemma GGUF file through the C++
loader (crabml_amd/csrc/host/gguf.hpp), prefill a prompt in batched passes, decode on the device: greedily by default, with
Llama2Sampler's temperature / top-p (crabml-llama2/src/sampler.rs) under --temperature > 0 -- the first token from the prompt's
logits on the host (C++ Llama2Sampler), the rest by crabml_hip_llama_decode_sample, coins from a seeded generator.
The tokenizer stays on the reference's side of the boundary (out of scope here), so the prompt is given as token ids.

usage: generate.py model.gguf [--prompt 1,15043,3186] [--steps 64] [--seq-len N] [--f32-kv] [--strict]
                   [--temperature 1.0 --topp 0.9 --seed 0] [--q5k-gemm]
       generate.py --synth tiny-gqa:Q4_K_M   (writes a synthetic file to a temp dir first: a self-contained demo)
       generate.py --synth qwen2.5-7b:Q4_0   (a Qwen2 file: q / k / v biases, NEOX rope)
       generate.py --synth gemma-2b:Q8_0     (a Gemma file: scaled embedding, NEOX rope, GELU, tied classifier)"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crabml_amd as ca
from crabml_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("gguf", nargs="?")
ap.add_argument("--synth", default=None, help="SHAPE:TYPE, e.g. tiny-gqa:Q4_0, llama3-8b:Q4_K_M, llama3-8b:Q5_K_M, llama3-8b:Q6_K, llama3-8b:Q5_0, llama3-8b:Q5_1, llama3-8b:Q3_K_M, llama3-8b:Q2_K, llama3-8b:Q2_K_MIX (llama.cpp's Q2_K recipe), llama3-8b:Q2_K_S, qwen2.5-7b:Q4_0, gemma-2b:Q8_0")
ap.add_argument("--prompt", default="1,365,400,282,7,9,11,13")
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--seq-len", type=int, default=0)
ap.add_argument("--f32-kv", action="store_true")
ap.add_argument("--strict", action="store_true", help="strict-order device: the reference's scalar summation order, bit for bit")
ap.add_argument("--temperature", type=float, default=0.0, help="0 (default): greedy; the CLI's default is 1.0")
ap.add_argument("--topp", type=float, default=0.9)
ap.add_argument("--seed", type=int, default=0, help="seed of the coins (one uniform [0, 1) f32 per token)")
ap.add_argument("--q5k-gemm", action="store_true", help="CRABML_HIP_LLAMA_PREFILL_Q5K_GEMM: prompt passes of 32 rows or more run Q5_K matrices on "
                "the f16 matrix-core GEMM instead of the row-by-row GEMV (opt-in; a stated deviation of the fast tier like the other K-quants')")
a = ap.parse_args()

path = a.gguf
tmp = None
if a.synth:
    shape_name, typ = a.synth.split(":")
    k_m = typ.upper() in ("Q4_K_M", "Q5_K_M")  # llama.cpp's recipes: the body type with attn_v / ffn_down / output.weight in Q6_K
    q3 = typ.upper()[5:] if typ.upper() in ("Q3_K_S", "Q3_K_M", "Q3_K_L") else None  # ... and the Q3_K recipes (synth.q3_k_mix_types)
    q2 = {"Q2_K_MIX": "K", "Q2_K_S": "S"}.get(typ.upper())  # ... and the Q2_K recipes (synth.q2_k_mix_types; plain Q2_K: every matrix Q2_K)
    model = synth.build_model(synth.SHAPES[shape_name], synth.TYPE_BY_NAME[typ.upper()[:4]] if k_m or q3 or q2 else synth.TYPE_BY_NAME[typ], seed=8,
                              k_m_mix=k_m, q3_k_mix=q3, q2_k_mix=q2)
    tmp = tempfile.TemporaryDirectory()
    path = os.path.join(tmp.name, "model.gguf")
    synth.write_gguf(model, path)
if not path:
    ap.error("give a GGUF file or --synth SHAPE:TYPE")

t0 = time.perf_counter()
gf = ca.GGUFFile(path)
conf = gf.load_config()
types = sorted({t[2] for t in gf.tensor_infos()})
print(f"{path}: GGUF v{gf.version}, {len(gf.tensor_infos())} tensors (ggml types {types}), arch {gf.architecture}, "
      f"dim {conf.embedding_dim}, layers {conf.n_layers}, heads {conf.n_heads}/{conf.n_kv_heads}, vocab {conf.vocab_size}")
dev = ca.HipTensorDevice(0, False, 0, a.strict)
weights = gf.load_weights(conf, dev)
dev.sync()
print(f"loaded + uploaded in {time.perf_counter() - t0:.2f} s")
prompt = [int(t) for t in a.prompt.split(",") if t]
seq_len = a.seq_len or min(conf.seq_len, len(prompt) + a.steps + 8)
r = ca.HipLlamaRunner(conf, weights, dev, seq_len, not a.f32_kv, extra_flags=536870912 if a.q5k_gemm else 0)
t0 = time.perf_counter()
logits = r.prefill(prompt)
t_prefill = time.perf_counter() - t0
import numpy as np  # noqa: E402

coins = np.random.default_rng(a.seed).random(max(a.steps, 1), dtype=np.float32)
if a.temperature > 0:
    first = int(ca.sample_llama2(logits, a.temperature, a.topp, float(coins[0])))
else:
    first = int(len(logits) - 1 - logits[::-1].argmax())  # the LAST maximum (sampler.rs:109-116)
t0 = time.perf_counter()
if a.steps <= 1:
    ids = [first]
elif a.temperature > 0:
    ids = [first] + [int(t) for t in r.decode_sample(first, a.steps - 1, a.temperature, a.topp, coins[1:a.steps])]
else:
    ids = [first] + [int(t) for t in r.decode_greedy(first, a.steps - 1)]
t_decode = time.perf_counter() - t0
print(f"prefill: {len(prompt)} tokens in {t_prefill * 1e3:.2f} ms ({len(prompt) / t_prefill:.0f} tok/s)")
if a.steps > 1:
    print(f"decode:  {a.steps - 1} tokens in {t_decode * 1e3:.2f} ms ({(a.steps - 1) / t_decode:.1f} tok/s)")
print("tokens:", ",".join(str(t) for t in ids))
