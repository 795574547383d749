#!/usr/bin/env python3
"""Prompt passes of 2..15 rows: the skinny GEMM (gemm_skinny.hip) against one GEMV per row (the A/B hook CRABML_HIP_NO_SKINNY_GEMM).
usage: skinny_bench.py [--model llama3-8b] [--wtype Q4_0 | Q8_0 | Q4_K | Q6_K | Q4_K_M] [--layers 8] [--rows 2,4,8,12,15] [--deep 1024] [--reps 9] [--rounds 3]
Every configuration runs in a child process of its own and the two configurations alternate, `rounds` times each.  A child times
each pass with the host clock around the blocking call (crabml_hip_llama_prefill returns the last row's logits), `reps` times after
two warm-up passes, at cache depth 0 and at depth `deep`, and one decode step beside them.  Prints one JSON line per child and a
summary: median and range over all of a configuration's samples, and the layer weight bytes over the median pass time."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="llama3-8b")
ap.add_argument("--wtype", default="Q4_0")
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--rows", default="2,4,8,12,15")
ap.add_argument("--deep", type=int, default=1024)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--child", action="store_true")
a = ap.parse_args()
rows = [int(x) for x in a.rows.split(",")]


def child():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import crabml_amd as ca
    from crabml_amd import synth

    shape = synth.SHAPES[a.model]
    k_m = a.wtype.upper() == "Q4_K_M"  # llama.cpp's mix: Q4_K body, attn_v / ffn_down in Q6_K on some layers
    model = synth.build_model(shape, synth.TYPE_BY_NAME["Q4_K" if k_m else a.wtype], seed=8, n_layers=a.layers, k_m_mix=k_m)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    wbytes = sum(t.data.nbytes for n, t in model.tensors.items() if n.startswith("blk.") and len(t.shape) == 2)
    toks = [(7 * i + 1) % shape.vocab for i in range(a.deep + 32 + a.reps)]
    r = ca.HipLlamaRunner(conf, w, dev, a.deep + 48 + a.reps, True)
    out = {"layer_weight_bytes": wbytes, "pass_ms": {}}
    for depth in (0, a.deep):
        for b in rows:
            ts = []
            for rep in range(a.reps + 2):
                r.reset()
                if depth:
                    r.prefill(toks[:depth])
                dev.sync()
                t0 = time.perf_counter()
                r.prefill(toks[depth:depth + b])
                ts.append((time.perf_counter() - t0) * 1e3)
            out["pass_ms"][f"{depth}/{b}"] = ts[2:]
    r.reset()
    r.prefill(toks[:16])
    ts = []
    for i in range(16, 16 + a.reps + 2):
        dev.sync()
        t0 = time.perf_counter()
        r.forward(toks[i], i)
        ts.append((time.perf_counter() - t0) * 1e3)
    out["decode_ms"] = ts[2:]
    print(json.dumps(out), flush=True)


if a.child:
    child()
    sys.exit(0)

samples = {"skinny": [], "rows": []}
for rnd in range(a.rounds):
    for cfg in ("skinny", "rows"):
        env = dict(os.environ)
        if cfg == "rows":
            env.update(CRABML_HIP_TEST_HOOKS="1", CRABML_HIP_NO_SKINNY_GEMM="1")
        p = subprocess.run([sys.executable, __file__, "--child"] + [x for x in sys.argv[1:] if x != "--child"], env=env, capture_output=True,
                           text=True, timeout=600)
        if p.returncode != 0:
            sys.exit(f"child {cfg} failed ({p.returncode}):\n{p.stderr[-2000:]}")
        line = p.stdout.strip().splitlines()[-1]
        print(cfg, line, flush=True)
        samples[cfg].append(json.loads(line))


def stat(v):
    return f"{statistics.median(v):7.3f} [{min(v):7.3f}, {max(v):7.3f}]"


wb = samples["skinny"][0]["layer_weight_bytes"]
print(f"{a.model} {a.wtype}, {a.layers} layers ({wb / 1e9:.3f} GB of layer matrices); ms per pass: median [min, max]")
for key in samples["skinny"][0]["pass_ms"]:
    s = [t for c in samples["skinny"] for t in c["pass_ms"][key]]
    g = [t for c in samples["rows"] for t in c["pass_ms"][key]]
    ms, mg = statistics.median(s), statistics.median(g)
    print(f"depth/rows {key:>8}: skinny {stat(s)}  ({wb / ms / 1e9:5.2f} TB/s of layer weights)   row GEMVs {stat(g)}   x{mg / ms:.2f}"
          f"   ranges {'clear' if max(s) < min(g) else 'OVERLAP'}")
print("decode step: skinny-build " + stat([t for c in samples["skinny"] for t in c["decode_ms"]]) + "   hook set " +
      stat([t for c in samples["rows"] for t in c["decode_ms"]]))
