"""Contexts of 32768 positions on the fused decode step: decode and prompt rates deep in the cache, against the per-op runner (the
only way a build without them serves such a context) and against a context at the old create-time bound.
Usage: python tools/long_context_bench.py [--runs llama3-8b:Q4_0,llama3-8b:Q4_K,qwen2.5-7b:Q4_0] [--sections decode,prompt,short,memory,baseline]
                                          [--seq-len 32768] [--at 4096,16000,24576,32760] [--baseline-to 32768] [--baseline-budget SECONDS] [--baseline-mode per-op|lazy] [--tree DIR]
Synthetic weights, f16 KV cache, one process.  Per SHAPE:FORMAT, markdown rows:
  decode    crabml_hip_llama_decode_greedy tok/s at each --at position of a --seq-len context (cache filled by prefill; 64 steps, 8 at
            the cache's end; median of 3)
  prompt    prefill tok/s of a prompt of --seq-len tokens (second of two runs)
  short     one 32-row pass at pos0 = 30000 against the same pass at pos0 = 96 (median of 5): the difference is what its attention
            (k_attn_flash_rows: n_heads workgroups walking ~470 tiles each) costs -- the prompt pass's launches carry no event pairs
  memory    crabml_hip_device_mem_in_use before and after the context is created and after its first prompt pass (taken first: the
            pool keeps the blocks that earlier contexts of the process freed)
  baseline  Llama2Runner<HipTensor> on a per-op device (one launch per Tensor call) at --seq-len, token by token from position 0 to
            --baseline-to: tok/s in a 64-token window at each --at position, and over the whole loop (the prompt rate of that path);
            --baseline-mode lazy --tree DIR: the recorded-op queue of the build in DIR (the parent commit: its fallback for such a context)
--tree DIR: import crabml_amd from another checkout (a build of the parent commit) -- with --seq-len 16256 --sections decode the
A/B of the unchanged kernels at 4096 and 16000 positions."""
import argparse
import gc
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def build(ca, synth, spec):
    shape, fmt = spec.split(":")
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=1)
    return shape, fmt, model


def decode_rows(ca, dev, conf, w, seq, at):
    r = ca.HipLlamaRunner(conf, w, dev, seq, True)
    prompt = [(11 * i + 5) % conf.vocab_size for i in range(seq)]
    out = {}
    for pos in at:
        n = min(64, seq - pos)
        rates = []
        for _ in range(3):
            r.reset()
            r.prefill(prompt[:pos])
            dev.sync()
            rates.append(n / timed(lambda: r.decode_greedy(1, n)))
        out[pos] = statistics.median(rates)
    return out


def prompt_rate(ca, dev, conf, w, seq):
    r = ca.HipLlamaRunner(conf, w, dev, seq, True)
    prompt = [(11 * i + 5) % conf.vocab_size for i in range(seq)]
    r.prefill(prompt)
    r.reset()
    dev.sync()
    return seq / timed(lambda: r.prefill(prompt))


def short_pass(ca, dev, conf, w, seq, deep=30000, shallow=96, rows=32):
    r = ca.HipLlamaRunner(conf, w, dev, seq, True)
    prompt = [(11 * i + 5) % conf.vocab_size for i in range(seq)]
    out = {}
    for pos0 in (shallow, deep):
        r.reset()
        r.prefill(prompt[:pos0])
        r.prefill(prompt[pos0:pos0 + rows])  # warm: the pass's buffers and kernels
        ts = []
        for i in range(1, 6):
            dev.sync()
            ts.append(timed(lambda: r.prefill(prompt[pos0 + i * rows:pos0 + (i + 1) * rows])))
        out[pos0] = statistics.median(ts)
    return out[shallow], out[deep]


def memory(ca, dev, conf, w, model, seq):
    gc.collect()
    dev.sync()
    m0 = dev.mem_in_use()
    r = ca.HipLlamaRunner(conf, w, dev, seq, True)
    m1 = dev.mem_in_use()
    r.prefill([(11 * i + 5) % conf.vocab_size for i in range(2048)])
    m2 = dev.mem_in_use()
    s = model.shape
    kv = 2 * s.n_layers * s.n_kv_heads * seq * s.head_dim * 2
    return m0, m1, m2, kv


def baseline(ca, synth, model, seq, at, upto, budget, mode):
    """the per-op runner's token loop from position 0: -> ({pos: tok/s over the 64 tokens from pos}, tok/s of the whole loop, its length);
    budget > 0: the loop ends after that many seconds, the windows it did not reach are left out"""
    import numpy as np
    dev = ca.HipTensorDevice(0, False, 0, False, mode)
    conf, w = synth.to_hip(model, dev)
    r = ca.Llama2Runner(conf, w, dev, seq, True)
    marks, tok = {}, 1
    starts = {p: min(p, upto - 64) for p in at if p < upto and upto >= 64}
    t_all = time.perf_counter()
    for pos in range(upto):
        if budget > 0 and time.perf_counter() - t_all > budget:
            upto = pos
            break
        if pos % 4096 == 0 and pos:
            print("  (per-op token loop at position %d, %.0f s)" % (pos, time.perf_counter() - t_all), file=sys.stderr, flush=True)
        for p, s0 in starts.items():
            if pos == s0:
                marks[p] = [time.perf_counter(), None]
            if pos == s0 + 64:
                marks[p][1] = time.perf_counter()
        tok = int(ca.sample_argmax(np.asarray(r.forward([tok], pos)))) % conf.vocab_size
    t_end = time.perf_counter()
    done = {p: m for p, m in marks.items() if m[1] is not None or starts[p] + 64 == upto}
    for m in done.values():
        m[1] = m[1] or t_end
    return {p: 64 / (b - a) for p, (a, b) in done.items()}, upto / (t_end - t_all), upto


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="llama3-8b:Q4_0,llama3-8b:Q4_K,qwen2.5-7b:Q4_0")
    ap.add_argument("--sections", default="memory,decode,prompt,short")
    ap.add_argument("--seq-len", type=int, default=32768)
    ap.add_argument("--at", default="4096,16000,24576,32760")
    ap.add_argument("--baseline-to", type=int, default=32768)
    ap.add_argument("--baseline-budget", type=float, default=0.0, help="seconds after which the per-op token loop ends (0: never)")
    ap.add_argument("--baseline-mode", default="per-op", choices=["per-op", "lazy"],
                    help="the baseline runner's device: per-op launches, or the recorded-op queue (with --tree: what that build does with such a context)")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import crabml_amd as ca
    from crabml_amd import synth
    seq, sections = a.seq_len, a.sections.split(",")
    at = [int(p) for p in a.at.split(",") if int(p) < seq]
    tag = os.path.basename(os.path.abspath(a.tree))
    for spec in a.runs.split(","):
        shape, fmt, model = build(ca, synth, spec)
        head = "| %s | %s | %s | seq_len %d |" % (tag, shape, fmt, seq)
        dev = ca.HipTensorDevice(0)
        conf, w = synth.to_hip(model, dev)
        if "memory" in sections:  # (first: the pool keeps what earlier contexts of the process freed)
            m0, m1, m2, kv = memory(ca, dev, conf, w, model, seq)
            print(head + " memory | weights %.2f GiB | context +%.2f GiB (KV cache %.2f GiB) | first 2048-token prompt pass +%.2f GiB |"
                  % (m0 / 2**30, (m1 - m0) / 2**30, kv / 2**30, (m2 - m1) / 2**30), flush=True)
        if "decode" in sections:
            d = decode_rows(ca, dev, conf, w, seq, at)
            print(head + " decode tok/s | " + " | ".join("@%d %.1f" % (p, d[p]) for p in at) + " |", flush=True)
        if "prompt" in sections:
            print(head + " prompt of %d tokens | %.0f tok/s |" % (seq, prompt_rate(ca, dev, conf, w, seq)), flush=True)
        if "short" in sections and seq >= 30000 + 6 * 32:
            t0, t1 = short_pass(ca, dev, conf, w, seq)
            print(head + " 32-row pass | at pos0 96: %.2f ms | at pos0 30000: %.2f ms | attention's share at depth %.0f %% |"
                  % (t0 * 1e3, t1 * 1e3, 100 * (t1 - t0) / t1), flush=True)
        del w, dev
        gc.collect()
        if "baseline" in sections:
            b, whole, n = baseline(ca, synth, model, seq, at, a.baseline_to, a.baseline_budget, a.baseline_mode)
            print(head + " %s runner tok/s | " % a.baseline_mode + " | ".join("@%d %.1f" % (p, b[p]) for p in sorted(b)) +
                  " | token loop of %d: %.1f tok/s |" % (n, whole), flush=True)


if __name__ == "__main__":
    main()
