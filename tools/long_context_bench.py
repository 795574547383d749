"""Contexts of 32768 positions on the fused decode step: decode and prompt rates deep in the cache, against the per-op runner (the
only way a build without them serves such a context) and against a context at the old create-time bound.
Usage: python tools/long_context_bench.py [--runs llama3-8b:Q4_0,llama3-8b:Q4_K,qwen2.5-7b:Q4_0] [--sections decode,prompt,short,memory,baseline]
                                          [--seq-len 32768] [--at 4096,16000,24576,32760] [--short-ends 128,512,...] [--baseline-to 32768] [--baseline-budget SECONDS] [--baseline-mode per-op|lazy] [--tree DIR]
Synthetic weights, f16 KV cache, one process.  Per SHAPE:FORMAT, markdown rows:
  decode    crabml_hip_llama_decode_greedy tok/s at each --at position of a --seq-len context (cache filled by prefill; 64 steps, 8 at
            the cache's end; median of 3)
  prompt    prefill tok/s of a prompt of --seq-len tokens (second of two runs)
  short     32-row and 64-row passes that end at each --short-ends position, in a context created with
            CRABML_HIP_LLAMA_NO_FLASH_ROWS_SPLIT (k_attn_flash_rows as one launch: n_heads workgroups walking every tile) and in a default
            context (the split-KV form where flash_rows_slices picks it), alternating pass by pass: median of 5 [min .. max].  The pass
            that ends at 128 is the shallow one: the difference to it is what the attention costs at depth
  memory    crabml_hip_device_mem_in_use before and after the context is created and after its first prompt pass (taken first: the
            pool keeps the blocks that earlier contexts of the process freed)
  baseline  Llama2Runner<HipTensor> on a per-op device (one launch per Tensor call) at --seq-len, token by token from position 0 to
            --baseline-to: tok/s in a 64-token window at each --at position, and over the whole loop (the prompt rate of that path);
            --baseline-mode lazy --tree DIR: the recorded-op queue of the build in DIR (the parent commit: its fallback for such a context)
  kvq8      (not in the default sections) the Q8 KV cache against the f16 one: two contexts alternating run by run -- context bytes,
            decode tok/s at each --at position (median of 3), five 32-row passes from --kvq8-pass-at (median)
  kvq8long  (not in the default sections; --seq-len above 32768) a Q8 context on k_attn_flash<.., KV8> against one on k_attn_flash_mm
            at every --at position, alternating run by run (medians of 3 with ranges), context bytes, prompt tok/s of the whole fill
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


def build(ca, synth, spec, n_layers=None):
    shape, fmt = spec.split(":")
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=1, n_layers=n_layers)
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


NO_FLASH_ROWS_SPLIT = 1073741824  # CRABML_HIP_LLAMA_NO_FLASH_ROWS_SPLIT


def short_pass(ca, dev, conf, w, seq, rows, ends):
    """-> {end: ([seconds, flag set: one launch], [seconds, default: split-KV where flash_rows_slices says so])}: five passes of `rows`
    rows each, the first ending at `end`, the two contexts alternating pass by pass"""
    runners = [ca.HipLlamaRunner(conf, w, dev, seq, True, extra_flags=f) for f in (NO_FLASH_ROWS_SPLIT, 0)]
    prompt = [(11 * i + 5) % conf.vocab_size for i in range(seq)]
    out = {}
    for end in ends:
        pos0 = end - rows
        for r in runners:
            r.reset()
            r.prefill(prompt[:pos0 - rows])
            r.prefill(prompt[pos0 - rows:pos0])  # warm: the pass's buffers and kernels
        ts = ([], [])
        for i in range(5):
            for r, t in zip(runners, ts):
                dev.sync()
                t.append(timed(lambda: r.prefill(prompt[pos0 + i * rows:pos0 + (i + 1) * rows])))
        out[end] = ts
    return out


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


def kv_q8_ab(ca, dev, conf, w, seq, at, pass_at):
    """the Q8 KV cache (use_f16_kv_cache = 2) against the f16 cache, two contexts of one process alternating run by run:
    -> (context bytes {kind: mem_in_use difference}, {pos: {kind: median decode tok/s of 3 runs}}, {kind: median seconds of five 32-row
    passes from pass_at}).  Both caches are filled once, front to back; a run is min(64, (seq - pos) / 3) decode steps, its three
    repetitions at consecutive positions -- at the cache's end the three runs END at seq."""
    runners, mem = {}, {}
    for kind in (1, 2):
        dev.sync()
        m0 = dev.mem_in_use()
        runners[kind] = ca.HipLlamaRunner(conf, w, dev, seq, kind)
        mem[kind] = dev.mem_in_use() - m0
    prompt = [(11 * i + 5) % conf.vocab_size for i in range(seq)]
    filled = 0

    def fill_to(pos):
        nonlocal filled
        for lo in range(filled, pos, 2048):
            for r in runners.values():
                r.prefill(prompt[lo:min(lo + 2048, pos)])
        filled = pos

    rates, passes = {}, {1: [], 2: []}
    for pos in sorted(set(at) | {pass_at}):
        if pos == pass_at and pos + 6 * 32 <= seq:
            fill_to(pos - 32)
            fill_to(pos)  # warm: a 32-row pass's buffers and kernels
            for i in range(5):
                for kind, r in runners.items():
                    dev.sync()
                    passes[kind].append(timed(lambda: r.prefill(prompt[pos + 32 * i:pos + 32 * (i + 1)])))
            filled = pos + 160
        if pos not in at:
            continue
        n = min(64, (seq - pos) // 3)
        fill_to(max(filled, min(pos, seq - 3 * n)))
        rates[pos] = {1: [], 2: []}
        for _ in range(3):
            for kind, r in runners.items():
                dev.sync()
                rates[pos][kind].append(n / timed(lambda: r.decode_greedy(1, n)))
            filled += n
    return mem, {p: {k: statistics.median(v) for k, v in d.items()} for p, d in rates.items()}, {k: statistics.median(v) for k, v in passes.items() if v}


def kv_q8_long_ab(ca, dev, conf, w, seq, at):
    """a Q8 context of more than 32768 positions, k_attn_flash<.., KV8> at every depth (lab hook CRABML_HIP_ATTN_MM_FROM=0) against
    k_attn_flash_mm at every depth (=1): two contexts of one process alternating run by run, both caches filled once, front to back.
    -> (context bytes, prompt tok/s over the whole fill, {pos: {kind: [decode tok/s of 3 runs]}})"""
    os.environ["CRABML_HIP_TEST_HOOKS"] = "1"
    runners = {}
    dev.sync()
    m0 = dev.mem_in_use()
    for kind in ("flash", "mm"):
        os.environ["CRABML_HIP_ATTN_MM_FROM"] = "0" if kind == "flash" else "1"
        runners[kind] = ca.HipLlamaRunner(conf, w, dev, seq, 2)
    mem = (dev.mem_in_use() - m0) // 2
    del os.environ["CRABML_HIP_ATTN_MM_FROM"]
    prompt = [(11 * i + 5) % conf.vocab_size for i in range(seq)]
    filled, fill_s, fill_n, rates = 0, 0.0, 0, {}
    for pos in sorted(at):
        n = min(32, (seq - pos) // 3)
        target = max(filled, min(pos, seq - 3 * n))
        for lo in range(filled, target, 2048):
            runners["flash"].prefill(prompt[lo:min(lo + 2048, target)])
            dev.sync()
            fill_s += timed(lambda: (runners["mm"].prefill(prompt[lo:min(lo + 2048, target)]), dev.sync()))
        fill_n, filled = fill_n + max(0, target - filled), target
        rates[pos] = {"flash": [], "mm": []}
        for _ in range(3):
            for kind, r in runners.items():
                dev.sync()
                rates[pos][kind].append(n / timed(lambda: r.decode_greedy(1, n)))
            filled += n
    return mem, fill_n / fill_s if fill_s else 0.0, rates


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
    ap.add_argument("--short-ends", type=lambda v: [int(x) for x in v.split(",")], default=[128, 512, 1024, 2048, 4096, 8192, 30000],
                    help="the position at which the first of a short leg's five passes ends")
    ap.add_argument("--kvq8-pass-at", type=int, default=30000, help="section kvq8: where its five 32-row passes start")
    ap.add_argument("--baseline-to", type=int, default=32768)
    ap.add_argument("--baseline-budget", type=float, default=0.0, help="seconds after which the per-op token loop ends (0: never)")
    ap.add_argument("--baseline-mode", default="per-op", choices=["per-op", "lazy"],
                    help="the baseline runner's device: per-op launches, or the recorded-op queue (with --tree: what that build does with such a context)")
    ap.add_argument("--layers", type=int, default=0, help="build the shape with this many layers (attention times of a large shape)")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import crabml_amd as ca
    from crabml_amd import synth
    seq, sections = a.seq_len, a.sections.split(",")
    at = [int(p) for p in a.at.split(",") if int(p) < seq]
    tag = os.path.basename(os.path.abspath(a.tree))
    for spec in a.runs.split(","):
        shape, fmt, model = build(ca, synth, spec, a.layers or None)
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
        if "short" in sections:
            s = model.shape
            for rows in (32, 64):
                ends = [e for e in a.short_ends if 2 * rows < e and e + 5 * rows <= seq]
                for end, (off, on) in short_pass(ca, dev, conf, w, seq, rows, ends).items():
                    ms = lambda t: "%.3f ms [%.3f .. %.3f]" % (statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3)  # noqa: E731
                    print(head + " %d-row pass ending at %d | one launch: %s | default (%d slices): %s | one launch / default %.2f |"
                          % (rows, end, ms(off), dev.debug_flash_rows_slices(s.n_heads, s.n_kv_heads, rows, end - rows), ms(on),
                             statistics.median(off) / statistics.median(on)), flush=True)
        if "kvq8" in sections:
            mem, d, p = kv_q8_ab(ca, dev, conf, w, seq, at, a.kvq8_pass_at)
            print(head + " context | f16 cache +%.3f GiB | Q8 cache +%.3f GiB |" % (mem[1] / 2**30, mem[2] / 2**30), flush=True)
            print(head + " decode tok/s, f16 / Q8 cache | " + " | ".join("@%d %.1f / %.1f (x%.3f)" % (q, d[q][1], d[q][2], d[q][2] / d[q][1]) for q in sorted(d)) + " |",
                  flush=True)
            if p:
                print(head + " 32-row pass at %d, f16 / Q8 cache | %.3f ms / %.3f ms |" % (a.kvq8_pass_at, p[1] * 1e3, p[2] * 1e3), flush=True)
        if "kvq8long" in sections:
            mem, prate, d = kv_q8_long_ab(ca, dev, conf, w, seq, at)
            fmt3 = lambda v: "%.1f [%.1f .. %.1f]" % (statistics.median(v), min(v), max(v))  # noqa: E731
            print(head + " Q8 context +%.3f GiB | prompt, whole fill (k_attn_flash_mm context) %.0f tok/s |" % (mem / 2**30, prate), flush=True)
            for q in sorted(d):
                print(head + " decode tok/s @%d | k_attn_flash %s | k_attn_flash_mm %s | x%.3f |"
                      % (q, fmt3(d[q]["flash"]), fmt3(d[q]["mm"]), statistics.median(d[q]["mm"]) / statistics.median(d[q]["flash"])), flush=True)
        del w, dev
        gc.collect()
        if "baseline" in sections:
            b, whole, n = baseline(ca, synth, model, seq, at, a.baseline_to, a.baseline_budget, a.baseline_mode)
            print(head + " %s runner tok/s | " % a.baseline_mode + " | ".join("@%d %.1f" % (p, b[p]) for p in sorted(b)) +
                  " | token loop of %d: %.1f tok/s |" % (n, whole), flush=True)


if __name__ == "__main__":
    main()
