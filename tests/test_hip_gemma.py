"""GPU parity of the Gemma decode step (crabml_hip_llama_create_arch with CRABML_HIP_ARCH_GEMMA: the embedded row times sqrtf(dim),
the q|k|v kernels' QKV_GEMMA form -- NEOX row pairs, no bias --, h = gelu(g) * u through the reference's f16 table in every gate | up
kernel) against tests/gemma_ref.py, the restatement of Llama2Runner<CpuTensor>::forward_gemma (llama2.rs:455-524), and of the
split-KV decode attention at head_dim 256 (k_attn_flash<G, 256, ..>), the geometry of Gemma-2B's multi-query attention.

  * strict-order device: logits AND KV-cache bytes bit-identical to the restatement at every step, on every kernel form (ordered
    fused launches, K-quant segments, per-op segments), graph replay and eager launches;
  * fast device: within the per-format FAST_TOL of the restatement and of the per-op trait path;
  * every launch of the fast step against float64 (tests/gemma_step_ref.py through the tap recorder), across attn_long_from;
  * k_attn_flash at head_dim 256 by itself against float64 on the same f16 inputs;
  * the prompt pass, the device samplers, the unchanged runner, the create-time answers, and two layers of the Gemma-2B shape."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests import gemma_step_ref as G
from tests.gemma_ref import FAST_Q4_K_SEEDS, FAST_TOKS, OracleGemmaRunner, to_oracle_gemma
from tests.helpers import EXACT_NORM, FAST_TOL, check_fast, record_observed
from tests.sampler_ref import sample as sampler_ref_sample
from tests.test_hip_flash_attention import run_case as flash_case

pytestmark = pytest.mark.gpu
TOKS = [1, 365, 400, 282, 7, 9, 11]
PREFILL_INT8_GEMM = 524288  # CRABML_HIP_LLAMA_PREFILL_INT8_GEMM (include/crabml_hip_debug.h)
EXACT_ATTENTION = 4194304  # CRABML_HIP_LLAMA_EXACT_ATTENTION (include/crabml_hip.h)
# The repository's convention for a tiny model whose default (hop-free norm) step exceeds its format row of FAST_TOL: a per-model bound
# of 2 x what MI355X shows -- and here never above 2 x what the per-op trait path (old code: the yardstick) shows on the same model and
# tokens, which the test computes and asserts next to the table.  (shape, format) -> (median, max) bound, each entry with the figures
# behind it (fused median / max, trait median / max).  Empty: every model here is held to its format row of FAST_TOL.
GEMMA_TOL_DEFAULT_NORM = {}
_OBSERVED = {}


def shape_of(name, **kw):
    return synth.ModelShape(**{**synth.SHAPES[name].__dict__, **kw})


def restated(model, kv_f16, tokens, seq_len=64):
    odev = o.OracleDevice(thread_num=4)
    r = OracleGemmaRunner(*to_oracle_gemma(model, odev), odev, seq_len, kv_f16)
    return [r.forward([t], i).copy() for i, t in enumerate(tokens)], r


def rel_errs(a, b):
    return np.array([np.max(np.abs(x - y)) / np.max(np.abs(y)) for x, y in zip(a, b)])


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def check_kv(r, orr, s, n, kv_f16, cap=64):
    es = 2 if kv_f16 else 4
    for layer in range(s.n_layers):
        for which, cache in ((False, orr.key_cache), (True, orr.value_cache)):
            got = r.debug_kv(layer, which, kv_f16)
            exp = cache[layer].storage.view(np.uint8)
            for h in range(s.n_kv_heads):
                lo = h * cap * s.head_dim * es
                assert np.array_equal(got[lo:lo + n * s.head_dim * es], exp[lo:lo + n * s.head_dim * es]), (layer, which, h)


STRICT = [("tiny-gemma", "Q4_0", True, {}), ("tiny-gemma", "Q8_0", True, {}), ("tiny-gemma", "Q4_1", True, {}),
          ("tiny-gemma", "Q4_K", True, {}), ("tiny-gemma", "Q4_K_M", True, {}),
          ("tiny-gemma-g8", "Q4_0", True, {}), ("tiny-gemma-g8", "Q4_K", True, {}),
          ("tiny-gemma", "Q4_0", True, {"rope_dim": 128}), ("tiny-gemma", "Q8_0", False, {})]


@pytest.mark.parametrize("shape,fmt,kv_f16,over", STRICT, ids=lambda v: str(v))
def test_gemma_strict_is_bit_exact(ca, shape, fmt, kv_f16, over):
    mix = fmt == "Q4_K_M"
    model = synth.build_model(shape_of(shape, **over), synth.Q4_K if mix else synth.TYPE_BY_NAME[fmt], seed=21, k_m_mix=mix)
    ref, orr = restated(model, kv_f16, TOKS)
    dev = ca.HipTensorDevice(0, False, 0, True)
    conf, w = synth.to_hip(model, dev)
    assert conf.architecture == "gemma"
    for use_graph in (True, False):
        r = ca.HipLlamaRunner(conf, w, dev, 64, kv_f16, use_graph)
        for i, t in enumerate(TOKS):
            assert same_bits(r.forward(t, i), ref[i]), f"graph={use_graph} step {i}"
        check_kv(r, orr, model.shape, len(TOKS), kv_f16)


@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0", "Q4_1", "Q4_K"])
@pytest.mark.parametrize("shape", ["tiny-gemma", "tiny-gemma-g8"])
def test_gemma_fast_matches_restatement_and_trait_path(ca, shape, fmt):
    """The Q4_K models' seeds come from the REFERENCE ALONE (tests/gemma_ref.FAST_Q4_K_SEEDS, pinned without a device by
    tests/test_gemma.py::test_q4_k_fast_path_seeds_are_quiet_in_the_reference): with one kv head every head reads the same f16 cache
    rows, so ONE flipped quant of the round-to-nearest Q8_K quantizer lands in a cache row and moves every later step -- the
    reference itself, its row dots moved by +-1 ulp (what any other order of the block sums does), shows flip-sized steps (4e-3 ..
    1e-2 of max|logit|) on 10-78 % of the steps of most seeds of these two shapes, where FAST_TOL's Q4_K median of 5e-7 assumes that
    flips are rare.  MI355X at seed 22, tiny-gemma-g8: fused and exact-norm median 4.3e-3 / max 6.8e-3 (6 of 10 steps flip-sized: the
    steps at which the perturbed reference flips too), trait path 3.4e-7 / 5.0e-3."""
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=FAST_Q4_K_SEEDS[shape] if fmt == "Q4_K" else 22)
    toks = FAST_TOKS
    assert toks == TOKS + [3, 5, 8]
    ref, _ = restated(model, True, toks)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    fused = ca.HipLlamaRunner(conf, w, dev, 64, True)
    exact = ca.HipLlamaRunner(conf, w, dev, 64, True, extra_flags=EXACT_NORM)
    pdev = ca.HipTensorDevice(0, False, 0, False, "per-op")  # the per-op trait path: one launch per Tensor call
    pconf, pw = synth.to_hip(model, pdev)
    trait = ca.Llama2Runner(pconf, pw, pdev, 64, True)
    lf = [fused.forward(t, i).copy() for i, t in enumerate(toks)]
    le = [exact.forward(t, i).copy() for i, t in enumerate(toks)]
    lt = [trait.forward([t], i).copy() for i, t in enumerate(toks)]
    assert all(np.isfinite(x).all() for x in lf + le + lt)
    ef, ee, et, eft = rel_errs(lf, ref), rel_errs(le, ref), rel_errs(lt, ref), rel_errs(lf, lt)
    print(f"{shape}/{fmt}: fused median {np.median(ef):.3e} max {ef.max():.3e}; exact-norm median {np.median(ee):.3e} max {ee.max():.3e}; "
          f"trait median {np.median(et):.3e} max {et.max():.3e}; fused vs trait max {eft.max():.3e}")
    check_fast(f"gemma-trait/{shape}/{fmt}", fmt, et)
    check_fast(f"gemma-fused-exact-norm/{shape}/{fmt}", fmt, ee)  # held to FAST_TOL with no exception
    if (shape, fmt) in GEMMA_TOL_DEFAULT_NORM:
        med, mx = GEMMA_TOL_DEFAULT_NORM[(shape, fmt)]
        _OBSERVED[f"gemma-fused/{shape}/{fmt}"] = {"median": float(np.median(ef)), "max": float(np.max(ef)), "steps": int(ef.size),
                                                    "bound": [med, mx], "trait_median": float(np.median(et)), "trait_max": float(np.max(et))}
        record_observed(_OBSERVED)
        assert np.median(ef) <= min(med, 2 * np.median(et)) and np.max(ef) <= min(mx, 2 * np.max(et)), (ef, et)
    else:
        check_fast(f"gemma-fused/{shape}/{fmt}", fmt, ef)
    med, mx = FAST_TOL[fmt]
    assert np.max(eft) <= 2 * mx


# ---- every launch of the fast step against float64 ----
def expect_defer(model, n_cu):
    return model.wtype in (synth.Q4_0, synth.Q8_0) and model.shape.dim // 32 <= n_cu


LAUNCH_POSITIONS = [0, 1, 94, 95, 96, 97, 128, 129, 191]  # across attn_long_from = 96; 2 and 3 slices, an odd row count in the last one


@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0"])
@pytest.mark.parametrize("shape", ["tiny-gemma", "tiny-gemma-g8"])
def test_gemma_every_launch_against_float64(ca, shape, fmt):
    """tests/test_hip_fused_launches.run_case with the Gemma reference: a runner is teacher-forced greedily on its own tokens up to
    `pos` (from the graph), then takes ONE tapped step; every launch is compared with the float64 restatement of what it computes from
    the bytes it read.  Layer 1 at every position, layer 0 (the scaled embedding, the norm launch) at 0 and 97.  From 96 cached positions
    the attention is k_attn_flash<G, 256> with the merge inside the launch (held to FLASH_REL of float64 on the same f16 inputs)."""
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=31)
    seq = 256
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    mk = lambda: ca.HipLlamaRunner(conf, w, dev, seq, True)  # noqa: E731
    r, twin = mk(), mk()
    fails, observed = [], {}
    for pos in LAUNCH_POSITIONS:
        twin.reset()
        tok = int(twin.decode_greedy(1, pos)[-1]) if pos else 1
        want = twin.forward(tok, pos).copy()
        for layer in ([0, 1] if pos in (0, 97) else [1]):
            ctx = f"gemma/{shape}/{fmt} layer {layer} pos {pos}"
            r.reset()
            if pos:
                assert int(r.decode_greedy(1, pos)[-1]) == tok, ctx
            tap = r.debug_tap(tok, pos, layer)
            assert r.kv_cache_len() == pos + 1
            plan = tap["plan"]
            defer, flash = plan["defer_norm"] == 1, plan["attn_variant"] >= 16
            assert defer == expect_defer(model, plan["n_cu"]), (ctx, plan)
            assert flash == (pos + 1 >= 96), (ctx, plan)  # head_dim 256, group 2 / 8, f16 cache: the split-KV kernel from attn_long_from on
            if flash:
                assert plan["attn_variant"] == 16 + 2, (ctx, plan)  # below 768 cached positions the merge runs inside the launch
            assert np.array_equal(tap["logits"].view(np.uint32), want.view(np.uint32)), f"{ctx}: the tapped (eager) step's logits differ from the graph's"
            form = R.Form(defer=defer, kv_f16=True, seq_cap=seq, flash_from=pos + 1 if flash else 0)
            kc, vc = r.debug_kv(layer, False, True), r.debug_kv(layer, True, True)
            res = G.check_layer(tap, kc, vc, model, layer, pos, form, ctx, token=tok)
            for name, rr in res.items():
                print(f"{ctx} {name}: error / bound {rr.worst:.3f} excused {rr.excused}")
            observed[f"gemma/{shape}/{fmt}/L{layer}/p{pos}"] = {"error_over_bound": {k: round(v.worst, 4) for k, v in res.items()},
                                                               "excused_share": {k: {n: round(x, 4) for n, x in v.excused.items()} for k, v in res.items() if v.excused}}
            fails += G.failures(res)
    record_observed(observed, "fused_launch_pins.json")
    assert not fails, "\n".join(fails)


# ---- the kernel alone: k_attn_flash<G, 256> against float64 on the same f16 inputs ----
FLASH_TOL_KERNEL = 2e-5  # the kernel's stated tolerance (tests/test_hip_flash_attention.py), not widened for head_dim 256


@pytest.mark.parametrize("n_heads,n_kv,hd", [(8, 1, 256), (2, 1, 256), (4, 4, 256), (8, 2, 256)])
def test_flash_attention_256_equals_float64_arithmetic(ca, n_heads, n_kv, hd):
    """groups 8, 2, 1 and 4 at head_dim 256 (a row = 32 lanes x 16 bytes, two rows per wave instruction): one row, ragged row pairs, the
    slice thresholds, many slices; the ticket form (last arriver merges) bit-identical to the two-launch form (asserted in run_case)"""
    dev = ca.HipTensorDevice(0)
    rng = np.random.default_rng(100 * n_kv + hd + n_heads)
    worst = 0.0
    for seq in (1, 2, 3, 5, 31, 127, 128, 129, 257, 1000, 2049):
        for slices in (1, 7, 32):
            err = flash_case(ca, dev, rng, n_heads, n_kv, hd, seq, slices)
            worst = max(worst, err)
            assert err <= FLASH_TOL_KERNEL, (seq, slices, err)
    print(f"flash vs float64, {n_heads} heads / {n_kv} kv x {hd}: worst {worst:.2e} of max|out|")


@pytest.mark.parametrize("kind", ["spike", "ties", "dead"])
def test_flash_attention_256_merge_edge_cases(ca, kind):
    dev = ca.HipTensorDevice(0)
    rng = np.random.default_rng(7)
    for seq in (130, 513, 3000):
        err = flash_case(ca, dev, rng, 8, 1, 256, seq, 32, spread=4.0, kind=kind)
        assert err <= FLASH_TOL_KERNEL, (kind, seq, err)


def test_gemma_split_kv_attention_end_to_end(ca):
    """the fast step with the switch to k_attn_flash<2, 256> forced to 8 cached positions, 40 positions against the restatement inside
    the FLASH row of FAST_TOL; and the prompt pass of the same tokens (head_dim 256 keeps the exact tile kernel there)"""
    model = synth.build_model(synth.SHAPES["tiny-gemma"], synth.Q4_0, seed=29)
    toks = [(7 * i + 3) % 1000 for i in range(40)]
    ref, _ = restated(model, True, toks, seq_len=48)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    fl = ca.HipLlamaRunner(conf, w, dev, 48, True, attn_long_from=8)
    lf = [fl.forward(t, i).copy() for i, t in enumerate(toks)]
    check_fast("gemma-fused/flash-from-8/tiny-gemma/Q4_0", "FLASH:Q4_0", rel_errs(lf, ref))
    lg = np.array(ca.HipLlamaRunner(conf, w, dev, 48, True, attn_long_from=8).prefill(toks))
    assert np.max(np.abs(lg - ref[-1])) <= FAST_TOL["FLASH:Q4_0"][1] * np.max(np.abs(ref[-1]))


# ---- the other public entries ----
@pytest.mark.parametrize("fmt", ["Q4_0", "Q4_K"])
def test_gemma_prefill(ca, fmt):
    """Strict device: prefill = the token loop bit for bit (logits of the last token, KV bytes) across a chunk boundary.  Fast device:
    the int8 and the f16-weight GEMM passes within the format's bound of the restatement."""
    model = synth.build_model(synth.SHAPES["tiny-gemma"], synth.TYPE_BY_NAME[fmt], seed=23)
    n = 40
    prompt = [(11 * i + 5) % model.shape.vocab for i in range(n)]
    ref, orr = restated(model, True, prompt)
    sdev = ca.HipTensorDevice(0, False, 0, True)
    conf, w = synth.to_hip(model, sdev)
    r = ca.HipLlamaRunner(conf, w, sdev, 64, True, prefill_chunk=24)
    assert same_bits(r.prefill(prompt), ref[-1])
    check_kv(r, orr, model.shape, n, True)
    loop = ca.HipLlamaRunner(conf, w, sdev, 64, True)
    for i, t in enumerate(prompt):
        lg = loop.forward(t, i)
    assert same_bits(lg, ref[-1])
    fdev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, fdev)
    tol = FAST_TOL[fmt][1]
    for flags in (0, PREFILL_INT8_GEMM):
        lg = np.array(ca.HipLlamaRunner(conf, w, fdev, 64, True, prefill_chunk=24, extra_flags=flags).prefill(prompt))
        assert np.isfinite(lg).all()
        err = np.max(np.abs(lg - ref[-1])) / np.max(np.abs(ref[-1]))
        print(f"gemma prefill {fmt} flags {flags}: {err:.3e}")
        assert err <= tol, (flags, err)


def test_gemma_device_samplers(ca):
    model = synth.build_model(synth.SHAPES["tiny-gemma"], synth.Q4_0, seed=24)
    dev = ca.HipTensorDevice(0, False, 0, True)
    conf, w = synth.to_hip(model, dev)
    odev = o.OracleDevice(thread_num=4)
    orr = OracleGemmaRunner(*to_oracle_gemma(model, odev), odev, 64, True)
    for i, t in enumerate(TOKS[:3]):
        orr.forward([t], i)
    ids_ref, tok = [], o.argmax_last(orr.logits)
    for s in range(6):
        ids_ref.append(tok)
        orr.forward([tok], 3 + s)
        tok = o.argmax_last(orr.logits)
    r = ca.HipLlamaRunner(conf, w, dev, 64, True)
    for i, t in enumerate(TOKS[:3]):
        r.forward(t, i)
    assert list(r.decode_greedy(int(ids_ref[0]), 6)) == ids_ref[1:] + [tok]
    coins = [0.13, 0.71, 0.42, 0.95]
    orr2 = OracleGemmaRunner(*to_oracle_gemma(model, odev), odev, 64, True)
    for i, t in enumerate(TOKS[:3]):
        orr2.forward([t], i)
    first = int(o.argmax_last(orr2.logits))
    exp, tok = [], first
    for s, c in enumerate(coins):
        lg = orr2.forward([tok], 3 + s).copy()
        tok = sampler_ref_sample(lg, 0.8, 0.9, c)
        exp.append(tok)
    r2 = ca.HipLlamaRunner(conf, w, dev, 64, True)
    for i, t in enumerate(TOKS[:3]):
        r2.forward(t, i)
    assert list(r2.decode_sample(first, len(coins), 0.8, 0.9, coins)) == exp


def test_gemma_unchanged_runner_equals_per_op(ca):
    """The C++ mirror's forward_gemma over HipTensor (llama2.rs:455-524 op for op) on the strict device equals the restatement and
    the CRABML_HIP_FLAG_PER_OP device bit for bit; the lazy device served every token from the Gemma decode context."""
    model = synth.build_model(synth.SHAPES["tiny-gemma"], synth.Q8_0, seed=25)
    ref, _ = restated(model, True, TOKS[:4])
    for mode in ("lazy", "per-op"):
        dev = ca.HipTensorDevice(0, False, 0, True, mode)
        conf, w = synth.to_hip(model, dev)
        r = ca.Llama2Runner(conf, w, dev, 64, True)
        for i, t in enumerate(TOKS[:4]):
            assert same_bits(r.forward([t], i), ref[i]), (mode, i)
        if mode == "lazy":
            st = dev.lazy_stats()
            assert st["learned"] == 1 and st["fused_tokens"] == 4 and st["replayed"] == 0, st


def test_gemma_create_answers(ca):
    model = synth.build_model(synth.SHAPES["tiny-gemma"], synth.Q4_0, seed=26)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    s = model.shape

    def conf_as(arch):
        return ca.LlamaConfig(embedding_dim=s.dim, hidden_dim=s.hidden, n_layers=s.n_layers, n_heads=s.n_heads,
                              n_kv_heads=s.n_kv_heads, vocab_size=s.vocab, seq_len=s.seq_len, rms_norm_eps=s.rms_eps,
                              rope_dim=s.rope_dim, architecture=arch)

    def kind(e):
        return int(str(e.value).split("ErrorKind(")[1].split(")")[0])

    with pytest.raises(ca.CrabmlError) as e:  # Gemma + tensor parallelism
        ca.HipLlamaRunner(conf, w, dev, 64, True, True, True, 2, 0)
    assert kind(e) == 9  # NotImplemented
    with pytest.raises(ca.CrabmlError) as e:
        ca.HipLlamaRunner(conf_as("phi2"), w, dev, 64, True)
    assert kind(e) == 9
    # Gemma + q / k / v biases: there is no such step
    qmodel = synth.build_model(synth.SHAPES["tiny-qwen2"], synth.Q4_0, seed=26)
    _, qw = synth.to_hip(qmodel, dev)
    qs = qmodel.shape
    gq = ca.LlamaConfig(embedding_dim=qs.dim, hidden_dim=qs.hidden, n_layers=qs.n_layers, n_heads=qs.n_heads, n_kv_heads=qs.n_kv_heads,
                        vocab_size=qs.vocab, seq_len=qs.seq_len, rms_norm_eps=qs.rms_eps, rope_dim=qs.rope_dim, architecture="gemma")
    with pytest.raises(ca.CrabmlError) as e:
        ca.HipLlamaRunner(gq, qw, dev, 64, True)
    assert kind(e) == 9
    # a Gemma model created as "llama" still runs -- as a Llama model: the oracle's Llama runner on the same weights, bit for bit
    sdev = ca.HipTensorDevice(0, False, 0, True)
    sconf, sw = synth.to_hip(model, sdev)
    from tests.helpers import to_oracle
    odev = o.OracleDevice(thread_num=4)
    lr = o.OracleLlamaRunner(*to_oracle(model, odev), odev, 64, True)
    as_llama = ca.HipLlamaRunner(conf_as("llama"), sw, sdev, 64, True)
    as_gemma = ca.HipLlamaRunner(sconf, sw, sdev, 64, True)
    for i, t in enumerate(TOKS[:3]):
        want = lr.forward([t], i).copy()
        assert same_bits(as_llama.forward(t, i), want), i
        assert not same_bits(as_gemma.forward(t, i), want), i


@pytest.mark.parametrize("fmt", ["Q8_0", "Q4_0"])
def test_gemma_2b_shape_two_layers(ca, fmt):
    """Two layers of the Gemma-2B shape (dim 2048, hidden 16384, 8 heads on 1 kv head of 256, vocabulary 256000, tied): strict is
    bit-exact over 3 tokens, fast is within FAST_TOL; then one fast step at position 1023 behind a 1023-token prompt pass --
    k_attn_flash<8, 256> with 16 slices and the merge launch -- against the same step of a CRABML_HIP_LLAMA_EXACT_ATTENTION context (the
    chain the kernel replaces; a restatement of 1024 tokens at this vocabulary is minutes of CPU), inside the FLASH row of FAST_TOL."""
    model = synth.build_model(synth.SHAPES["gemma-2b"], synth.TYPE_BY_NAME[fmt], seed=27, n_layers=2)
    toks = TOKS[:3]
    ref, _ = restated(model, True, toks, seq_len=64)
    sdev = ca.HipTensorDevice(0, False, 0, True)
    conf, w = synth.to_hip(model, sdev)
    r = ca.HipLlamaRunner(conf, w, sdev, 64, True)
    for i, t in enumerate(toks):
        assert same_bits(r.forward(t, i), ref[i]), f"strict step {i}"
    del r, w
    fdev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, fdev)
    f = ca.HipLlamaRunner(conf, w, fdev, 64, True)
    lf = [f.forward(t, i).copy() for i, t in enumerate(toks)]
    assert all(np.isfinite(x).all() for x in lf)
    check_fast(f"gemma-fused/gemma-2b-2L/{fmt}", fmt, rel_errs(lf, ref))
    del f
    prompt = [(7 * i + 3) % model.shape.vocab for i in range(1023)]
    steps = []
    for flags in (0, EXACT_ATTENTION):
        c = ca.HipLlamaRunner(conf, w, fdev, 1032, True, extra_flags=flags)
        c.prefill(prompt)
        steps.append(np.array(c.forward(11, 1023)))
        del c
    assert np.isfinite(steps[0]).all()
    check_fast(f"gemma-fused/gemma-2b-2L/flash-vs-exact-at-1023/{fmt}", "FLASH:" + fmt, rel_errs([steps[0]], [steps[1]]))
