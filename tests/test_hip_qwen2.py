"""GPU parity of the Qwen2 decode step (crabml_hip_llama_create_arch: the q|k|v kernels' QKV_QWEN2 form -- NEOX row pairs, the
q / k / v biases) against tests/qwen2_ref.py, the restatement of Llama2Runner<CpuTensor>::forward_qwen2 (llama2.rs:283-351).

  * strict-order device: logits AND KV-cache bytes bit-identical to the restatement at every step, on every q|k|v kernel form
    (ordered fused launches, K-quant segments, per-op segments), graph replay and eager launches;
  * fast device: within the per-format FAST_TOL of the restatement and of the per-op trait path;
  * the prompt pass, the device samplers, the unchanged runner and the create-time errors."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests.helpers import FAST_TOL, FAST_TOL_MODEL, check_fast
from tests.qwen2_ref import OracleQwen2Runner, to_oracle_qwen2
from tests.sampler_ref import sample as sampler_ref_sample

pytestmark = pytest.mark.gpu
TOKS = [1, 365, 400, 282, 7, 9, 11]
# The fast step's default hop-free norm (wo quantizes x * w_norm per block and leaves 1 / rms to the consumer, which
# re-rolls the 126-vs-127 rounding of a block's largest element) is the one deviation the per-op trait path does not have.  On the tiny
# head_dim-64 Qwen2 model (20-60x bias channels) it shows median 9.1e-3 / max 1.0e-2 of max|logit| on MI355X against the per-op path's
# 7.4e-3 / 8.2e-3.  With CRABML_HIP_LLAMA_EXACT_NORM the fused step is held to the Llama bounds (FAST_TOL) like the per-op path; the
# default step is held to 2 x observed on this model (the FAST_TOL_MODEL convention of tests/helpers.py).
EXACT_NORM = 8388608  # CRABML_HIP_LLAMA_EXACT_NORM (include/crabml_hip.h)
QWEN2_TOL_DEFAULT_NORM = {("tiny-qwen2", "Q4_0"): (1.8e-2, 2.1e-2)}
PREFILL_INT8_GEMM = 524288  # CRABML_HIP_LLAMA_PREFILL_INT8_GEMM (include/crabml_hip_debug.h)


def shape_of(name, **kw):
    return synth.ModelShape(**{**synth.SHAPES[name].__dict__, **kw})


def restated(model, kv_f16, tokens, seq_len=64):
    odev = o.OracleDevice(thread_num=4)
    r = OracleQwen2Runner(*to_oracle_qwen2(model, odev), odev, seq_len, kv_f16)
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


STRICT = [("tiny-qwen2", "Q4_0", True, {}), ("tiny-qwen2", "Q8_0", False, {}), ("tiny-qwen2", "Q4_1", True, {}),
          ("tiny-qwen2", "Q4_K", False, {}), ("tiny-qwen2", "Q4_K_M", True, {}), ("tiny-qwen2", "Q5_K", True, {}),
          ("tiny-qwen2-g7", "Q4_0", True, {}), ("tiny-qwen2-g7", "Q4_K", False, {}),
          ("tiny-qwen2", "Q4_0", False, {"rope_dim": 32}), ("tiny-qwen2", "Q4_K", True, {"rope_dim": 32}),
          ("tiny-qwen2", "Q8_0", True, {"tied": True})]


@pytest.mark.parametrize("shape,fmt,kv_f16,over", STRICT, ids=lambda v: str(v))
def test_qwen2_strict_is_bit_exact(ca, shape, fmt, kv_f16, over):
    mix = fmt == "Q4_K_M"
    model = synth.build_model(shape_of(shape, **over), synth.Q4_K if mix else synth.TYPE_BY_NAME[fmt], seed=21, k_m_mix=mix)
    ref, orr = restated(model, kv_f16, TOKS)
    dev = ca.HipTensorDevice(0, False, 0, True)
    conf, w = synth.to_hip(model, dev)
    for use_graph in (True, False):
        r = ca.HipLlamaRunner(conf, w, dev, 64, kv_f16, use_graph)
        for i, t in enumerate(TOKS):
            assert same_bits(r.forward(t, i), ref[i]), f"graph={use_graph} step {i}"
        check_kv(r, orr, model.shape, len(TOKS), kv_f16)


@pytest.mark.parametrize("shape,fmt", [("tiny-qwen2", "Q4_0"), ("tiny-qwen2", "Q8_0"), ("tiny-qwen2", "Q4_1"), ("tiny-qwen2", "Q4_K"),
                                       ("tiny-qwen2-g7", "Q4_0"), ("tiny-qwen2-g7", "Q4_K")])
def test_qwen2_fast_matches_restatement_and_trait_path(ca, shape, fmt):
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=22)
    toks = TOKS + [3, 5, 8]
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
    check_fast(f"qwen2-trait/{shape}/{fmt}", fmt, et)
    check_fast(f"qwen2-fused-exact-norm/{shape}/{fmt}", fmt, ee)
    if (shape, fmt) in QWEN2_TOL_DEFAULT_NORM:
        med, mx = QWEN2_TOL_DEFAULT_NORM[(shape, fmt)]
        assert np.median(ef) <= med and np.max(ef) <= mx, ef
    else:
        check_fast(f"qwen2-fused/{shape}/{fmt}", fmt, ef)
    med, mx = FAST_TOL[fmt]
    assert np.max(eft) <= 2 * mx


@pytest.mark.parametrize("fmt", ["Q4_0", "Q4_K"])
def test_qwen2_prefill(ca, fmt):
    """Strict device: prefill = the token loop bit for bit (logits of the last token, KV bytes) across a chunk boundary.  Fast device:
    the int8 and the f16-weight GEMM passes within the format's bound of the restatement."""
    model = synth.build_model(synth.SHAPES["tiny-qwen2"], synth.TYPE_BY_NAME[fmt], seed=23)
    n = 40
    prompt = [(11 * i + 5) % model.shape.vocab for i in range(n)]
    ref, orr = restated(model, True, prompt)
    sdev = ca.HipTensorDevice(0, False, 0, True)
    conf, w = synth.to_hip(model, sdev)
    r = ca.HipLlamaRunner(conf, w, sdev, 64, True, prefill_chunk=24)
    assert same_bits(r.prefill(prompt), ref[-1])
    check_kv(r, orr, model.shape, n, True)
    fdev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, fdev)
    tol = FAST_TOL_MODEL.get(("tiny-qwen2", fmt), FAST_TOL[fmt])[1]
    for flags in (0, PREFILL_INT8_GEMM):
        lg = np.array(ca.HipLlamaRunner(conf, w, fdev, 64, True, prefill_chunk=24, extra_flags=flags).prefill(prompt))
        assert np.isfinite(lg).all()
        err = np.max(np.abs(lg - ref[-1])) / np.max(np.abs(ref[-1]))
        assert err <= tol, (flags, err)


def test_qwen2_device_samplers(ca):
    model = synth.build_model(synth.SHAPES["tiny-qwen2"], synth.Q4_0, seed=24)
    dev = ca.HipTensorDevice(0, False, 0, True)
    conf, w = synth.to_hip(model, dev)
    # greedy: the device loop = a host arg-max loop over the restated logits
    odev = o.OracleDevice(thread_num=4)
    orr = OracleQwen2Runner(*to_oracle_qwen2(model, odev), odev, 64, True)
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
    # sampling: decode_sample = sampler_ref on the restated logits, coin for coin
    coins = [0.13, 0.71, 0.42, 0.95]
    orr2 = OracleQwen2Runner(*to_oracle_qwen2(model, odev), odev, 64, True)
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


def test_qwen2_unchanged_runner_equals_per_op(ca):
    """The C++ mirror's forward_qwen2 over HipTensor (llama2.rs:283-351 op for op) on the strict device equals the restatement and
    the CRABML_HIP_FLAG_PER_OP device bit for bit."""
    model = synth.build_model(synth.SHAPES["tiny-qwen2"], synth.Q8_0, seed=25)
    ref, _ = restated(model, True, TOKS[:4])
    for mode in ("lazy", "per-op"):
        dev = ca.HipTensorDevice(0, False, 0, True, mode)
        conf, w = synth.to_hip(model, dev)
        r = ca.Llama2Runner(conf, w, dev, 64, True)
        for i, t in enumerate(TOKS[:4]):
            assert same_bits(r.forward([t], i), ref[i]), (mode, i)
        if mode == "lazy":  # served by the Qwen2 decode context, every token
            st = dev.lazy_stats()
            assert st["learned"] == 1 and st["fused_tokens"] == 4 and st["replayed"] == 0, st


def test_qwen2_create_errors(ca):
    model = synth.build_model(synth.SHAPES["tiny-qwen2"], synth.Q4_0, seed=26)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    s = model.shape

    def conf_as(arch):
        return ca.LlamaConfig(embedding_dim=s.dim, hidden_dim=s.hidden, n_layers=s.n_layers, n_heads=s.n_heads,
                              n_kv_heads=s.n_kv_heads, vocab_size=s.vocab, seq_len=s.seq_len, rms_norm_eps=s.rms_eps,
                              rope_dim=s.rope_dim, architecture=arch)

    def kind(e):
        return int(str(e.value).split("ErrorKind(")[1].split(")")[0])

    for arch in ("gemma", "phi2"):
        with pytest.raises(ca.CrabmlError) as e:
            ca.HipLlamaRunner(conf_as(arch), w, dev, 64, True)
        assert kind(e) == 9, arch  # NotImplemented
    with pytest.raises(ca.CrabmlError) as e:
        ca.HipLlamaRunner(conf, w, dev, 64, True, True, True, 2, 0)
    assert kind(e) == 9
    good = list(w.bk)
    for bad in (ca.HipTensor.from_cpu(np.zeros(s.kv_dim - 32, np.float32).view(np.uint8), [s.kv_dim - 32], ca.GGMLType.F32, dev),
                ca.HipTensor.from_cpu(np.zeros(s.kv_dim, np.float16).view(np.uint8), [s.kv_dim], ca.GGMLType.F16, dev)):
        w.bk = good[:-1] + [bad]
        with pytest.raises(ca.CrabmlError) as e:
            ca.HipLlamaRunner(conf, w, dev, 64, True)
        assert kind(e) == 5  # BadInput
    conf, w = synth.to_hip(model, dev)  # fresh handles (a list assigned to w.bk assigns into the tensors it replaces)
    with pytest.raises(ca.CrabmlError) as e:  # good biases on a Llama model
        ca.HipLlamaRunner(conf_as("llama"), w, dev, 64, True)
    assert kind(e) == 5
    assert np.isfinite(ca.HipLlamaRunner(conf, w, dev, 64, True).forward(1, 0)).all()


def test_create_arch_without_an_architecture_is_create(ca):
    """crabml_hip_llama_create_arch(NULL) and with {LLAMA, no biases} equal crabml_hip_llama_create bit for bit on a Llama model."""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=28)
    for strict in (True, False):
        dev = ca.HipTensorDevice(0, False, 0, strict)
        conf, w = synth.to_hip(model, dev)
        runners = [ca.HipLlamaRunner(conf, w, dev, 64, True, create_entry=e) for e in (0, 1, 2)]
        for i, t in enumerate(TOKS):
            lg = [r.forward(t, i).copy() for r in runners]
            assert same_bits(lg[1], lg[0]) and same_bits(lg[2], lg[0]), (strict, i)


def test_qwen2_7b_shape_four_layers(ca):
    model = synth.build_model(synth.SHAPES["qwen2.5-7b"], synth.Q4_0, seed=27, n_layers=4)
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
    check_fast("qwen2-fused/qwen2.5-7b-4L/Q4_0", "Q4_0", rel_errs(lf, ref))
