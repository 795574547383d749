"""Qwen2 without a GPU: the restatement of forward_qwen2 (tests/qwen2_ref.py) against the oracle's Llama runner and a float64 numpy
forward, the synthetic Qwen2 weights and their GGUF round trip through the C++ loader, and the recorded-op matcher on the library's
record-only test device (CRABML_HIP_FLAG_DRY, armed by CRABML_HIP_TEST_HOOKS=1, as in tests/test_lazy_queue.py): the unchanged runner's
Qwen2 token is served by the fused step, and every deviation from forward_qwen2's op sequence stays op by op."""
import math
import os

import numpy as np
import pytest

os.environ["CRABML_HIP_TEST_HOOKS"] = "1"

import crabml_amd as ca  # noqa: E402
from crabml_amd import synth  # noqa: E402
from oracle import oracle as o  # noqa: E402
from tests.helpers import to_oracle  # noqa: E402
from tests.qwen2_ref import OracleQwen2Runner, to_oracle_qwen2  # noqa: E402

F32, F16 = ca.GGMLType.F32, ca.GGMLType.F16
TOKS = [1, 365, 400, 282, 7, 9]


def qwen2_model(shape="tiny-qwen2", wtype=synth.Q4_0, seed=3, **kw):
    return synth.build_model(synth.SHAPES[shape], wtype, seed=seed, **kw)


def test_restatement_without_biases_and_rope_is_the_llama_runner(oracle):
    """With zero biases and rope_dim = 0 forward_qwen2 is forward_llama op for op: the restatement equals OracleLlamaRunner bit
    for bit.  With the biases and NEOX rope it does not (both matter)."""
    shp = synth.ModelShape(**{**synth.SHAPES["tiny-qwen2"].__dict__, "rope_dim": 0})
    model = synth.build_model(shp, synth.Q8_0, seed=4)
    llama = synth.build_model(shp, synth.Q8_0, seed=4, arch="llama")
    for name in [n for n in model.tensors if n.endswith(".bias")]:
        model.tensors[name].data[:] = 0
    odev = o.OracleDevice(thread_num=2)
    qr = OracleQwen2Runner(*to_oracle_qwen2(model, odev), odev, 16, True)
    lr = o.OracleLlamaRunner(*to_oracle(llama, odev), odev, 16, True)
    for i, t in enumerate(TOKS):
        a, b = qr.forward([t], i).copy(), lr.forward([t], i).copy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"step {i}"
    full = qwen2_model(wtype=synth.Q8_0, seed=4)
    fr = OracleQwen2Runner(*to_oracle_qwen2(full, odev), odev, 16, True)
    lr2 = o.OracleLlamaRunner(*to_oracle(llama, odev), odev, 16, True)
    got = [fr.forward([t], i).copy() for i, t in enumerate(TOKS[:3])]
    ref = [lr2.forward([t], i).copy() for i, t in enumerate(TOKS[:3])]
    assert all(np.isfinite(g).all() for g in got)
    assert not any(np.array_equal(g, r) for g, r in zip(got, ref))


def test_synthetic_qwen2_weights():
    """The Qwen2 build is the same seed's Llama build plus F32 biases of the right lengths, some channels far larger than the rest;
    the 7B / 3B shapes carry their group sizes and the 3B classifier is tied."""
    q = qwen2_model("tiny-qwen2-g7", synth.Q4_0, seed=5)
    lm = qwen2_model("tiny-qwen2-g7", synth.Q4_0, seed=5, arch="llama")
    s = q.shape
    assert s.arch == "qwen2" and lm.shape.arch == "llama" and s.n_heads // s.n_kv_heads == 7 and s.head_dim == 128
    assert set(q.tensors) - set(lm.tensors) == {f"blk.{l}.attn_{x}.bias" for l in range(s.n_layers) for x in "qkv"}
    for n, t in lm.tensors.items():
        assert np.array_equal(q.tensors[n].data, t.data), n
    for l in range(s.n_layers):
        for x, n in (("q", s.dim), ("k", s.kv_dim), ("v", s.kv_dim)):
            t = q.tensors[f"blk.{l}.attn_{x}.bias"]
            b = t.data.view(np.float32)
            assert t.typ == synth.F32 and t.shape == [n] and b.size == n
            assert np.max(np.abs(b)) > 15 * np.median(np.abs(b))
    b7, b3 = synth.SHAPES["qwen2.5-7b"], synth.SHAPES["qwen2.5-3b"]
    assert (b7.dim, b7.hidden, b7.n_layers, b7.n_heads, b7.n_kv_heads, b7.vocab) == (3584, 18944, 28, 28, 4, 152064)
    assert (b3.dim, b3.hidden, b3.n_layers, b3.n_heads, b3.n_kv_heads, b3.vocab) == (2048, 11008, 36, 16, 2, 151936) and b3.tied
    tied = synth.build_model(b3, synth.Q4_0, seed=1, n_layers=1)
    assert "output.weight" not in tied.tensors



def f64_qwen2_forward(model, tokens):
    """forward_qwen2 (llama2.rs:283-351) in float64 numpy from the dequantized weights, independent of the oracle: f32 weights (no rhs
    quantizer), f32 KV cache; the softmax's exponential rounded through f16 as the reference's table does (softmax.rs:36-54)."""
    s = model.shape
    W = {n: (t.data.view(np.float32).astype(np.float64).reshape(t.shape) if t.typ == synth.F32 else None) for n, t in model.tensors.items()}
    hd, nh, nkv = s.head_dim, s.n_heads, s.n_kv_heads
    rope_dim = s.rope_dim if s.rope_dim is not None else hd
    kc = [[] for _ in range(s.n_layers)]
    vc = [[] for _ in range(s.n_layers)]

    def rms(x, w, eps):
        return x / np.sqrt(np.mean(x * x) + eps) * w

    def neox(v, pos):
        v = v.reshape(-1, hd).copy()
        for i in range(rope_dim // 2):
            th = pos / 10000.0 ** (2.0 * i / hd)
            a, b = v[:, i].copy(), v[:, i + hd // 2].copy()
            v[:, i], v[:, i + hd // 2] = a * math.cos(th) - b * math.sin(th), a * math.sin(th) + b * math.cos(th)
        return v

    out = []
    for pos, tok in enumerate(tokens):
        x = W["token_embd.weight"][tok].copy()
        for l in range(s.n_layers):
            b = f"blk.{l}."
            xn = rms(x, W[b + "attn_norm.weight"], s.rms_eps)
            q = W[b + "attn_q.weight"] @ xn + W[b + "attn_q.bias"]
            k = W[b + "attn_k.weight"] @ xn + W[b + "attn_k.bias"]
            v = W[b + "attn_v.weight"] @ xn + W[b + "attn_v.bias"]
            q, k = neox(q, pos) / math.sqrt(hd), neox(k, pos)
            kc[l].append(k)
            vc[l].append(v.reshape(nkv, hd))
            K, V = np.stack(kc[l], 1), np.stack(vc[l], 1)  # (nkv, t, hd)
            att = np.empty((nh, hd))
            for h in range(nh):
                g = h % nkv  # the f32 cache pairs head h with kv head h % n_kv (the batch_matmul broadcast)
                sc = K[g] @ q[h]
                e = np.float16(np.exp(np.float16(sc - sc.max()).astype(np.float64))).astype(np.float64)
                att[h] = (e / e.sum()) @ V[g]
            x = x + W[b + "attn_output.weight"] @ att.reshape(-1)
            xn = rms(x, W[b + "ffn_norm.weight"], 1e-5)
            g1, u = W[b + "ffn_gate.weight"] @ xn, W[b + "ffn_up.weight"] @ xn
            x = x + W[b + "ffn_down.weight"] @ (g1 / (1 + np.exp(-g1)) * u)
        xn = rms(x, W["output_norm.weight"], s.rms_eps)
        out.append(W["output.weight"] @ xn)
    return out


F64_BOUND = 2e-3  # of max|logit| (f32 arithmetic + the f16-rounded exponentials against float64; observed about 3e-4)


def test_restatement_with_biases_tracks_a_float64_forward(oracle):
    model = qwen2_model(wtype=synth.F32, seed=6)
    odev = o.OracleDevice(thread_num=2)
    qr = OracleQwen2Runner(*to_oracle_qwen2(model, odev), odev, 16, False)
    ref = f64_qwen2_forward(model, TOKS)
    for i, t in enumerate(TOKS):
        got = qr.forward([t], i).astype(np.float64)
        err = np.max(np.abs(got - ref[i])) / np.max(np.abs(ref[i]))
        assert err <= F64_BOUND, (i, err)


def test_qwen2_gguf_round_trips_through_the_cpp_loader(tmp_path):
    model = qwen2_model("tiny-qwen2-g7", synth.Q4_0, seed=7)
    s = model.shape
    path = str(tmp_path / "qwen2.gguf")
    synth.write_gguf(model, path)
    gf = ca.GGUFFile(path)
    assert gf.architecture == "qwen2"
    conf = gf.load_config()
    assert conf.architecture == "qwen2"
    assert (conf.embedding_dim, conf.hidden_dim, conf.n_layers, conf.n_heads, conf.n_kv_heads, conf.vocab_size, conf.seq_len) == \
        (s.dim, s.hidden, s.n_layers, s.n_heads, s.n_kv_heads, s.vocab, s.seq_len)
    assert conf.rms_norm_eps == np.float32(s.rms_eps) and conf.rope_dim is None
    infos = {t[0]: t for t in gf.tensor_infos()}
    for l in range(s.n_layers):
        for x, n in (("q", s.dim), ("k", s.kv_dim), ("v", s.kv_dim)):
            name = f"blk.{l}.attn_{x}.bias"
            assert list(infos[name][1]) == [n] and infos[name][2] == synth.F32
            assert gf.tensor_data(name)[:4 * n] == model.tensors[name].data.tobytes()
    w = gf.load_weights(conf, dry())
    assert len(w.bq) == len(w.bk) == len(w.bv) == s.n_layers
    assert w.bq[0].shape() == [s.dim] and w.bk[1].shape() == [s.kv_dim] and w.bv[1].dtype() == ca.GGMLType.F32
    # a Llama file loads without biases
    lpath = str(tmp_path / "llama.gguf")
    synth.write_gguf(synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=7, n_layers=1), lpath)
    lg = ca.GGUFFile(lpath)
    assert lg.load_config().architecture == "llama" and len(lg.load_weights(lg.load_config(), dry()).bq) == 0


def dry():
    return ca.HipTensorDevice(0, False, 0, False, "dry")


def forward_rs_qwen2(conf, w, dev, kc, vc, tok, pos, eps=1e-6, adds=True, mode=None, skip_adds_layer=None, bias=None):
    """forward_qwen2's call sequence with every handle released where rustc would (the twin of tests/test_lazy_queue.forward_rs).
    Deviations for the matcher: adds=False (no bias adds), mode (the rope mode), skip_adds_layer (one layer without its adds),
    bias (a replacement for layer 0's k bias)."""
    dim, hd = conf.embedding_dim, conf.head_size()
    nh, nkv = conf.n_heads, conf.n_kv_heads
    mode = ca.RopeMode.Neox if mode is None else mode
    x = ca.HipTensor.alloc([1, dim], F32, dev)
    x.copy_rows_from(w.token_embed, [tok])
    for l in range(conf.n_layers):
        x_attn_orig = x.dup()                                  # llama2.rs:302
        x = x.rms_norm_inplace(eps)
        x = x.mul_inplace(w.rms_att_weight[l])
        q = w.wq[l].matmul_vec(x)                              # :312-314
        k = w.wk[l].matmul_vec(x)
        v = w.wv[l].matmul_vec(x)
        if adds and l != skip_adds_layer:
            q = q.add_inplace(w.bq[l])                         # :315-317
            k = k.add_inplace(bias if (bias is not None and l == 0) else w.bk[l])
            v = v.add_inplace(w.bv[l])
        q = q.reshape([1, nh, hd]).rope_inplace(mode, pos, hd)  # :321-327
        k = k.reshape([1, nkv, hd]).rope_inplace(mode, pos, hd)
        kv_k = k.reshape([1, nkv, hd]).transpose([1, 0, 2])
        kv_v = v.reshape([1, nkv, hd]).transpose([1, 0, 2])
        kc[l].concatenate(kv_k, 1)
        vc[l].concatenate(kv_v, 1)
        del kv_k, kv_v
        q = q.reshape([1, nh, hd]).transpose([1, 0, 2]).contiguous().scale_inplace(1.0 / math.sqrt(np.float32(hd)))
        k_cache, kc[l] = kc[l], None
        k_orig = k_cache.strider()
        k_cache = k_cache.transpose([0, 2, 1])
        attn = q.batch_matmul(k_cache)
        attn = attn.softmax_inplace(2)
        kc[l] = k_cache.with_strider(k_orig)
        del k_cache
        v_cache, vc[l] = vc[l], None
        v_orig = v_cache.strider()
        x_with_attn = attn.batch_matmul(v_cache)
        x_with_attn = x_with_attn.reshape([1, dim])
        vc[l] = v_cache.with_strider(v_orig)
        del v_cache
        x = w.wo[l].matmul_vec(x_with_attn)
        del q, attn, x_with_attn
        del k, v
        x = x.add_inplace(x_attn_orig)
        x_orig_ffn = x.dup()
        x = x.rms_norm_inplace(1e-5)
        x = x.mul_inplace(w.rms_ffn_weight[l])
        h1 = w.ffn_gate_weight[l].matmul_vec(x)
        h2 = w.ffn_up_weight[l].matmul_vec(x)
        h1 = h1.silu_inplace()
        h1 = h1.mul_inplace(h2)
        x = w.ffn_down_weight[l].matmul_vec(h1)
        x = x.add_inplace(x_orig_ffn)
        del x_orig_ffn, h1, h2
        del x_attn_orig
    x = x.rms_norm_inplace(eps)
    x = x.mul_inplace(w.rms_final_weight)
    x_final = ca.HipTensor.alloc([dim], F32, dev)
    x_final.copy_rows_from(x, [0])
    ow = w.output_weight if w.output_weight is not None else w.token_embed
    logits = ow.matmul_vec(x_final)
    out = np.array(logits.export())
    del x, x_final, logits
    return out


def caches(conf, dev, seq=32):
    mk = lambda: ca.HipTensor.alloc([conf.n_kv_heads, seq, conf.head_size()], F16, dev).resize(1, 0)  # noqa: E731
    return [mk() for _ in range(conf.n_layers)], [mk() for _ in range(conf.n_layers)]


@pytest.mark.parametrize("shape", ["tiny-qwen2", "tiny-qwen2-g7"])
def test_the_unchanged_runner_is_served_by_the_fused_step(shape):
    """The C++ mirror's forward_qwen2 over HipTensor: learned once, every token (the learning one included) runs as 2 L + 1 fused
    segments of the Qwen2 decode context."""
    dev = dry()
    conf, w = synth.to_hip(qwen2_model(shape), dev)
    r = ca.Llama2Runner(conf, w, dev, 32, True)
    n = 5
    for i, t in enumerate(TOKS[:n]):
        r.forward([t], i)
    st = dev.lazy_stats()
    L = conf.n_layers
    assert st["learned"] == 1 and st["fused_tokens"] == n and st["segments"] == (2 * L + 1) * n, st
    assert st["replayed"] == 0 and st["aborts"] == 0, st
    assert r.kv_cache_len() == n


def test_the_rust_twin_is_served_by_the_fused_step():
    dev = dry()
    conf, w = synth.to_hip(qwen2_model(), dev)
    kc, vc = caches(conf, dev)
    for i, t in enumerate(TOKS[:4]):
        forward_rs_qwen2(conf, w, dev, kc, vc, t, i)
    st = dev.lazy_stats()
    assert st["learned"] == 1 and st["fused_tokens"] == 4 and st["segments"] == (2 * conf.n_layers + 1) * 4, st
    assert st["replayed"] == 0 and st["aborts"] == 0, st


@pytest.mark.parametrize("deviation", ["neox-without-adds", "adds-with-llama-rope", "one-layer-without-adds", "broadcast-bias", "f16-bias"])
def test_deviations_from_forward_qwen2_stay_per_op(deviation):
    dev = dry()
    conf, w = synth.to_hip(qwen2_model(), dev)
    kc, vc = caches(conf, dev)
    kw = {"neox-without-adds": {"adds": False}, "adds-with-llama-rope": {"mode": ca.RopeMode.Llama},
          "one-layer-without-adds": {"skip_adds_layer": 1}}.get(deviation, {})
    if deviation == "broadcast-bias":  # a bias of the wrong length (1: add_inplace broadcasts it)
        kw["bias"] = ca.HipTensor.from_cpu(np.ones(1, np.float32).view(np.uint8), [1], F32, dev)
    if deviation == "f16-bias":  # add_inplace refuses a non-f32 rhs: the token never completes, nothing is fused
        kw["bias"] = ca.HipTensor.from_cpu(np.zeros(conf.kv_dim(), np.float16).view(np.uint8), [conf.kv_dim()], F16, dev)
        with pytest.raises(ca.CrabmlError):
            forward_rs_qwen2(conf, w, dev, kc, vc, 1, 0, **kw)
        st = dev.lazy_stats()
        assert st["learned"] == 0 and st["fused_tokens"] == 0, st
        return
    for i, t in enumerate(TOKS[:3]):
        forward_rs_qwen2(conf, w, dev, kc, vc, t, i, **kw)
    st = dev.lazy_stats()
    assert st["learned"] == 0 and st["fused_tokens"] == 0 and st["segments"] == 0, st
    assert st["replayed"] == st["recorded"] > 0, st
