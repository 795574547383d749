"""Gemma without a GPU: the synthetic Gemma weights and their GGUF round trip through the C++ loader, the restatement of
forward_gemma (tests/gemma_ref.py) against the oracle's Llama runner, and the recorded-op matcher on the library's record-only test
device (CRABML_HIP_FLAG_DRY, armed by CRABML_HIP_TEST_HOOKS=1, as in tests/test_lazy_queue.py): the unchanged runner's Gemma token
is served by the fused step, and every single deviation from forward_gemma's op sequence stays op by op."""
import math
import os

import numpy as np
import pytest

os.environ["CRABML_HIP_TEST_HOOKS"] = "1"

import crabml_amd as ca  # noqa: E402
from crabml_amd import synth  # noqa: E402
from oracle import oracle as o  # noqa: E402
from tests.gemma_ref import FAST_Q4_K_SEEDS, FAST_TOKS, OracleGemmaRunner, perturbed_reference, to_oracle_gemma  # noqa: E402
from tests.helpers import to_oracle  # noqa: E402

F32, F16 = ca.GGMLType.F32, ca.GGMLType.F16
TOKS = [1, 365, 400, 282, 7, 9]


def gemma_model(shape="tiny-gemma", wtype=synth.Q4_0, seed=3, **kw):
    return synth.build_model(synth.SHAPES[shape], wtype, seed=seed, **kw)


def dry():
    return ca.HipTensorDevice(0, False, 0, False, "dry")


def test_synthetic_gemma_weights():
    """The Gemma build is the same seed's Llama build without output.weight (tied) and without biases; the shapes carry Gemma-2B's
    multi-query geometry: head_dim 256 on one kv head."""
    g = gemma_model(seed=5)
    lm = gemma_model(seed=5, arch="llama")
    s = g.shape
    assert s.arch == "gemma" and s.tied and s.head_dim == 256 and s.n_kv_heads == 1 and s.n_heads == 2
    assert "output.weight" not in g.tensors and not [n for n in g.tensors if n.endswith(".bias")]
    assert set(lm.tensors) == set(g.tensors)  # (the shape is tied whatever the architecture)
    for n, t in g.tensors.items():
        assert np.array_equal(lm.tensors[n].data, t.data), n
    g8, b2 = synth.SHAPES["tiny-gemma-g8"], synth.SHAPES["gemma-2b"]
    assert (g8.dim, g8.hidden, g8.n_layers, g8.n_heads, g8.n_kv_heads, g8.vocab, g8.seq_len, g8.head_dim) == (2048, 1024, 2, 8, 1, 1024, 256, 256)
    assert (b2.dim, b2.hidden, b2.n_layers, b2.n_heads, b2.n_kv_heads, b2.vocab, b2.seq_len) == (2048, 16384, 18, 8, 1, 256000, 8192)
    assert b2.tied and b2.arch == "gemma" and b2.rms_eps == 1e-6 and b2.head_dim == 256
    # a Llama shape built as Gemma is tied by default; an explicit classifier type unties it
    assert "output.weight" not in synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=1, n_layers=1, arch="gemma").tensors
    assert "output.weight" in synth.build_model(synth.SHAPES["tiny-gemma"], synth.Q4_0, seed=1, n_layers=1, output_type=synth.Q8_0).tensors


def test_gemma_gguf_round_trips_through_the_cpp_loader(tmp_path):
    model = gemma_model("tiny-gemma", synth.Q8_0, seed=7)
    s = model.shape
    path = str(tmp_path / "gemma.gguf")
    synth.write_gguf(model, path)
    gf = ca.GGUFFile(path)
    assert gf.architecture == "gemma"
    conf = gf.load_config()
    assert conf.architecture == "gemma"
    assert (conf.embedding_dim, conf.hidden_dim, conf.n_layers, conf.n_heads, conf.n_kv_heads, conf.vocab_size, conf.seq_len) == \
        (s.dim, s.hidden, s.n_layers, s.n_heads, s.n_kv_heads, s.vocab, s.seq_len)
    assert conf.rms_norm_eps == np.float32(s.rms_eps) and conf.rope_dim is None
    names = {t[0] for t in gf.tensor_infos()}
    assert "output.weight" not in names and not [n for n in names if n.endswith(".bias")]
    w = gf.load_weights(conf, dry())
    assert w.output_weight is None  # tied: the classifier is token_embd (llama2.rs:203-207)
    assert len(w.bq) == len(w.bk) == len(w.bv) == 0
    assert len(w.wq) == s.n_layers and w.wk[1].shape() == [s.kv_dim, s.dim] and w.token_embed.shape() == [s.vocab, s.dim]
    # an untied Gemma file keeps its output.weight (create does not insist on the tie)
    upath = str(tmp_path / "gemma_untied.gguf")
    synth.write_gguf(gemma_model("tiny-gemma", synth.Q8_0, seed=7, n_layers=1, output_type=synth.Q8_0), upath)
    ug = ca.GGUFFile(upath)
    assert ug.load_weights(ug.load_config(), dry()).output_weight is not None


def test_restatement_is_not_the_llama_runner_and_its_activation_matters(oracle):
    """forward_gemma is not forward_llama on the same weights; and with the FFN's activation alone swapped back to SiLU the logits
    change again (the embed scale and NEOX rope already differ from Llama)."""
    model = gemma_model(wtype=synth.Q8_0, seed=4)
    odev = o.OracleDevice(thread_num=2)

    class SiluFfn(OracleGemmaRunner):
        def forward_ffn_gelu(self, x, l):
            return self.forward_ffn(x, l)

    gr = OracleGemmaRunner(*to_oracle_gemma(model, odev), odev, 16, True)
    lr = o.OracleLlamaRunner(*to_oracle(model, odev), odev, 16, True)
    sr = SiluFfn(*to_oracle_gemma(model, odev), odev, 16, True)
    got = [gr.forward([t], i).copy() for i, t in enumerate(TOKS[:3])]
    ref = [lr.forward([t], i).copy() for i, t in enumerate(TOKS[:3])]
    sil = [sr.forward([t], i).copy() for i, t in enumerate(TOKS[:3])]
    assert all(np.isfinite(g).all() for g in got + sil)
    assert not any(np.array_equal(g, r) for g, r in zip(got, ref))
    assert not any(np.array_equal(g, r) for g, r in zip(got, sil))
    assert not any(np.array_equal(g, r) for g, r in zip(sil, ref))


@pytest.mark.parametrize("shape", ["tiny-gemma", "tiny-gemma-g8"])
def test_q4_k_fast_path_seeds_are_quiet_in_the_reference(oracle, shape):
    """Where the Q4_K seeds of the GPU fast-path comparison come from.  With ONE kv head every head reads the same f16 cache rows, so a
    single flipped quant of the round-to-nearest Q8_K quantizer lands in a cache row and moves every later step: on most seeds of these
    shapes the reference itself -- every row dot moved by +-1 or +-2 f32 ulps, what another order of its block sums does -- shows
    flip-sized steps (seed 22, tiny-gemma-g8: 24 of 60 steps over six perturbations, up to 7e-3 of max|logit|).  The median bound of
    FAST_TOL's K-quant row assumes that flips are rare, so the comparison runs on a seed at which the reference is QUIET: no step of
    any perturbation moves by 1e-4 (FLIP_SIZED, tests/helpers.py).  The criterion looks at the reference only; and a seed that is not
    quiet is shown not to be, so the criterion can tell."""
    def flip_sized_steps(seed):
        model = gemma_model(shape, synth.Q4_K, seed=seed)
        ref = perturbed_reference(model, FAST_TOKS, None, 0)
        n = 0
        for ns, ulps in ((0, 1), (1, 2), (2, 1)):
            got = perturbed_reference(model, FAST_TOKS, ns, ulps)
            n += sum(np.max(np.abs(g - r)) / np.max(np.abs(r)) > 1e-4 for g, r in zip(got, ref))
        return n

    assert flip_sized_steps(FAST_Q4_K_SEEDS[shape]) == 0
    if shape == "tiny-gemma-g8":
        assert flip_sized_steps(22) > 0


def forward_rs_gemma(conf, w, dev, kc, vc, tok, pos, eps=1e-6, scale="sqrt", mode=None, silu_layer=None, bias=None):
    """forward_gemma's call sequence with every handle released where rustc would (the twin of tests/test_lazy_queue.forward_rs).
    Deviations for the matcher: scale (None: no embed scale; a float: that factor), mode (the rope mode), silu_layer (SiLU in that
    layer), bias (an f32 vector added to layer 0's k)."""
    dim, hd = conf.embedding_dim, conf.head_size()
    nh, nkv = conf.n_heads, conf.n_kv_heads
    mode = ca.RopeMode.Neox if mode is None else mode
    x = ca.HipTensor.alloc([1, dim], F32, dev)
    x.copy_rows_from(w.token_embed, [tok])
    if scale is not None:
        x = x.scale_inplace(float(np.sqrt(np.float32(dim))) if scale == "sqrt" else scale)    # llama2.rs:468
    for l in range(conf.n_layers):
        x_attn_orig = x.dup()                                  # :473
        x = x.rms_norm_inplace(eps)
        x = x.mul_inplace(w.rms_att_weight[l])
        q = w.wq[l].matmul_vec(x)                              # :488-490
        k = w.wk[l].matmul_vec(x)
        v = w.wv[l].matmul_vec(x)
        if bias is not None and l == 0:
            k = k.add_inplace(bias)
        q = q.reshape([nh, hd]).rope_inplace(mode, pos, hd)    # :496-500
        k = k.reshape([nkv, hd]).rope_inplace(mode, pos, hd)
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
        h1 = h1.silu_inplace() if l == silu_layer else h1.gelu_inplace()  # :624-627
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


@pytest.mark.parametrize("shape", ["tiny-gemma", "tiny-gemma-g8"])
def test_the_unchanged_runner_is_served_by_the_fused_step(shape):
    """The C++ mirror's forward_gemma over HipTensor: learned once, every token (the learning one included) runs as 2 L + 1 fused
    segments of the Gemma decode context."""
    dev = dry()
    conf, w = synth.to_hip(gemma_model(shape), dev)
    assert conf.architecture == "gemma"
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
    conf, w = synth.to_hip(gemma_model(), dev)
    kc, vc = caches(conf, dev)
    n = 4
    for i, t in enumerate(TOKS[:n]):
        forward_rs_gemma(conf, w, dev, kc, vc, t, i)
    st = dev.lazy_stats()
    assert st["learned"] == 1 and st["fused_tokens"] == n and st["segments"] == (2 * conf.n_layers + 1) * n, st
    assert st["replayed"] == 0 and st["aborts"] == 0, st


@pytest.mark.parametrize("deviation", ["no-embed-scale", "another-scale", "silu-in-one-layer", "llama-rope", "a-bias-add"])
def test_single_deviations_from_forward_gemma_stay_per_op(deviation):
    """Only the complete combination -- the scale by exactly sqrtf(dim), NEOX rope without adds, GELU in every layer -- is Gemma."""
    dev = dry()
    conf, w = synth.to_hip(gemma_model(), dev)
    kc, vc = caches(conf, dev)
    kw = {"no-embed-scale": {"scale": None}, "another-scale": {"scale": float(np.float32(np.sqrt(np.float32(conf.embedding_dim))) * np.float32(1.0000002))},
          "silu-in-one-layer": {"silu_layer": 1}, "llama-rope": {"mode": ca.RopeMode.Llama}}.get(deviation, {})
    if deviation == "another-scale":
        assert np.float32(kw["scale"]) != np.sqrt(np.float32(conf.embedding_dim))
    if deviation == "a-bias-add":
        kw["bias"] = ca.HipTensor.from_cpu(np.zeros(conf.kv_dim(), np.float32).view(np.uint8), [conf.kv_dim()], F32, dev)
    for i, t in enumerate(TOKS[:3]):
        forward_rs_gemma(conf, w, dev, kc, vc, t, i, **kw)
    st = dev.lazy_stats()
    assert st["learned"] == 0 and st["fused_tokens"] == 0 and st["segments"] == 0, st
    assert st["replayed"] == st["recorded"] > 0, st
