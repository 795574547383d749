"""Llama2Runner<CpuTensor>::forward_gemma (crabml-llama2/src/llama2.rs:455-524) restated over the oracle's tensor ops, the way
tests/qwen2_ref.py restates forward_qwen2: forward_llama with the embedded row scaled by sqrt(embed_dim) (:468), NEOX rope without
biases (:499-500) and GELU in the FFN (:512, forward_ffn's Activation::GeLU arm :624-627).  Attention, wo, the norms and the classifier
(tied when the weights carry no output.weight, :203-207) are the oracle runner's own (test infrastructure)."""
import numpy as np

from oracle import oracle as o
from tests.helpers import to_oracle


# tests/test_hip_gemma.py's fast-path comparison on Q4_K models: the tokens, and per shape a model seed at which the REFERENCE is quiet
# under ulp-sized reordering noise (tests/test_gemma.py::test_q4_k_fast_path_seeds_are_quiet_in_the_reference says what that means and
# checks it without a device).  Chosen from the reference alone -- the smallest quiet seed from 22 on.
FAST_TOKS = [1, 365, 400, 282, 7, 9, 11, 3, 5, 8]
FAST_Q4_K_SEEDS = {"tiny-gemma": 26, "tiny-gemma-g8": 29}


def perturbed_reference(model, tokens, noise_seed, ulps, seq_len=64):
    """forward_gemma's logits with every matmul_vec output moved by a random whole number of f32 ulps in [-ulps, ulps] (noise_seed
    None: unperturbed): what ANOTHER ORDER of the f32 block sums of a row dot does to it, and so what any re-associating
    implementation may do -- the reference's own sensitivity, no device involved."""
    rng = np.random.default_rng(noise_seed)
    orig = o.OracleTensor.matmul_vec

    def noisy(self, x):
        c = orig(self, x)
        if noise_seed is not None:
            k = rng.integers(-ulps, ulps + 1, size=c.storage.size).astype(np.int32)
            c.storage[:] = (c.storage.view(np.int32) + k).view(np.float32)
        return c

    o.OracleTensor.matmul_vec = noisy
    try:
        odev = o.OracleDevice(thread_num=4)
        r = OracleGemmaRunner(*to_oracle(model, odev), odev, seq_len, True)
        return [r.forward([t], i).copy() for i, t in enumerate(tokens)]
    finally:
        o.OracleTensor.matmul_vec = orig


def to_oracle_gemma(model, odev):
    """RawModel of a Gemma shape -> (oracle LlamaConfig, LlamaWeights); a Gemma file has the Llama tensors (model.rs:229)."""
    return to_oracle(model, odev)


class OracleGemmaRunner(o.OracleLlamaRunner):
    """OracleLlamaRunner whose forward runs forward_gemma (llama2.rs:184-211 dispatches on the architecture)."""

    def forward_llama(self, tokens, pos):
        return self.forward_gemma(tokens, pos)

    def forward_gemma(self, tokens, pos):  # llama2.rs:455-524
        c, w, T = self.conf, self.weights, self.T
        embed_dim, n_heads, n_kv_heads, head_dim = c.embedding_dim, c.n_heads, c.n_kv_heads, c.head_size()
        rope_dim = c.rope_dim if c.rope_dim is not None else head_dim
        n_batch = len(tokens)
        x = T.alloc([n_batch, embed_dim], o.F32, self.device)
        x.copy_rows_from(w.token_embed, list(tokens))
        x = x.scale_inplace(np.sqrt(np.float32(embed_dim)))  # (embed_dim as f32).sqrt()
        x = x.with_name("scaled_embed")
        for l in range(c.n_layers):
            x_attn_orig = x.dup()
            x = x.rms_norm_inplace(c.rms_norm_eps)
            x = x.mul_inplace(w.rms_att_weight[l])
            x = x.with_name(f"attn_rmsnorm:{l}:{pos}")
            q = w.wq[l].matmul_vec(x)
            k = w.wk[l].matmul_vec(x)
            v = w.wv[l].matmul_vec(x)
            q = q.reshape([n_heads, head_dim])
            k = k.reshape([n_kv_heads, head_dim])
            q = q.rope_inplace(o.ROPE_NEOX, pos, rope_dim)
            k = k.rope_inplace(o.ROPE_NEOX, pos, rope_dim)
            x = self.forward_multi_query_attention(q, k, v, l, pos, n_kv_heads, n_heads, embed_dim, head_dim, n_batch)
            x = x.add_inplace(x_attn_orig)
            x = self.forward_ffn_gelu(x, l)
            x = x.with_name(f"ffn_out:{l}:{pos}")
        x = x.rms_norm_inplace(c.rms_norm_eps)
        x = x.mul_inplace(w.rms_final_weight)
        return x.with_name(f"final_rmsnorm:{pos}")

    def forward_ffn_gelu(self, x, l):  # llama2.rs:605-638 with Activation::GeLU (the FFN norm's eps is the literal 1e-5)
        w = self.weights
        x_orig = x.dup()
        x = x.rms_norm_inplace(1e-5)
        x = x.mul_inplace(w.rms_ffn_weight[l])
        h1 = w.ffn_gate_weight[l].matmul_vec(x)
        h2 = w.ffn_up_weight[l].matmul_vec(x)
        h1 = h1.gelu_inplace()
        h1 = h1.mul_inplace(h2)
        x = w.ffn_down_weight[l].matmul_vec(h1)
        return x.add_inplace(x_orig)
