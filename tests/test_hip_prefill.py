"""GPU parity for the batched prefill (crabml_hip_llama_prefill): the token loop of Llama2Runner::prefill
(llama2.rs:111-129) as (rows, k) matmul_vec passes + causal attention.

  * strict-order device: the last logits AND the KV-cache bytes are bit-identical to the oracle's token loop, for any
    chunking, and decoding continues bit-identically after it;
  * fast device: prompts of >= 16 rows put the Q4_0 / Q8_0 weight matrices on the matrix cores (gemm_mfma.hip); the
    last logits agree with the oracle within the fast-mode tolerance and the greedy continuation with the token loop's."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests.helpers import FAST_TOL, FAST_TOL_MODEL, to_oracle

EXACT = 4194304  # CRABML_HIP_LLAMA_EXACT_ATTENTION: the fast step keeps the reference's exact attention arithmetic
pytestmark = pytest.mark.gpu
PROMPT = [1, 365, 400, 282, 7, 9, 11, 13, 2, 77, 500, 31, 8, 19, 64, 128, 3, 5, 900, 12, 14, 16, 18]  # 23 tokens


def oracle_run(model, kv_f16, tokens, seq_len=64):
    odev = o.OracleDevice(thread_num=4)
    oconf, ow = to_oracle(model, odev)
    r = o.OracleLlamaRunner(oconf, ow, odev, seq_len, kv_f16)
    out = [r.forward([t], i).copy() for i, t in enumerate(tokens)]
    return out, r


def kv_equal(runner, orr, model, n_pos, kv_f16, seq_len=64):
    s = model.shape
    es = 2 if kv_f16 else 4
    for layer in range(s.n_layers):
        for which, cache in ((False, orr.key_cache), (True, orr.value_cache)):
            got = runner.debug_kv(layer, which, kv_f16)
            exp = cache[layer].storage.view(np.uint8)
            for h in range(s.n_kv_heads):
                lo = h * seq_len * s.head_dim * es
                n = n_pos * s.head_dim * es
                if not np.array_equal(got[lo:lo + n], exp[lo:lo + n]):
                    return False
    return True


@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0", "Q4_1", "Q4_K", "Q8_K", "F32"])
@pytest.mark.parametrize("kv_f16", [False, True])
@pytest.mark.parametrize("chunk", [0, 5])
def test_prefill_strict_equals_the_oracle_token_loop(ca, fmt, kv_f16, chunk):
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.TYPE_BY_NAME[fmt], seed=81)
    ref, orr = oracle_run(model, kv_f16, PROMPT + [21, 22])
    dev = ca.HipTensorDevice(0, False, 0, True)
    conf, w = synth.to_hip(model, dev)
    r = ca.HipLlamaRunner(conf, w, dev, 64, kv_f16, prefill_chunk=chunk)
    lg = r.prefill(PROMPT)
    n = len(PROMPT)
    assert r.kv_cache_len() == n
    assert np.array_equal(lg.view(np.uint32), ref[n - 1].view(np.uint32))
    # decoding continues from the prefilled cache
    for i, t in enumerate([21, 22]):
        assert np.array_equal(r.forward(t, n + i).view(np.uint32), ref[n + i].view(np.uint32)), f"step {i} after prefill"
    assert kv_equal(r, orr, model, n + 2, kv_f16)


@pytest.mark.parametrize("fmt", ["Q5_0", "Q5_1", "Q2_K", "Q3_K", "Q5_K"])
@pytest.mark.parametrize("strict", [True, False])
def test_prefill_formats_without_a_matrix_core_kernel(ca, fmt, strict):
    """The formats the reference serves with scalar code only: a prompt pass runs their GEMVs row by row (no MFMA tile kernel).
    Strict order: bit-identical to the oracle's token loop; fast: inside the format's decode tolerance."""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.TYPE_BY_NAME[fmt], seed=84)
    ref, orr = oracle_run(model, True, PROMPT + [21])
    dev = ca.HipTensorDevice(0, False, 0, strict)
    conf, w = synth.to_hip(model, dev)
    r = ca.HipLlamaRunner(conf, w, dev, 64, True)
    lg = r.prefill(PROMPT)
    n = len(PROMPT)
    nxt = r.forward(21, n)
    if strict:
        assert np.array_equal(lg.view(np.uint32), ref[n - 1].view(np.uint32))
        assert np.array_equal(nxt.view(np.uint32), ref[n].view(np.uint32))
        assert kv_equal(r, orr, model, n + 1, True)
    else:
        from tests.helpers import FAST_TOL
        for got, want in ((lg, ref[n - 1]), (nxt, ref[n])):
            assert np.max(np.abs(got - want)) / np.max(np.abs(want)) <= FAST_TOL[fmt][1], fmt


def test_prefill_15m_shape_head_dim_48_strict(ca):
    """tinyllamas-15M geometry: head_dim 48, rope_dim 48, dim 288 (k not a multiple of 256)."""
    model = synth.build_model(synth.SHAPES["15m"], synth.Q8_0, seed=82)
    ref, orr = oracle_run(model, True, PROMPT)
    dev = ca.HipTensorDevice(0, False, 0, True)
    conf, w = synth.to_hip(model, dev)
    r = ca.HipLlamaRunner(conf, w, dev, 64, True)
    assert np.array_equal(r.prefill(PROMPT).view(np.uint32), ref[-1].view(np.uint32))
    assert kv_equal(r, orr, model, len(PROMPT), True)


def test_prefill_in_two_calls_and_after_decode_steps(ca):
    """prefill appends at the current KV length (base_pos = kv_cache_len(), llama2.rs:124): forward, prefill, forward,
    prefill again -- the same cache and logits as one token loop."""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=83)
    toks = PROMPT + [40, 41, 42, 43, 44]
    ref, orr = oracle_run(model, True, toks)
    dev = ca.HipTensorDevice(0, False, 0, True)
    conf, w = synth.to_hip(model, dev)
    r = ca.HipLlamaRunner(conf, w, dev, 64, True)
    r.forward(toks[0], 0)
    lg = r.prefill(toks[1:18])
    assert np.array_equal(lg.view(np.uint32), ref[17].view(np.uint32))
    assert np.array_equal(r.forward(toks[18], 18).view(np.uint32), ref[18].view(np.uint32))
    lg = r.prefill(toks[19:])
    assert np.array_equal(lg.view(np.uint32), ref[-1].view(np.uint32))
    assert r.kv_cache_len() == len(toks)
    assert kv_equal(r, orr, model, len(toks), True)


@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0", "Q4_1", "Q4_K", "Q6_K", "Q8_K"])
def test_prefill_fast_on_the_matrix_cores(ca, fmt):
    """23 rows >= 16: q/k/v, wo, gate/up, down run as MFMA GEMMs.  Logits within the fast-mode tolerance of the oracle;
    the greedy continuation equals the one after a fast token loop over the same prompt."""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.TYPE_BY_NAME[fmt], seed=84)
    ref, _ = oracle_run(model, True, PROMPT)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    a = ca.HipLlamaRunner(conf, w, dev, 64, True)
    lg = a.prefill(PROMPT)
    # fast-mode bound of tests/test_hip_fused.py: median 3e-2, max 1e-1 of max|logit| (one chaotic 126-vs-127 flip of
    # the truncating Q8_0 quantizer, buf_q8_0.rs:119-124, moves a whole block)
    err = np.max(np.abs(lg - ref[-1])) / np.max(np.abs(ref[-1]))
    assert err <= 1e-1, err
    b = ca.HipLlamaRunner(conf, w, dev, 64, True)
    for i, t in enumerate(PROMPT):
        lb = b.forward(t, i)
    assert np.max(np.abs(lg - lb)) / np.max(np.abs(lb)) <= 1e-1
    nxt = int(np.argmax(ref[-1]))
    ta, tb = list(a.decode_greedy(nxt, 8)), list(b.decode_greedy(nxt, 8))
    assert a.kv_cache_len() == b.kv_cache_len() == len(PROMPT) + 8
    assert ta[0] == tb[0]


def test_prefill_rejects_bad_input(ca):
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=85)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    r = ca.HipLlamaRunner(conf, w, dev, 16, True)
    with pytest.raises(Exception):
        r.prefill([])  # "expected at least 1 prompt token" (llama2.rs:117-122)
    with pytest.raises(Exception):
        r.prefill([1] * 17)  # does not fit the cache
    with pytest.raises(Exception):
        r.prefill([model.shape.vocab_size])  # token out of range
    assert r.kv_cache_len() == 0
    r.prefill([1, 2, 3])
    assert r.kv_cache_len() == 3


@pytest.mark.parametrize("n_heads,n_kv", [(8, 8), (8, 4), (8, 2), (8, 1)])
@pytest.mark.parametrize("kv_f16", [False, True])
def test_row_tiled_attention_equals_the_per_row_kernel(ca, n_heads, n_kv, kv_f16):
    """Prefill attention runs as one workgroup per (kv head, 4-row tile) carrying the G = n_heads / n_kv queries of each
    row (k_attn_tile); per (row, head) it is k_attn's arithmetic, so the pass is bit-identical to the per-row kernel
    (flag 2048 = NO_TILE_ATTENTION), for every group size, both cache types, ragged tiles and a non-zero base position."""
    shape = synth.ModelShape(f"g{n_heads // n_kv}", 512, 1024, 2, n_heads, n_kv, 1024, 64)
    model = synth.build_model(shape, synth.Q8_0, seed=86)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    a = ca.HipLlamaRunner(conf, w, dev, 64, kv_f16, extra_flags=EXACT)  # (the fast step's default is k_attn_flash_rows, not these)
    b = ca.HipLlamaRunner(conf, w, dev, 64, kv_f16, extra_flags=EXACT + 2048)
    for r in (a, b):
        r.forward(3, 0)
        r.forward(4, 1)
    la, lb = a.prefill(PROMPT), b.prefill(PROMPT)  # 23 rows at base position 2: five full tiles + a ragged one
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    la, lb = a.prefill([9, 8, 7]), b.prefill([9, 8, 7])  # a short second pass (one ragged tile)
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    s = model.shape
    es = 2 if kv_f16 else 4
    filled = a.kv_cache_len() * s.head_dim * es
    for layer in range(s.n_layers):
        for which in (False, True):
            ka, kb = a.debug_kv(layer, which, kv_f16), b.debug_kv(layer, which, kv_f16)
            for h in range(s.n_kv_heads):
                lo = h * 64 * s.head_dim * es
                assert np.array_equal(ka[lo:lo + filled], kb[lo:lo + filled]), (layer, which, h)


@pytest.mark.parametrize("n_heads,n_kv", [(8, 2), (8, 8)])
def test_long_prompt_attention_paths_are_bit_identical(ca, n_heads, n_kv):
    """A 1100-token prompt in 512-row passes: rows up to position 1024 take the row-tiled kernel, rows beyond it the
    long-context kernels with a row dimension (scores / softmax with the block-tree row sum / f16 PV chain, 64 rows per
    launch).  Against the per-(head, row) kernel everywhere (flag 2048): the same logits and the same KV cache, bit for
    bit; decoding continues identically."""
    shape = synth.ModelShape("long", 512, 1024, 2, n_heads, n_kv, 1024, 1200)
    model = synth.build_model(shape, synth.Q8_0, seed=87)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    prompt = [(7 * i + 3) % 1024 for i in range(1100)]
    a = ca.HipLlamaRunner(conf, w, dev, 1200, True, extra_flags=EXACT)
    b = ca.HipLlamaRunner(conf, w, dev, 1200, True, extra_flags=EXACT + 2048)
    la, lb = a.prefill(prompt), b.prefill(prompt)
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    # ... and the PV pass with one prompt row per workgroup (flag 16384) instead of the row tiles
    c = ca.HipLlamaRunner(conf, w, dev, 1200, True, extra_flags=EXACT + 16384)
    assert np.array_equal(c.prefill(prompt).view(np.uint32), la.view(np.uint32))
    nxt = int(np.argmax(la))
    assert list(a.decode_greedy(nxt, 6)) == list(b.decode_greedy(nxt, 6))
    filled = a.kv_cache_len() * shape.head_dim * 2
    for layer in range(shape.n_layers):
        for which in (False, True):
            ka, kb = a.debug_kv(layer, which, True), b.debug_kv(layer, which, True)
            for h in range(n_kv):
                lo = h * 1200 * shape.head_dim * 2
                assert np.array_equal(ka[lo:lo + filled], kb[lo:lo + filled]), (layer, which, h)


@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0", "Q4_1"])
def test_prefill_row_fusion_equals_the_separate_launches(ca, fmt):
    """Residual add + RMSNorm + quantize as one launch per prompt row and SiLU * mul + quantize as one (the default for Q8_0 /
    Q8_1 rhs formats) against the separate launches (flag 262144): same logits and the same decoding afterwards, bit for
    bit, in fast and in strict mode, in one and in several passes."""
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.TYPE_BY_NAME[fmt], seed=83)
    prompt = [(3 * i + 1) % 1000 for i in range(45)]
    for strict in (False, True):
        dev = ca.HipTensorDevice(0, False, 0, strict)
        conf, w = synth.to_hip(model, dev)
        for chunk in (0, 16):
            a = ca.HipLlamaRunner(conf, w, dev, 64, True, prefill_chunk=chunk)
            b = ca.HipLlamaRunner(conf, w, dev, 64, True, prefill_chunk=chunk, extra_flags=262144)
            la, lb = a.prefill(prompt), b.prefill(prompt)
            assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)), (fmt, strict, chunk)
            nxt = int(np.argmax(la))
            assert list(a.decode_greedy(nxt, 5)) == list(b.decode_greedy(nxt, 5))


@pytest.mark.parametrize("fmt", ["Q4_K", "Q4_K_M", "Q6_K"])
def test_prefill_row_fusion_k_quants_equals_the_separate_launches(ca, fmt):
    """Q8_K rows (K-quant layers), passes of >= 192 rows: residual add (+ the k pieces of the GEMM behind it) + RMSNorm + Q8_K quantize
    (+ the next GEMM's f16 planes) as ONE launch per prompt row (k_norm_quant_rows_k) against k_addn_f32 / k_res_epi / k_norm_f32_rows /
    k_quantize_q8_k (flag 262144): same logits and the same decoding afterwards, bit for bit, fast and strict, one pass of 200 rows
    and passes of 192 + 8 (the short tail keeps the separate launches)."""
    model = (synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_K, seed=29, k_m_mix=True) if fmt == "Q4_K_M"
             else synth.build_model(synth.SHAPES["tiny-gqa"], synth.TYPE_BY_NAME[fmt], seed=29))
    prompt = [(7 * i + 4) % 1000 for i in range(200)]
    for strict in (False, True):
        dev = ca.HipTensorDevice(0, False, 0, strict)
        conf, w = synth.to_hip(model, dev)
        for chunk in (512, 192):
            a = ca.HipLlamaRunner(conf, w, dev, 232, True, prefill_chunk=chunk)
            b = ca.HipLlamaRunner(conf, w, dev, 232, True, prefill_chunk=chunk, extra_flags=262144)
            la, lb = a.prefill(prompt), b.prefill(prompt)
            assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)), (fmt, strict, chunk)
            nxt = int(np.argmax(la))
            assert list(a.decode_greedy(nxt, 5)) == list(b.decode_greedy(nxt, 5))


PREFILL_INT8_GEMM = 524288  # CRABML_HIP_LLAMA_PREFILL_INT8_GEMM (include/crabml_hip_debug.h)


def _record_f16w(key, row):
    """the observed last-row logit errors of the f16 / int8 prompt passes -> gpurun_out/f16w_prefill_errors.json (evidence only)"""
    import json
    import os

    try:
        os.makedirs("gpurun_out", exist_ok=True)
        path = os.path.join("gpurun_out", "f16w_prefill_errors.json")
        prev = {}
        if os.path.exists(path):
            with open(path) as f:
                prev = json.load(f)
        prev[key] = row
        with open(path, "w") as f:
            json.dump(prev, f, indent=1, sort_keys=True)
    except (OSError, ValueError):
        pass


@pytest.mark.parametrize("fmt,shape,n", [("Q4_0", "tiny-gqa", 200), ("Q4_0", "15m", 173), ("Q4_0", "tiny-hd128", 384),
                                         ("Q8_0", "tiny-gqa", 200), ("Q8_0", "15m", 173), ("Q4_K", "tiny-gqa", 200),
                                         ("Q4_K", "tiny-hd128", 384), ("Q4_K_M", "tiny-gqa", 173), ("Q6_K", "tiny-gqa", 200),
                                         ("Q6_K", "tiny-hd128", 384), ("Q4_1", "tiny-gqa", 200), ("Q4_1", "15m", 173)])
def test_fast_prompt_pass_f16_weight_gemm(ca, fmt, shape, n):
    """Passes of >= 32 rows, Q4_0 / Q8_0 / Q4_1 / Q4_K / Q6_K weights, fast device: the weight GEMMs run on the f16 matrix cores with the block
    scales folded into the operands (k_gemm_f16w, gemm_f16w.hip -- a stated deviation of the fast tier: two (Q4_K: three) f16
    roundings per product instead of exact integer block dots).  Against the oracle's token loop it must sit inside the fast
    tolerance the int8 kernels are held to; against the int8 kernels (A/B flag) the two passes must agree inside it; the greedy
    continuation starts with the same token.  Shapes: k = 512 / 1024 (4 and 8 whole chunks; 2 and 4 super-blocks), 288 / 768 (the
    15M model: 9 and 24 blocks -- a ragged last chunk, rows that are no multiple of 64), ragged last column tiles (200 = 128 + 72,
    173 = 128 + 45), three full tiles (384).  Q4_K_M: the llama.cpp mix -- the q | k | v launch splits where v is Q6_K, and the rows'
    f16 planes are made once per k-slot order (Q4_K's and Q6_K's differ)."""
    if fmt == "Q4_K_M":
        model = synth.build_model(synth.SHAPES[shape], synth.Q4_K, seed=91, k_m_mix=True)
        tol_fmt = "Q4_K"
    else:
        model = synth.build_model(synth.SHAPES[shape], getattr(synth, fmt), seed=91)
        tol_fmt = fmt
    prompt = [(11 * i + 5) % model.shape.vocab for i in range(n)]
    odev = o.OracleDevice(thread_num=8, use_avx2=False)
    oconf, ow = to_oracle(model, odev)
    orr = o.OracleLlamaRunner(oconf, ow, odev, n + 16, True)
    ref = None
    for i, t in enumerate(prompt):
        ref = orr.forward([t], i)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    a = ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=512)
    b = ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=512, extra_flags=PREFILL_INT8_GEMM)
    la, lb = np.array(a.prefill(prompt)), np.array(b.prefill(prompt))
    scale = float(np.max(np.abs(ref)))
    ea, eb, eab = (float(np.max(np.abs(x - y))) / scale for x, y in ((la, ref), (lb, ref), (la, lb)))
    tol = FAST_TOL_MODEL.get((shape, tol_fmt), FAST_TOL[tol_fmt])[1]
    _record_f16w("%s/%s/%d" % (shape, fmt, n), {"f16_vs_oracle": ea, "int8_vs_oracle": eb, "f16_vs_int8": eab, "bound": tol})
    assert eb <= tol, ("int8 pass vs oracle", eb)
    # (where the exact int8 pass itself sits near the bound -- a flipped round-to-nearest quant on this prompt: tiny-gqa Q6_K, 4.1e-2 --
    # the f16 pass is held to 1.25 x that instead of to a margin of 1e-5)
    assert ea <= max(tol, 1.25 * eb), ("f16 pass vs oracle", ea)
    assert eab <= tol, ("f16 pass vs int8 pass", eab)
    assert not np.array_equal(la, lb)  # (the two passes are different arithmetic: equal logits would mean the flag does nothing)
    nxt = int(np.argmax(ref))
    assert list(a.decode_greedy(nxt, 4))[0] == list(b.decode_greedy(nxt, 4))[0]
    assert a.kv_cache_len() == b.kv_cache_len() == n + 4


@pytest.mark.parametrize("fmt,n", [("Q4_0", 200), ("Q4_K", 40), ("Q6_K", 64), ("Q8_0", 33), ("Q4_1", 130)])
def test_fast_prompt_pass_f16_weight_gemm_k_pieces(ca, fmt, n):
    """A wide feed-forward (hidden = 4096 against dim = 512, one layer): ffn_down's k range is cut into 8 pieces of 4 chunks (two
    super-blocks) and gate | up, q | k | v and wo (k = 512) into none -- the partial tiles of the pieces are added in piece order by
    k_addn_f32.  Row counts: 200 (T = 8, two column tiles), 40 and 64 (T = 4), 33 (T = 4, one row past T = 2's tile), 130.
    Same bounds as above: oracle token loop, the int8 pass, the two against each other."""
    shape = synth.ModelShape("tiny-wide", 512, 4096, 1, 4, 2, 512, 256, 1e-5, None)
    model = synth.build_model(shape, getattr(synth, fmt), seed=17)
    prompt = [(13 * i + 3) % shape.vocab for i in range(n)]
    odev = o.OracleDevice(thread_num=8, use_avx2=False)
    oconf, ow = to_oracle(model, odev)
    orr = o.OracleLlamaRunner(oconf, ow, odev, n + 16, True)
    ref = None
    for i, t in enumerate(prompt):
        ref = orr.forward([t], i)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    a = ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=512)
    b = ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=512, extra_flags=PREFILL_INT8_GEMM)
    la, lb = np.array(a.prefill(prompt)), np.array(b.prefill(prompt))
    la2 = np.array(ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=512).prefill(prompt))
    assert np.array_equal(la.view(np.uint32), la2.view(np.uint32))  # (the pieces are added in a fixed order: run to run the same bits)
    scale = float(np.max(np.abs(ref)))
    ea, eb, eab = (float(np.max(np.abs(x - y))) / scale for x, y in ((la, ref), (lb, ref), (la, lb)))
    tol = FAST_TOL[fmt][1]
    _record_f16w("tiny-wide/%s/%d" % (fmt, n), {"f16_vs_oracle": ea, "int8_vs_oracle": eb, "f16_vs_int8": eab, "bound": tol})
    assert eb <= tol, ("int8 pass vs oracle", eb)
    assert ea <= tol, ("f16 pass vs oracle", ea)
    assert eab <= tol, ("f16 pass vs int8 pass", eab)
    assert not np.array_equal(la, lb)


SEPARATE_F16_ROWS = 33554432  # CRABML_HIP_LLAMA_PREFILL_SEPARATE_F16_ROWS
NO_GU_EPILOGUE = 67108864  # CRABML_HIP_LLAMA_PREFILL_NO_GU_EPILOGUE


@pytest.mark.parametrize("fmt,shape,n", [("Q4_0", "tiny-gqa", 200), ("Q4_0", "15m", 77), ("Q8_0", "tiny-hd128", 96), ("Q4_1", "tiny-gqa", 130),
                                         ("Q4_K", "tiny-gqa", 200), ("Q4_K_M", "tiny-gqa", 64), ("Q6_K", "tiny-hd128", 40),
                                         ("Q4_0", "wide-ffn", 200), ("Q4_K", "wide-ffn", 173), ("Q8_0", "wide-ffn", 130),
                                         ("Q4_0", "dim-4096", 200), ("Q4_1", "dim-4096", 70), ("Q8_0", "dim-8192", 130)])
def test_fast_prompt_pass_rows_write_their_own_f16_planes(ca, fmt, shape, n):
    """The kernels that quantize the rows of a fast prompt pass (norm + quantize, SiLU * mul + quantize, the stand-alone quantizer for
    the attention output and for Q8_K rows) also leave the pre-scaled f16 planes the next weight GEMM reads (f16w_rows.hpp), in that
    GEMM's k-slot order -- the same bits k_rows_to_f16 makes from the finished planes in its own launch (the A/B flag): logits, the
    greedy continuation and the cache rows are bit-identical.  Q4_K_M: where v is Q6_K its GEMM re-makes the planes in its own order.
    Likewise SiLU * mul as the epilogue of the gate | up GEMM (one fragment of each matrix per wave; h quantized by the quantizer
    launch) against the separate SiLU * mul + quantize launch -- on these small shapes the epilogue form is taken where 64-row tiles of
    both matrices cover 1.5 workgroups per CU (the 8B shape's passes; here the `wide-ffn` cases)."""
    kw = dict(seed=23)
    # wide-ffn: hidden = 12288 -- 192 row tiles of 64 x two column tiles = 1.5 workgroups per CU: the gate | up launch takes the
    # SiLU * mul epilogue (one pass of > 128 rows; the 48-row passes keep the separate launch)
    # dim-4096 / dim-8192: rows of 4096 / 8192 elements take the 256-thread norm + quantize kernel (k_norm_quant_rows_w: a thread owns
    # half a quant block / a whole one) -- against the 1024-thread kernel behind the flag, on the fast AND the strict device
    shp = (synth.ModelShape("wide-ffn", 512, 12288, 1, 4, 2, 512, 256, 1e-5, None) if shape == "wide-ffn"
           else synth.ModelShape("dim-4096", 4096, 1024, 1, 32, 8, 512, 256, 1e-5, None) if shape == "dim-4096"
           else synth.ModelShape("dim-8192", 8192, 1024, 1, 64, 8, 512, 256, 1e-5, None) if shape == "dim-8192" else synth.SHAPES[shape])
    model = (synth.build_model(shp, synth.Q4_K, k_m_mix=True, **kw) if fmt == "Q4_K_M" else synth.build_model(shp, getattr(synth, fmt), **kw))
    prompt = [(17 * i + 2) % model.shape.vocab for i in range(n)]
    for strict in ((False, True) if shape.startswith("dim-") else (False,)):
        dev = ca.HipTensorDevice(0, False, 0, strict)
        conf, w = synth.to_hip(model, dev)
        for chunk in (512, 48):  # one pass / passes of 48 rows and a ragged tail
            a = ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=chunk)
            b = ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=chunk, extra_flags=SEPARATE_F16_ROWS | NO_GU_EPILOGUE)
            la, lb = np.array(a.prefill(prompt)), np.array(b.prefill(prompt))
            assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)), (fmt, shape, chunk, strict)
            nxt = int(np.argmax(la))
            assert list(a.decode_greedy(nxt, 6)) == list(b.decode_greedy(nxt, 6))


@pytest.mark.parametrize("fmt,shape", [("Q4_K", "tiny-gqa")])
def test_fast_prompt_pass_recomputes_a_chunk_whose_f16_rows_overflow(ca, fmt, shape):
    """A few massive channels (two elements of every ffn_norm weight x 2^16, as real checkpoints have): the ffn input's quantized
    rows hold values past 65504, which the f16 GEMM's B' = f16(q d) cannot, while the int8 GEMM -- and the oracle -- stay finite.
    The writers of B' raise the pass's overflow flag, and the chunk is computed again with the int8 GEMMs: its logits are those of
    the int8 pass bit for bit, the KV cache advances once, decoding continues identically; a second, shorter pass on the same
    runner (stale +-inf behind its rows in the f16 planes) stays finite."""
    model = synth.build_model(synth.SHAPES[shape], getattr(synth, fmt), seed=5)
    s = model.shape
    for l in range(s.n_layers):
        t = model.tensors[f"blk.{l}.ffn_norm.weight"]
        w = t.data.view(np.float32).copy()
        w[[3, s.dim // 2 + 1]] *= np.float32(2.0 ** 16)
        t.data = w.view(np.uint8)
    n = 64
    prompt = [(11 * i + 5) % s.vocab for i in range(n)]
    ref, orr = oracle_run(model, True, prompt, seq_len=n + 16)
    assert all(np.all(np.isfinite(r)) for r in ref), "the oracle must stay finite"
    for l in range(s.n_layers):
        assert np.all(np.isfinite(orr.key_cache[l].storage.view(np.float16)))
        assert np.all(np.isfinite(orr.value_cache[l].storage.view(np.float16)))
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    a = ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=512)
    b = ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=512, extra_flags=PREFILL_INT8_GEMM)
    la, lb = np.array(a.prefill(prompt)), np.array(b.prefill(prompt))
    assert np.all(np.isfinite(lb))
    assert np.all(np.isfinite(la)), "f16 pass: non-finite logits"
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    assert a.kv_cache_len() == b.kv_cache_len() == n
    nxt = int(np.argmax(ref[-1]))
    assert list(a.decode_greedy(nxt, 4)) == list(b.decode_greedy(nxt, 4))
    a.reset()
    l2 = np.array(a.prefill(prompt[:40]))
    assert np.all(np.isfinite(l2)) and a.kv_cache_len() == 40
