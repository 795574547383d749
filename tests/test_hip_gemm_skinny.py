"""The skinny GEMM of short prompt passes (k_gemm_skinny / k_gemm_skinny_k, gemm_skinny.hip): Q4_0 / Q8_0 weights x Q8_0 rows and
Q4_K / Q6_K weights x Q8_K rows.

1. the kernel by itself (crabml_hip_debug_gemm_skinny) against the float64 sum of the dequantized operands, per output inside
   (k / 32 + 3) * 2^-24 * S, S = the sum over the 32-element groups of |group term| (Q4_K: |scale term| + |minimum term|): the
   integer dots are exact, a group contributes at most one f32 term with two roundings before it, and any order of adding
   T <= k / 32 terms costs at most (T - 1) * 2^-24 * S (weight_formats.chunk_dots states exactly this bound for the four formats);
2. rows past the live ones are never read: the hook quantizes every row x holds, and NaN rows behind the b live ones change no bit;
3. through crabml_hip_llama_prefill: the pass's plan names the kernel (4) for every matrix from 6 rows, the row GEMV (3) below, and
   the logits stay inside the format's fast tolerance of the oracle's token loop."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests.fused_step_ref import parse_act
from tests.helpers import FAST_TOL, to_oracle
from tests.weight_formats import FORMATS, chunk_dots, weight_rows

pytestmark = pytest.mark.gpu

FMTS = ["Q4_0", "Q8_0", "Q4_K", "Q6_K"]
# a partial row tile and one block / super-block; one tile and an odd block count no power-of-two k-split divides; 17 tiles, every
# wave one unit; one or two tiles of several units per wave with a short last run and waves without blocks
SHAPES = {32: [(40, 32), (16, 288), (272, 2048), (24, 6400)], 256: [(40, 256), (16, 768), (272, 2048), (24, 6400)]}
BLOCK_BYTES = {o.Q8_0: 34, o.Q8_K: 292}


def upload(ca, hdev, fmt, m, k, b, seed):
    F = FORMATS[synth.TYPE_BY_NAME[fmt]]
    rng = np.random.default_rng(seed)
    raw = synth.random_blocks(rng, m * k, F.typ)
    x = (rng.standard_normal((b, k)) * rng.uniform(0.1, 4.0)).astype(np.float32)
    return F, raw, x, ca.HipTensor.from_cpu(raw, [m, k], getattr(ca.GGMLType, F.ht), hdev)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("b", [2, 3, 8, 15])
def test_kernel_against_float64(ca, hdev, fmt, b):
    worst = 0.0
    for m, k in SHAPES[FORMATS[synth.TYPE_BY_NAME[fmt]].block_elems]:
        F, raw, x, w = upload(ca, hdev, fmt, m, k, b, 1000 * b + m + k)
        hx = ca.HipTensor.new(x.reshape(-1), [b, k], hdev)
        got = np.asarray(w.debug_gemm_skinny(hx, b), dtype=np.float64).reshape(b, m)
        rhs = ca.GGMLType.Q8_0 if F.rhs == o.Q8_0 else ca.GGMLType.Q8K
        xq = np.asarray(hx.debug_quantize(rhs)).reshape(b, -1)
        assert xq.shape[1] == k // (32 if F.rhs == o.Q8_0 else 256) * BLOCK_BYTES[F.rhs]
        wr = weight_rows(synth.RawTensor(raw, [m, k], F.typ), 0, m)
        for bi in range(b):
            exact, bound = chunk_dots(wr, parse_act(xq[bi], F.rhs))
            ratio = np.abs(got[bi] - exact) / bound
            worst = max(worst, float(ratio.max()))
            assert np.all(ratio <= 1.0), (fmt, b, m, k, bi, int(ratio.argmax()), float(ratio.max()))
    print(f"{fmt} b={b}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("fmt", FMTS)
def test_only_the_live_rows_are_read(ca, hdev, fmt):
    m, k, b = 40, 768 if fmt.endswith("K") else 288, 3
    F, raw, x, w = upload(ca, hdev, fmt, m, k, b, 77)
    padded = np.full((16, k), np.nan, np.float32)
    padded[:b] = x
    alone = np.asarray(w.debug_gemm_skinny(ca.HipTensor.new(x.reshape(-1), [b, k], hdev), b))
    behind = np.asarray(w.debug_gemm_skinny(ca.HipTensor.new(padded.reshape(-1), [16, k], hdev), b))
    assert np.all(np.isfinite(alone)) and np.array_equal(alone.view(np.uint32), behind.view(np.uint32))


@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0", "Q4_K", "Q4_K_M"])
@pytest.mark.parametrize("n,warm", [(2, 0), (5, 0), (6, 0), (7, 0), (14, 0), (15, 0), (7, 5), (16, 0)])
def test_public_prompt_pass(ca, fmt, n, warm):
    """n rows after `warm` decode steps.  The pass takes the skinny GEMM from 6 rows (passes of 1..5 rows stay on the row GEMV:
    profiles/skinny_gemm.md) up to 15, with Q8_K rows up to 14 (the existing launch pins hold 5-row passes and the K-quants' 15-row
    passes to the row GEMV); 16 rows keep the int8 matrix-core GEMM (2)"""
    top = 14 if fmt.startswith("Q4_K") else 15
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.TYPE_BY_NAME[fmt[:4]], seed=91, k_m_mix=fmt == "Q4_K_M")
    toks = [(11 * i + 5) % model.shape.vocab for i in range(warm + n + 1)]
    odev = o.OracleDevice(thread_num=4, use_avx2=False)
    oconf, ow = to_oracle(model, odev)
    orr = o.OracleLlamaRunner(oconf, ow, odev, 32, True)
    refs = [np.asarray(orr.forward([t], i)).copy() for i, t in enumerate(toks)]
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    r = ca.HipLlamaRunner(conf, w, dev, 32, True)
    for i in range(warm):
        r.forward(toks[i], i)
    tol = FAST_TOL[fmt[:4]][1]
    for layer in range(model.shape.n_layers):
        t = ca.HipLlamaRunner(conf, w, dev, 32, True)
        for i in range(warm):
            t.forward(toks[i], i)
        plan = t.debug_prefill_tap(toks[warm:warm + n], layer)["plan"]
        for word in ("q", "k", "v", "wo", "gate", "up", "down"):
            assert plan["kernel_" + word] == (2 if n >= 16 else 4 if 6 <= n <= top else 3), (fmt, n, warm, layer, word, plan)
    got = np.asarray(r.prefill(toks[warm:warm + n]))
    nxt = np.asarray(r.forward(toks[warm + n], warm + n))
    for what, a, ref in (("pass", got, refs[warm + n - 1]), ("next forward", nxt, refs[warm + n])):
        err = float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))
        print(f"{fmt} n={n} warm={warm} {what}: {err:.3e} (tolerance {tol})")
        assert err <= tol, (fmt, n, warm, what, err)
