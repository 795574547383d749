"""The Q8 KV cache (use_f16_kv_cache == 2: per 32 elements of a head's K or V row, int8 values and one f16 scale): its
three attention kernels against float64 over the DEQUANTIZED planes, the cache write through a context, a context end to end, and what
create refuses.  The kernels' bounds are the f16 forms' (2e-5 for k_attn_flash, 1.5e-3 for the flash-rows family): int8 x f16 is exact
in f32, so the Q8 forms get no allowance beyond the one rounding the flash-rows staging declares (K^, V^ = f16(d * q)), restated here."""
import json
import os

import numpy as np
import pytest

from crabml_amd import synth
from tests.poison import release_devices, tokens_for  # noqa: F401 (autouse fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(8, 2, 128), (7, 1, 128), (6, 2, 64), (8, 1, 64)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_plan_mi355x.json")


def quantize(x):
    """the stated rule: d = f16(max|x| / 127) per 32 elements, q = x / d rounded to nearest, clamped to +-127; d = 0: q = 0"""
    b = x.astype(np.float32).reshape(x.shape[:-1] + (-1, 32))
    d = (np.abs(b).max(-1) / np.float32(127)).astype(np.float16)
    df = d.astype(np.float32)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(df > 0, np.clip(np.rint(b / df), -127, 127), 0).astype(np.int8)
    return q.reshape(x.shape), d.view(np.uint16)


def dequant(q, d, f16=False):
    """q * d in float64 (exact); f16: rounded to f16 first, the flash-rows staging's one rounding"""
    x = q.reshape(q.shape[:-1] + (-1, 32)).astype(np.float32) * d.view(np.float16).astype(np.float32)[..., None]  # exact in f32
    return (x.astype(np.float16) if f16 else x).astype(np.float64).reshape(q.shape)


def f64_attention(q, kf, vf, rows, pos0, p16):
    """row r over positions 0 .. pos0 + r of kf / vf [n_kv][seq][hd] float64; q rounded to f16 as the kernels round it; p16: the
    probabilities rounded to f16, the normalizer summing the rounded values (the flash-rows kernels)"""
    n_kv, seq, hd = kf.shape
    q16 = q.astype(np.float16).astype(np.float64).reshape(rows, -1, hd)
    grp = q16.shape[1] // n_kv
    out = np.zeros_like(q16)
    for h in range(q16.shape[1]):
        s = q16[:, h] @ kf[h // grp].T
        s[np.arange(seq)[None, :] > (pos0 + np.arange(rows))[:, None]] = -np.inf
        p = np.exp(s - s.max(axis=1, keepdims=True))
        if p16:
            p = p.astype(np.float16).astype(np.float64)
        out[:, h] = (p @ vf[h // grp]) / p.sum(axis=1, keepdims=True)
    return out.reshape(-1)


def rel_err(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


@pytest.fixture(scope="module")
def dev(ca):
    return ca.HipTensorDevice(0)


def decode_case(dev, n_heads, n_kv, hd, seq, slices, spread=1.0, kind="normal"):
    rng = np.random.default_rng(1000 * n_heads + 10 * hd + seq)
    q = (rng.standard_normal(n_heads * hd) * spread / np.sqrt(hd)).astype(np.float32)
    k = rng.standard_normal((n_kv, seq, hd)).astype(np.float32)
    v = rng.standard_normal((n_kv, seq, hd)).astype(np.float32)
    if kind == "spike":  # one position dominates, far from the slice that holds the running maximum first
        k[:, seq // 2] *= 6.0
    elif kind == "ties":  # every score equal: uniform probabilities over all slices
        k[:] = k[:, :1]
    elif kind == "dead":  # scores so low in all but the last slice that their weights underflow to 0 in the merge
        k[:, : seq - 1] = -np.abs(k[:, : seq - 1]) * 3
        q = np.abs(q) * 8
    (kq, kd), (vq, vd) = quantize(k), quantize(v)
    got, ticket = dev.debug_flash_attention_q8(q, kq.reshape(-1), kd.reshape(-1), vq.reshape(-1), vd.reshape(-1), n_heads, n_kv, hd, seq, slices)
    assert np.array_equal(got.view(np.uint32), ticket.view(np.uint32))  # the ticket form: the same operations in the same order
    assert np.all(np.isfinite(got))
    err = rel_err(got, f64_attention(q, dequant(kq, kd), dequant(vq, vd), 1, seq - 1, False))
    print(f"flash q8 vs float64, {n_heads}/{n_kv} x {hd}, seq {seq}, {slices} slices, {kind}: {err:.2e} of max|out|")
    return err


@pytest.mark.parametrize("slices", [1, 7, 32])
@pytest.mark.parametrize("seq", [1, 2, 15, 16, 17, 127, 128, 129, 1000, 2049])
@pytest.mark.parametrize("n_heads,n_kv,hd", SHAPES)
def test_decode_kernel_equals_float64_over_the_dequantized_planes(dev, n_heads, n_kv, hd, seq, slices):
    assert decode_case(dev, n_heads, n_kv, hd, seq, slices) <= 2e-5


@pytest.mark.parametrize("kind", ["spike", "ties", "dead"])
def test_decode_kernel_merge_edge_cases(dev, kind):
    assert decode_case(dev, 8, 2, 128, 3000, 32, spread=4.0, kind=kind) <= 2e-5


@pytest.mark.parametrize("slices", [1, 4])
@pytest.mark.parametrize("pos0,rows", [(0, 1), (0, 17), (0, 65), (5, 33), (100, 129), (777, 32)])
@pytest.mark.parametrize("n_heads,n_kv,hd", SHAPES)
def test_prompt_kernels_equal_float64_and_ignore_junk_behind_the_live_cache(dev, n_heads, n_kv, hd, pos0, rows, slices):
    """slices 1: k_attn_flash_rows<.., KV8>; 4: k_attn_flash_rows_split<.., KV8> and its merge.  The planes behind pos0 + rows -- the
    scale planes too -- hold NaN / Inf / huge patterns in the second run: bit-identical to the clean one."""
    rng = np.random.default_rng(100 * n_heads + hd + pos0)
    seq = pos0 + rows
    q = (rng.standard_normal(rows * n_heads * hd) / np.sqrt(hd)).astype(np.float32)
    (kq, kd), (vq, vd) = quantize(rng.standard_normal((n_kv, seq, hd))), quantize(rng.standard_normal((n_kv, seq, hd)))

    def run(qfill, dfill):
        planes = []
        for a, fill in ((kq, qfill), (kd, dfill), (vq, qfill), (vd, dfill)):
            p = np.zeros((n_kv, seq + 37, a.shape[-1]), dtype=a.dtype)
            p[:, seq:] = np.array(fill, dtype=np.uint16 if a.dtype == np.uint16 else np.uint8).astype(a.dtype)
            p[:, :seq] = a
            planes.append(p.reshape(-1))
        return dev.debug_flash_attention_rows_q8(q, *planes, n_heads, n_kv, hd, pos0, rows, slices)

    got = run(0, 0)
    assert np.all(np.isfinite(got))
    err = rel_err(got, f64_attention(q, dequant(kq, kd, True), dequant(vq, vd, True), rows, pos0, True))
    print(f"flash rows q8 vs float64, {n_heads}/{n_kv} x {hd}, pos0 {pos0}, {rows} rows, {slices} slices: {err:.2e} of max|out|")
    assert err <= 1.5e-3, err
    for qfill, dfill in ((0xFF, 0xFFFF), (0x7F, 0x7C00), (0x80, 0x7BFF)):
        assert np.array_equal(run(qfill, dfill).view(np.uint32), got.view(np.uint32)), (hex(qfill), hex(dfill))


def context(ca, dev, shape, kv, **kw):
    model = synth.build_model(synth.SHAPES[shape], synth.Q4_0, seed=61)
    conf, w = synth.to_hip(model, dev)
    return model.shape, ca.HipLlamaRunner(conf, w, dev, 128, kv, **kw)


@pytest.mark.parametrize("shape", ["tiny-hd128", "tiny-qwen2"])
def test_cache_write_of_the_prompt_pass_and_of_the_decode_step(ca, dev, shape):
    """Layer 0's K / V rows do not depend on attention: the f32-cache context's layer-0 cache is the exact x of the Q8 context's planes.
    Per block |q| <= 127 and |x - q d| <= d / 2 + amax 2^-11 (half a step; the f16 rounding of d, times 127).  Rows 0 .. 39 come from
    one prompt pass, rows 40 .. 42 from decode steps."""
    s, r8 = context(ca, dev, shape, 2)
    _, r32 = context(ca, dev, shape, 0)
    toks = tokens_for(s, 43, salt=3)
    for r in (r8, r32):
        r.prefill(toks[:40])
        for i in range(40, 43):
            r.forward(toks[i], i)
    kq, kd, vq, vd = r8.debug_kv_q8_read(0, 0, 43)
    for which_v, qs, ds in ((False, kq, kd), (True, vq, vd)):
        x = np.asarray(r32.debug_kv(0, which_v, False)).view(np.float32).reshape(s.n_kv_heads, 128, -1)[:, :43].astype(np.float64)
        xb = x.reshape(s.n_kv_heads, 43, -1, 32)
        qb = np.asarray(qs).reshape(xb.shape).astype(np.float64)
        d = np.asarray(ds).view(np.float16).astype(np.float64).reshape(xb.shape[:-1])[..., None]
        amax = np.abs(xb).max(-1, keepdims=True)
        assert amax.max() > 0 and np.abs(qb).max() == 127
        slack = np.abs(xb - qb * d) - (0.5 * d + amax * 2.0 ** -11)
        print(f"{shape} {'v' if which_v else 'k'}: worst |x - q d| - bound = {slack.max():.3e}")
        assert np.all(slack <= 0), np.argwhere(slack > 0)[:4]


# Q8 against f16 logits, max|L2 - L1| / max|L1|: MEASURED on correct code 3.446e-3, 1.396e-2, 2.843e-3 (profiles/kv_q8.md), times a 2x margin
E8_16 = {"tiny-hd128": 6.9e-3, "tiny-qwen2": 2.8e-2, "tiny-qwen2-g7": 5.7e-3}


@pytest.mark.parametrize("shape", ["tiny-hd128", "tiny-qwen2", "tiny-qwen2-g7"])
def test_end_to_end_against_the_f16_and_the_f32_cache(ca, dev, shape):
    """70 prompt tokens in passes of 32, then 8 decode steps, with the Q8, the f16 and the f32 cache; L0 = the f32-cache logits,
    e8 = max|L2 - L0| / max|L0|, e16 = max|L1 - L0| / max|L0|: e8 <= 32 max(e16, 1e-6) (the step ratio 2^(11-8) = 8, times 4: a Q8
    block's error scales with the block maximum, about 2.7 elements' worth for 32 Gaussian values).  The f32 cache pairs head h with
    kv head h % n_kv, the f16 and Q8 caches with h / group (the reference's own pairings), so on these GQA shapes e8 and e16 both carry
    that difference (measured ratio 0.99 .. 1.02) and the bound above cannot fail.  What can: the Q8 logits against the f16 ones, which
    share a pairing -- 0 < e8_16 <= E8_16[shape], the measured value re-derived with a 2x margin (0: value 2 would be the f16 cache; a
    wrong plane, layer or kernel form gives errors of the order of the logits).  And the Q8 context once more with NaN patterns in the
    cache tail, both planes, the step's scratch and the pass's row buffers -- the staging rows among them -- before every launch group:
    bit-identical logits."""
    def run(kv, poison):
        s, r = context(ca, dev, shape, kv, prefill_chunk=32)
        toks = tokens_for(s, 78, salt=5)
        r.prefill(toks[:32])
        lg = []
        for i in [None] + list(range(70, 78)):
            if poison:
                r.debug_poison(7, 0x7E00, 0x7FC00000)
            lg.append(np.array(r.prefill(toks[32:70]) if i is None else r.forward(toks[i], i)).copy())
        return np.concatenate(lg)

    logits = {kv: run(kv, False) for kv in (2, 1, 0)}
    assert all(np.all(np.isfinite(v)) for v in logits.values())
    assert np.array_equal(run(2, True).view(np.uint32), logits[2].view(np.uint32))
    e8, e16, e8_16 = rel_err(logits[2], logits[0]), rel_err(logits[1], logits[0]), rel_err(logits[2], logits[1])
    print(f"{shape}: e8 {e8:.3e}, e16 {e16:.3e}, ratio {e8 / max(e16, 1e-6):.2f}; q8 against f16 {e8_16:.3e} of max|logit|")
    assert e8 <= 32 * max(e16, 1e-6), (e8, e16)
    assert 0 < e8_16 <= E8_16[shape], e8_16


@pytest.mark.parametrize("shape,kv,kw,strict,kind", [("tiny-hd128", 2, {}, True, 9), ("tiny-hd128", 2, {"tp_size": 2}, False, 9),
                                                     ("tiny-gemma", 2, {}, False, 9), ("tiny-hd128", 2, {"extra_flags": 64}, False, 9),
                                                     ("tiny-hd128", 3, {}, False, 5),
                                                     ("tiny-gqa", 1, {}, False, "kv16"), ("tiny-gqa", 0, {}, False, "kv32")])
def test_what_create_refuses_and_what_it_leaves_alone(ca, shape, kv, kw, strict, kind):
    """kind 9: NotImplemented (strict device, tensor parallelism, head_dim 256, NO_LONG_ATTENTION = 64); 5: BadInput; a string: the plan
    of cache kind 0 / 1 equals the recorded one (tests/golden/step_plan_mi355x.json)"""
    dev = ca.HipTensorDevice(0, False, 0, strict, "lazy")
    model = synth.build_model(synth.SHAPES[shape], synth.Q4_0, seed=3)
    conf, w = synth.to_hip(model, dev)
    if isinstance(kind, str):
        with open(GOLDEN) as f:
            want = json.load(f)[f"tiny-gqa/Q4_0/fast/{kind}/seq64"]
        assert ca.debug_step_plan(conf, w, dev, 64, kv) == want
        return
    with pytest.raises(ca.CrabmlError) as e:
        ca.HipLlamaRunner(conf, w, dev, 64, kv, **kw)
    assert f"ErrorKind({kind})" in str(e.value), str(e.value)
