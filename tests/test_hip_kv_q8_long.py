"""Q8 contexts past 32768 positions (up to 131072) and their decode attention on the matrix cores, k_attn_flash_mm:
the kernel alone against float64 over the dequantized planes, junk behind the live cache, the depth, two contexts end to end, and what
create still refuses.  Bound of the kernel: 1.5e-3 of max|out|, what the f16-probability matrix-core attention of the prompt pass is
held to (tests/test_hip_kv_q8.py)."""
import numpy as np
import pytest

from crabml_amd import synth
from crabml_amd import tp as tp_mod
from tests.helpers import FAST_TOL
from tests.poison import release_devices, tokens_for  # noqa: F401 (autouse fixture)
from tests.test_hip_kv_q8 import dequant, f64_attention, quantize, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(8, 2, 128), (7, 1, 128), (6, 2, 64), (8, 1, 64), (2, 2, 64)]
# the kernel's constants: FLASH_MM_BN = 32 positions per step; FLASH_MM_NW = 8 waves take steps round-robin, so a wave's second step
# starts at 256; FLASH_MM_MIN_ROWS = 256 live positions per slice: the second slice appears at 257, the third at 513
SEQS = [1, 2, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1000, 2049]
MOST = 32  # slices
LONG, FROM = 32768 + 256, 256  # FLASH_MM_FROM (fused.hip)
BOUND = 1.5e-3


@pytest.fixture(scope="module")
def dev(ca):
    return ca.HipTensorDevice(0)


def mm_case(dev, n_heads, n_kv, hd, seq, slices, spread=1.0, kind="normal", pad=0, fills=()):
    """tests/test_hip_kv_q8.py's decode_case for the new hook; fills: (int8 byte, scale bits) patterns behind the live cache, each
    run held to the clean run's bits"""
    rng = np.random.default_rng(1000 * n_heads + 10 * hd + seq)
    q = (rng.standard_normal(n_heads * hd) * spread / np.sqrt(hd)).astype(np.float32)
    k = rng.standard_normal((n_kv, seq, hd)).astype(np.float32)
    v = rng.standard_normal((n_kv, seq, hd)).astype(np.float32)
    if kind == "spike":
        k[:, seq // 2] *= 6.0
    elif kind == "ties":
        k[:] = k[:, :1]
    elif kind == "dead":
        k[:, : seq - 1] = -np.abs(k[:, : seq - 1]) * 3
        q = np.abs(q) * 8
    (kq, kd), (vq, vd) = quantize(k), quantize(v)

    def run(qfill, dfill):
        planes = []
        for a, fill in ((kq, qfill), (kd, dfill), (vq, qfill), (vd, dfill)):
            p = np.full((n_kv, seq + pad, a.shape[-1]), fill, dtype=np.uint16 if a.dtype == np.uint16 else np.uint8).view(a.dtype)
            p[:, :seq] = a
            planes.append(p.reshape(-1))
        got, again = dev.debug_flash_attention_q8_mm(q, *planes, n_heads, n_kv, hd, seq, slices)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32))  # the second run on the same scratch
        return got

    got = run(0, 0)
    assert np.all(np.isfinite(got))
    for qfill, dfill in fills:
        assert np.array_equal(run(qfill, dfill).view(np.uint32), got.view(np.uint32)), (hex(qfill), hex(dfill))
    err = rel_err(got, f64_attention(q, dequant(kq, kd), dequant(vq, vd), 1, seq - 1, False))
    print(f"flash mm q8 vs float64, {n_heads}/{n_kv} x {hd}, seq {seq}, {slices} slices, {kind}: {err:.2e} of max|out|")
    return err


@pytest.mark.parametrize("slices", [1, 7, MOST])
@pytest.mark.parametrize("seq", SEQS)
@pytest.mark.parametrize("n_heads,n_kv,hd", SHAPES)
def test_kernel_equals_float64_over_the_dequantized_planes(dev, n_heads, n_kv, hd, seq, slices):
    assert mm_case(dev, n_heads, n_kv, hd, seq, slices) <= BOUND


@pytest.mark.parametrize("kind", ["spike", "ties", "dead"])
def test_kernel_merge_edge_cases(dev, kind):
    assert mm_case(dev, 8, 2, 128, 3000, MOST, spread=4.0, kind=kind) <= BOUND


@pytest.mark.parametrize("n_heads,n_kv,hd", SHAPES)
def test_junk_behind_the_live_cache_changes_no_bit(dev, n_heads, n_kv, hd):
    assert mm_case(dev, n_heads, n_kv, hd, 777, 7, pad=37, fills=((0xFF, 0xFFFF), (0x7F, 0x7C00), (0x80, 0x7BFF))) <= BOUND


@pytest.mark.parametrize("slices", [1, MOST])
@pytest.mark.parametrize("seq", [32768 + 5, 131072])
def test_kernel_at_depth(dev, seq, slices):
    assert mm_case(dev, 2, 1, 64, seq, slices) <= BOUND


def runner(ca, dev, shape, seq_len, kv=2, **kw):
    model = synth.build_model(synth.SHAPES[shape], synth.Q4_0, seed=61)
    conf, w = synth.to_hip(model, dev)
    return model.shape, ca.HipLlamaRunner(conf, w, dev, seq_len, kv, **kw)


@pytest.mark.parametrize("shape", ["tiny-hd128", "tiny-qwen2-g7"])
def test_a_long_context_runs_the_new_kernel_and_agrees_with_a_short_one(ca, dev, shape, monkeypatch):
    """Create succeeds (refused before this kernel existed); the tap names k_attn_flash (16 + 2, its ticket form) below FROM cached positions and the new
    kernel (16 + 3) from there.  Then, the lab hook putting every decode step on the new kernel: 70 prompt tokens in passes of 32 and 8
    decode steps against the same in a 4096-position Q8 context, within e = that context against the f16 one (the quantization's own
    effect, the e8_16 of tests/test_hip_kv_q8.py, measured here)."""
    s, r = runner(ca, dev, shape, LONG)
    toks = tokens_for(s, FROM + 1, salt=5)
    r.prefill(toks[: FROM - 2])
    assert [r.debug_tap(toks[p], p, 0)["plan"]["attn_variant"] for p in (FROM - 2, FROM - 1, FROM)] == [16 + 2, 16 + 3, 16 + 3]

    def run(seq_len, kv):
        _, x = runner(ca, dev, shape, seq_len, kv, prefill_chunk=32)
        x.prefill(toks[:32])
        lg = [np.array(x.prefill(toks[32:70])).copy()] + [np.array(x.forward(toks[i], i)).copy() for i in range(70, 78)]
        if seq_len == LONG:
            assert x.debug_tap(toks[78], 78, 0)["plan"]["attn_variant"] == 16 + 3
        return np.concatenate(lg)

    q8, f16 = run(4096, 2), run(4096, 1)
    monkeypatch.setenv("CRABML_HIP_TEST_HOOKS", "1")
    monkeypatch.setenv("CRABML_HIP_ATTN_MM_FROM", "1")
    mm = run(LONG, 2)
    e, err = rel_err(q8, f16), rel_err(mm, q8)
    print(f"{shape}: new kernel against k_attn_flash {err:.3e}, q8 against f16 {e:.3e} of max|logit|")
    assert np.all(np.isfinite(mm)) and 0 < err <= e, (err, e)


@pytest.mark.parametrize("shape", ["tiny-hd128", "tiny-qwen2-g7"])
def test_decode_past_32768_positions_agrees_with_the_prompt_pass(ca, dev, shape):
    n = 32768 + 100
    got = []
    for decode in (True, False):
        s, r = runner(ca, dev, shape, LONG, prefill_chunk=1024)
        toks = tokens_for(s, n + 3, salt=7)
        r.prefill(toks[:n])
        got.append((np.array([r.forward(toks[i], i) for i in range(n, n + 3)][-1] if decode else r.prefill(toks[n:])).copy(),
                    [np.asarray(a).copy() for a in r.debug_kv_q8_read(0, 32768, 103)]))
    err = rel_err(got[0][0], got[1][0])
    print(f"{shape}: token loop against prompt pass at position {n + 2}: {err:.3e} of max|logit|")
    assert np.all(np.isfinite(got[0][0])) and err <= FAST_TOL["FLASH:Q4_0"][1], err
    assert all(np.array_equal(a, b) for a, b in zip(got[0][1], got[1][1]))


@pytest.mark.parametrize("seq_len,strict,tp,limit", [(131073, False, 1, "(limit 131072)"), (32769, True, 1, "(limit 32768)"),
                                                     (32769, False, 2, "(limit 32768)")])
def test_what_create_still_refuses(ca, seq_len, strict, tp, limit):
    d = ca.HipTensorDevice(0, False, 0, strict, "lazy")
    model = synth.build_model(synth.SHAPES["tiny-hd128"], synth.Q4_0, seed=61)
    conf, w = synth.to_hip(tp_mod.shard_model(model, 2, 0, True) if tp == 2 else model, d)
    with pytest.raises(ca.CrabmlError) as e:
        ca.HipLlamaRunner(conf, w, d, seq_len, 2, True, True, tp, 0)  # (use_graph, prefetch, tp_size, tp_rank)
    assert "ErrorKind(9)" in str(e.value) and limit in str(e.value) and "more positions than the limit" in str(e.value), str(e.value)
