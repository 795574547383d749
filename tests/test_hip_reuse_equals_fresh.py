"""A reused context equals a fresh one, without any hook: a long run that crosses attn_long_from, reset(), then a short run on the
same context, held against a fresh context of the same configuration at every step -- logits, tokens and live cache rows, bit for
bit.  What a reuse could leave behind: cache rows past the short run's positions, the scratch of the long-context kernels, the
prompt pass's row buffers sized by a longer pass, the sampler's histogram and step counter, a tap's scratch and plan."""
import numpy as np
import pytest

from crabml_amd import synth
from tests.poison import EXACT_ATTENTION, cache_rows, release_devices, same, same_cache, tokens_for  # noqa: F401 (autouse fixture)

pytestmark = pytest.mark.gpu

BOS = 1
# (name, shape, format, K_M mix, strict device, flags): k_attn_flash, the exact long-context kernels, a K-quant body, both devices
CONTEXTS = [("flash", "tiny-gqa", "Q4_0", False, False, 0), ("exact", "tiny-gqa", "Q8_0", False, False, EXACT_ATTENTION),
            ("Q4_K_M", "tiny-gqa", "Q4_K", True, False, 0), ("Q4_1-hd128", "tiny-hd128", "Q4_1", False, False, 0),
            ("strict", "tiny-gqa", "Q4_0", False, True, 0), ("strict-Q4_K", "tiny-gqa", "Q4_K", False, True, 0)]


def setup(ca, ctx, seq, seed, long_from=8):
    name, shape, fmt, mix, strict, flags = ctx
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=seed, k_m_mix=mix)
    dev = ca.HipTensorDevice(0, False, 0, strict)
    conf, w = synth.to_hip(model, dev)
    return model.shape, lambda: ca.HipLlamaRunner(conf, w, dev, seq, True, extra_flags=flags, attn_long_from=long_from)


def short_decode(r, s, seq):
    """six teacher-forced steps with their logits, then six greedy steps from the device's own arg-max, then the live cache rows"""
    out = [r.forward(t, pos).copy() for pos, t in enumerate(tokens_for(s, 6, salt=2))]
    toks = list(r.decode_greedy(int(np.argmax(out[-1])), 6))
    return out, toks, cache_rows(r, s, True, 12, seq)


def assert_same_run(got, want, what):
    (lg, toks, cache), (wlg, wtoks, wcache) = got, want
    for i, (a, b) in enumerate(zip(lg, wlg)):
        assert same(a, b), f"{what}: logits of step {i} differ from a fresh context's"
    assert len(lg) == len(wlg) and toks == wtoks, (what, toks, wtoks)
    assert same_cache(cache, wcache), f"{what}: live cache rows differ from a fresh context's"


@pytest.mark.parametrize("ctx", CONTEXTS, ids=lambda c: c[0])
def test_short_decode_after_a_long_one(ca, ctx):
    s, mk = setup(ca, ctx, 64, seed=81)
    want = short_decode(mk(), s, 64)
    r = mk()
    for pos, t in enumerate(tokens_for(s, 60, salt=1)):  # 60 steps: the short form, then the long one from 8 cached positions
        r.forward_async(t, pos)
    r.reset()
    assert_same_run(short_decode(r, s, 64), want, f"{ctx[0]}, after 60 steps")
    r.reset()
    assert_same_run(short_decode(r, s, 64), want, f"{ctx[0]}, after a second reset")


@pytest.mark.parametrize("ctx", CONTEXTS, ids=lambda c: c[0])
def test_short_prefill_after_a_long_one(ca, ctx):
    s, mk = setup(ca, ctx, 256, seed=82)

    def short(r, n):
        lg = [r.prefill(tokens_for(s, n, salt=3)).copy()]
        for step in range(4):
            lg.append(r.forward(int(np.argmax(lg[-1])), n + step).copy())
        return lg, [int(np.argmax(x)) for x in lg], cache_rows(r, s, True, n + 4, 256)

    r = mk()
    r.prefill(tokens_for(s, 200, salt=1))
    for n in (40, 33, 17):  # the f16 GEMM's sizes and an int8 pass, each behind whatever the longer pass before it left
        r.reset()
        assert_same_run(short(r, n), short(mk(), n), f"{ctx[0]}, {n} rows after a longer pass")


@pytest.mark.parametrize("ctx", [CONTEXTS[0], CONTEXTS[2], CONTEXTS[4]], ids=lambda c: c[0])
def test_short_sampled_decode_after_a_long_one(ca, ctx):
    s, mk = setup(ca, ctx, 64, seed=83)
    rng = np.random.default_rng(5)
    long_coins, coins = rng.random(60).astype(np.float32), rng.random(12).astype(np.float32)

    def short(r):
        toks = list(r.decode_sample(BOS, 12, 1.0, 0.9, coins))
        return [r.forward(int(toks[-1]), 12).copy()], toks, cache_rows(r, s, True, 13, 64)

    want = short(mk())
    r = mk()
    r.decode_sample(BOS, 60, 0.8, 0.95, long_coins)  # other parameters, other coins, 60 steps on the step counter
    r.reset()
    assert_same_run(short(r), want, f"{ctx[0]}, sampled, after 60 sampled steps")
    r.reset()
    r.decode_greedy(BOS, 30)  # the greedy graphs in between
    r.reset()
    assert_same_run(short(r), want, f"{ctx[0]}, sampled, after 30 greedy steps")


@pytest.mark.parametrize("ctx", CONTEXTS[:4], ids=lambda c: c[0])
def test_short_runs_after_taps(ca, ctx):
    """a context that was tapped in between (debug_tap: an eager step with copies between its launches; debug_prefill_tap: a tapped
    pass) serves a short run as a fresh one does"""
    s, mk = setup(ca, ctx, 64, seed=84)
    want = short_decode(mk(), s, 64)
    r = mk()
    toks = tokens_for(s, 30, salt=1)
    for pos, t in enumerate(toks):
        if pos in (3, 20):  # one tap on the short form, one on the long form
            r.debug_tap(t, pos, 1)
        else:
            r.forward_async(t, pos)
    r.reset()
    assert_same_run(short_decode(r, s, 64), want, f"{ctx[0]}, after tapped steps")
    r.reset()
    r.debug_prefill_tap(tokens_for(s, 40, salt=4), 0)
    r.reset()
    assert_same_run(short_decode(r, s, 64), want, f"{ctx[0]}, after a tapped pass")
