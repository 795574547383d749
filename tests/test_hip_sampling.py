"""Temperature / top-p sampling on the device (crabml_hip_llama_decode_sample, crabml_hip_debug_sample; sampler.hpp) against
tests/sampler_ref.py, the numpy restatement of Llama2Sampler (crabml-llama2/src/sampler.rs).

Strict-order device: the tokens are the reference's bit for bit (the oracle's logits + sampler_ref).  Fast device: the
softmax sum and the running sums are parallel, so a token must lie in sampler_ref's +-DELTA neighbourhood of the coin
(DESIGN.md 2.2), and equal the reference's wherever that neighbourhood is one token."""
import math
import os

import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import sampler_ref as sr
from tests.helpers import to_oracle

pytestmark = pytest.mark.gpu
F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "tinyllamas-stories-260k-f32.gguf")
BOS = 1
# the fast tier's bound on |its running sum - the reference's sequential one|: the reference's own f32
# running sums drift up to 1.0e-3 from the exact ones over 128 256 flat candidates; the parallel sums stay within ~1e-6
DELTA = 2e-3


def coins_for(seed, n):
    return np.random.default_rng(seed).random(n, dtype=np.float32)


def runner(ca, model_or_path, strict, seq_len=256, kv_f16=True, **kw):
    dev = ca.HipTensorDevice(0, False, 0, strict)
    if isinstance(model_or_path, str):
        gf = ca.GGUFFile(model_or_path)
        conf = gf.load_config()
        w = gf.load_weights(conf, dev)
    else:
        conf, w = synth.to_hip(model_or_path, dev)
    return dev, ca.HipLlamaRunner(conf, w, dev, seq_len, kv_f16, **kw)


def oracle_sampled(conf_w, seq_len, kv_f16, token, coins, temperature, topp):
    odev, conf, w = conf_w
    r = o.OracleLlamaRunner(conf, w, odev, seq_len, kv_f16)
    ids = []
    for pos, coin in enumerate(coins):
        lg = r.forward([token], pos).copy()
        token = sr.sample(lg, temperature, topp, coin)
        ids.append(token)
    return ids


def oracle_of_fixture():
    from tests.helpers import read_gguf_py
    model, _ = read_gguf_py(FIXTURE)
    odev = o.OracleDevice(thread_num=2, use_avx2=False)
    conf, w = to_oracle(model, odev)
    return odev, conf, w


@pytest.mark.parametrize("temperature", [0.8, 1.0])
@pytest.mark.parametrize("topp", [0.9, 1.0])
def test_strict_sampler_equals_the_reference_on_the_real_file(ca, temperature, topp):
    """The file's shape (hidden_dim 172) is not one the fused decode context takes, so its strict logits come from
    Llama2Runner<HipTensor> (bit-identical to the oracle's, test_real_fixture.py) and each token from the decode step's
    sampler kernels through crabml_hip_debug_sample: 100 sampled steps from BOS, token for token."""
    coins = coins_for(100 + int(temperature * 10) + int(topp * 100), 100)
    want = oracle_sampled(oracle_of_fixture(), 256, True, BOS, coins, temperature, topp)
    dev = ca.HipTensorDevice(0, False, 0, True)
    gf = ca.GGUFFile(FIXTURE)
    conf = gf.load_config()
    r = ca.Llama2Runner(conf, gf.load_weights(conf, dev), dev, 256, True)
    tok, got = BOS, []
    for pos, coin in enumerate(coins):
        tok = dev.debug_sample(r.forward([tok], pos), temperature, topp, float(coin))
        got.append(tok)
    assert got == want
    assert len(set(got)) > 20  # sampled, not a greedy loop


@pytest.mark.parametrize("fmt", ["Q4_0", "Q4_K"])
def test_strict_decode_sample_equals_the_reference_at_the_8b_shape(ca, fmt):
    model = synth.build_model(synth.SHAPES["llama3-8b"], synth.TYPE_BY_NAME[fmt], seed=81, n_layers=2)
    odev = o.OracleDevice(thread_num=8)
    conf, w = to_oracle(model, odev)
    coins = coins_for(7, 16)
    want = oracle_sampled((odev, conf, w), 64, True, BOS, coins, 1.0, 0.9)
    _, r = runner(ca, model, True, seq_len=64)
    got = r.decode_sample(BOS, 16, 1.0, 0.9, coins)
    assert list(got) == want


def crafted():
    rng = np.random.default_rng(5)
    ninf = (rng.standard_normal(4000) * 2).astype(F32)
    ninf[rng.random(4000) < 0.5] = -np.inf
    dom = np.zeros(3000, dtype=F32)
    dom[1234] = 15.0
    return {
        "ties": (rng.integers(0, 4, 1000).astype(F32), 1.0, 0.9),
        "flat": (np.zeros(5000, dtype=F32), 1.0, 0.9),
        "dominant": (dom, 1.0, 0.9),
        "neg_inf": (ninf, 0.8, 0.95),
        "vocab_128256": ((rng.standard_normal(128256) * 2).astype(F32), 1.0, 0.9),
        "whole_vocab": ((rng.standard_normal(2000) * 3).astype(F32), 1.2, 1.0),
    }


@pytest.mark.parametrize("case", list(crafted()))
def test_debug_sample_strict_is_bit_exact_on_crafted_logits(ca, case):
    lg, T, topp = crafted()[case]
    dev = ca.HipTensorDevice(0, False, 0, True)
    coins = coins_for(9, 256)
    for coin in coins:
        assert dev.debug_sample(lg, T, topp, float(coin)) == sr.sample(lg, T, topp, coin), (case, coin)
    assert dev.debug_sample(lg, 0.0, 0.9, 0.5) == o.argmax_last(lg)
    if case == "flat":  # ascending quirk: the nucleus is the LOWEST indices of a flat distribution
        assert max(dev.debug_sample(lg, T, topp, float(c)) for c in coins) < 4600


@pytest.mark.parametrize("case", list(crafted()))
def test_debug_sample_fast_is_within_the_stated_bound(ca, case):
    lg, T, topp = crafted()[case]
    dev = ca.HipTensorDevice(0, False, 0, False)
    coins = coins_for(10, 4096 if case == "vocab_128256" else 512)
    for coin in coins:
        tok = dev.debug_sample(lg, T, topp, float(coin))
        nb = sr.neighbourhood(lg, T, topp, coin, DELTA)
        assert tok in nb, (case, coin, tok, sorted(nb)[:8])
        if len(nb) == 1:
            assert tok == sr.sample(lg, T, topp, coin)
    assert dev.debug_sample(lg, 0.0, 0.9, 0.5) == o.argmax_last(lg)


@pytest.mark.parametrize("strict", [True, False])
def test_a_coin_exactly_on_a_cdf_boundary(ca, strict):
    dev = ca.HipTensorDevice(0, False, 0, strict)
    lg = np.zeros(4, dtype=F32)  # p = 0.25 each, exactly; topp = 1: cumulative 1.0
    for coin, want in [(0.0, 0), (0.25, 1), (0.5, 2), (0.75, 3)]:  # r = a running sum: the NEXT element wins (cdf > r)
        assert sr.sample(lg, 1.0, 1.0, coin) == want
        assert dev.debug_sample(lg, 1.0, 1.0, coin) == want


def test_debug_sample_rejects_what_the_reference_panics_on(ca):
    dev = ca.HipTensorDevice(0, False, 0, False)
    lg = np.zeros(16, dtype=F32)
    for bad in ([np.nan] + [0.0] * 15, [np.inf] + [0.0] * 15):
        with pytest.raises(ca.CrabmlError, match="nothing to sample"):
            dev.debug_sample(np.array(bad, dtype=F32), 1.0, 0.9, 0.5)
    assert dev.debug_sample(lg, 1.0, 0.9, 0.5) == sr.sample(lg, 1.0, 0.9, F32(0.5))  # the device is still fine


def test_fast_decode_sample_against_forward_steps(ca):
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=21)
    coins = coins_for(12, 40)
    _, a = runner(ca, model, False, seq_len=64)
    toks = a.decode_sample(BOS, 40, 1.0, 0.9, coins)
    _, b = runner(ca, model, False, seq_len=64)  # (near-flat synthetic logits: most neighbourhoods hold several tokens)
    prev = BOS
    for s, coin in enumerate(coins):
        lg = b.forward(prev, s)
        nb = sr.neighbourhood(lg, 1.0, 0.9, coin, DELTA)
        assert toks[s] in nb, (s, toks[s], sorted(nb)[:8])
        if len(nb) == 1:
            assert toks[s] == sr.sample(lg, 1.0, 0.9, coin)
        prev = toks[s]


@pytest.mark.parametrize("strict", [True, False])
def test_temperature_zero_is_decode_greedy(ca, strict):
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=22)
    _, a = runner(ca, model, strict, seq_len=64)
    _, b = runner(ca, model, strict, seq_len=64)
    assert list(a.decode_sample(BOS, 12, 0.0, 0.9, coins_for(1, 12))) == list(b.decode_greedy(BOS, 12))


@pytest.mark.parametrize("strict", [True, False])
def test_graph_replay_equals_eager_launches(ca, strict):
    # attn_long_from = 8: the 20 steps cross into the long-context attention variant, so two sampled graphs are captured
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=23)
    coins = coins_for(13, 20)
    _, g = runner(ca, model, strict, seq_len=64, attn_long_from=8)
    _, e = runner(ca, model, strict, seq_len=64, use_graph=False, attn_long_from=8)
    assert list(g.decode_sample(BOS, 20, 1.0, 0.9, coins)) == list(e.decode_sample(BOS, 20, 1.0, 0.9, coins))


def test_calls_continue_from_the_cache(ca):
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=24)
    odev = o.OracleDevice(thread_num=4)
    oconf, ow = to_oracle(model, odev)
    orr = o.OracleLlamaRunner(oconf, ow, odev, 64, True)
    _, r = runner(ca, model, True, seq_len=64)
    c1, c2 = coins_for(14, 5), coins_for(15, 4)
    t1 = list(r.decode_sample(BOS, 5, 1.0, 0.9, c1))
    assert r.kv_cache_len() == 5
    t2 = list(r.decode_greedy(t1[-1], 3))
    assert r.kv_cache_len() == 8
    r.forward(t2[-1], 8)
    assert r.kv_cache_len() == 9
    t3 = list(r.decode_sample(t2[-1], 4, 0.9, 0.95, c2))
    assert r.kv_cache_len() == 13
    # the oracle through the same sequence of tokens and samplers
    want, tok, pos = [], BOS, 0
    for coin in c1:
        tok = sr.sample(orr.forward([tok], pos).copy(), 1.0, 0.9, coin)
        want.append(tok)
        pos += 1
    for _ in range(3):
        tok = o.argmax_last(orr.forward([tok], pos).copy())
        want.append(tok)
        pos += 1
    orr.forward([tok], pos)
    pos += 1
    for coin in c2:
        tok = sr.sample(orr.forward([tok], pos).copy(), 0.9, 0.95, coin)
        want.append(tok)
        pos += 1
    assert t1 + t2 + t3 == want


def test_errors(ca):
    from crabml_amd import tp as tp_mod
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=25)
    _, r = runner(ca, model, False, seq_len=16)
    ok = coins_for(16, 4)
    for coins, msg in [(np.array([0.1, 1.0, 0.2, 0.3], F32), "coin"), (np.array([0.1, -0.1, 0.2, 0.3], F32), "coin"),
                       (np.array([0.1, np.nan, 0.2, 0.3], F32), "coin")]:
        with pytest.raises(ca.CrabmlError, match=msg):
            r.decode_sample(BOS, 4, 1.0, 0.9, coins)
    for T, topp, msg in [(-1.0, 0.9, "temperature"), (math.nan, 0.9, "temperature"), (1.0, 0.0, "topp"), (1.0, -0.5, "topp"),
                         (1.0, math.nan, "topp")]:
        with pytest.raises(ca.CrabmlError, match=msg):
            r.decode_sample(BOS, 4, T, topp, ok)
    assert r.kv_cache_len() == 0  # nothing ran
    with pytest.raises(ca.CrabmlError, match="do not fit"):
        r.decode_sample(BOS, 17, 1.0, 0.9, coins_for(17, 17))
    r.decode_sample(BOS, 16, 1.0, 0.9, coins_for(18, 16))
    with pytest.raises(ca.CrabmlError, match="do not fit"):
        r.decode_sample(BOS, 1, 1.0, 0.9, coins_for(19, 1))
    dev = ca.HipTensorDevice(0, False, 0, False)
    conf, w = synth.to_hip(tp_mod.shard_model(model, 2, 0, True), dev)
    rank = ca.HipLlamaRunner(conf, w, dev, 16, True, True, True, 2, 0)
    with pytest.raises(ca.CrabmlError, match="tensor-parallel"):
        rank.decode_sample(BOS, 4, 1.0, 0.9, ok)
