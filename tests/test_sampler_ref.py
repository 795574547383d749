"""CPU pins of tests/sampler_ref.py (the numpy restatement of Llama2Sampler, crabml-llama2/src/sampler.rs) with hand-worked
cases, against a plain Python loop written the way sampler.rs reads, and the C++ host restatement (crabml_amd.sample_llama2,
host/llama2_runner.hpp: the host baseline of crabml_hip_llama_decode_sample) against both."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import sampler_ref as sr

F32 = np.float32


def loop_sample(logits, temperature, topp, coin):
    """sampler.rs:28-130 line by line on np.float32 scalars."""
    x = [F32(v) for v in logits]
    if temperature == 0.0:
        best = 0
        for i in range(1, len(x)):
            if not (x[best] > x[i]):
                best = i
        return best
    x = [v / F32(temperature) for v in x]
    mx = F32(np.nan)
    for v in x:
        mx = v if np.isnan(mx) else (mx if np.isnan(v) else max(mx, v))
    tab = sr.exp_table()
    s = F32(0.0)
    e = []
    for v in x:
        h = int(o.f32_to_f16_bits(np.array([v - mx], dtype=F32))[0])
        ev = F32(o.f16_bits_to_f32(np.array([tab[h]], dtype=np.uint16))[0])
        e.append(ev)
        s = F32(s + ev)
    p = [F32(v / s) for v in e]
    cutoff = F32(F32(1.0) - F32(topp)) / F32(len(p) - 1)
    pi = [(p[i], i) for i in range(len(p)) if p[i] >= cutoff]
    pi = sorted(pi, key=lambda t: t[0])  # stable, ascending
    cum, last = F32(0.0), len(pi) - 1
    for k, (pv, _) in enumerate(pi):
        cum = F32(cum + pv)
        if cum > F32(topp):
            last = k
            break
    r = F32(F32(coin) * cum)
    cdf = F32(0.0)
    for pv, i in pi[: last + 1]:
        cdf = F32(cdf + pv)
        if cdf > r:
            return i
    return pi[last][1]


def test_temperature_zero_is_the_last_maximum():
    lg = np.array([1.0, 3.0, -2.0, 3.0, 2.0], dtype=F32)
    assert sr.sample(lg, 0.0, 0.9, 0.5) == 3
    assert loop_sample(lg, 0.0, 0.9, 0.5) == 3


def test_candidates_are_sorted_ascending_and_ties_stay_in_index_order():
    lg = np.array([0.0, 0.0, -1.0, 0.0, -3.0], dtype=F32)
    order, cums = sr.nucleus(lg, 1.0, 1.0)
    assert order.tolist() == [4, 2, 0, 1, 3]
    assert np.all(np.diff(cums) >= 0)
    # topp = 1: the walk never exceeds it before the end, so the last coin lands on the last (largest, latest) element
    assert sr.sample(lg, 1.0, 1.0, 0.9999) == 3


def test_the_element_that_crosses_topp_is_included():
    lg = np.log(np.array([0.05, 0.1, 0.15, 0.2, 0.22, 0.28], dtype=np.float64)).astype(F32)
    order, cums = sr.nucleus(lg, 1.0, 0.6)  # cutoff (1 - 0.6) / 5 = 0.08 drops token 0
    assert order.tolist() == [1, 2, 3, 4, 5]
    assert sr.last_index(cums, 0.6) == 3  # 0.1 + 0.15 + 0.2 + 0.22 > 0.6: token 4 ends the nucleus and is in it
    assert sr.sample(lg, 1.0, 0.6, 0.999) == 4
    assert loop_sample(lg, 1.0, 0.6, 0.999) == 4
    # ascending quirk: the most likely token (5) is never drawn
    assert all(sr.sample(lg, 1.0, 0.6, c) != 5 for c in np.linspace(0, 0.999, 50))


def test_topp_at_least_one_samples_the_whole_vocabulary():
    lg = np.array([0.0, -30.0, 1.0, 0.5], dtype=F32)  # e(-30 - 1) rounds to 0 in f16: p = 0 is a candidate too
    p, keys = sr.softmax_keys(lg, 1.0)
    assert keys[1] == 0 and p[1] == 0.0
    for topp in (1.0, 1.5):
        order, _ = sr.nucleus(lg, 1.0, topp)
        assert order.tolist() == [1, 0, 3, 2]
        for c in (0.0, 0.3, 0.7, 0.999):
            assert sr.sample(lg, 1.0, topp, c) == loop_sample(lg, 1.0, topp, c)
    assert sr.sample(lg, 1.0, 1.0, 0.0) == 0  # cdf > 0 first at the smallest positive probability


def test_rounding_fallback_takes_the_last_index():
    # r = coin * cumulative can equal the last running sum only with subnormal probabilities: nothing exceeds it
    tiny = np.array([np.finfo(F32).smallest_subnormal], dtype=F32)
    assert sr.topp_walk(tiny, 0.9, 0.99) == 0
    two = np.array([0.0, np.finfo(F32).smallest_subnormal], dtype=F32)
    assert sr.topp_walk(two, 0.9, 0.99) == 1


def test_restatement_equals_a_plain_loop_bit_for_bit():
    rng = np.random.default_rng(7)
    for trial in range(60):
        n = int(rng.integers(2, 40))
        lg = (rng.standard_normal(n) * rng.choice([0.5, 2.0, 6.0])).astype(F32)
        if trial % 5 == 0:
            lg[rng.integers(0, n, size=n // 2)] = lg[0]  # exact ties
        T = float(rng.choice([0.0, 0.5, 0.8, 1.0, 1.7]))
        topp = float(rng.choice([0.05, 0.5, 0.9, 0.95, 1.0, 1.2]))
        for coin in rng.random(6).astype(F32):
            try:
                want = loop_sample(lg, T, topp, coin)
            except IndexError:  # n0 == 0: the reference underflows n0 - 1
                with pytest.raises(sr.NoSample):
                    sr.sample(lg, T, topp, coin)
                continue
            assert sr.sample(lg, T, topp, coin) == want, (trial, T, topp, coin)


def test_neighbourhood_holds_the_exact_token():
    rng = np.random.default_rng(3)
    lg = (rng.standard_normal(5000) * 2).astype(F32)
    for coin in rng.random(64).astype(F32):
        tok = sr.sample(lg, 1.0, 0.9, coin)
        nb = sr.neighbourhood(lg, 1.0, 0.9, coin, 0.0)
        assert tok in nb
        assert tok in sr.neighbourhood(lg, 1.0, 0.9, coin, 1e-3)


def test_host_cpp_sampler_equals_the_restatement():
    import crabml_amd as ca
    rng = np.random.default_rng(11)
    cases = [rng.standard_normal(257).astype(F32) * 3, np.zeros(1000, dtype=F32), (rng.standard_normal(128256) * 2).astype(F32)]
    for lg in cases:
        for T, topp in [(0.0, 0.9), (1.0, 0.9), (0.8, 1.0), (1.3, 0.5)]:
            for coin in rng.random(5).astype(F32):
                assert ca.sample_llama2(lg, T, topp, float(coin)) == sr.sample(lg, T, topp, coin)
    with pytest.raises(ca.CrabmlError):
        ca.sample_llama2(np.array([1.0, np.nan], dtype=F32), 1.0, 0.9, 0.5)
