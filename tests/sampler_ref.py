"""An independent numpy restatement of Llama2Sampler (crabml-llama2/src/sampler.rs:28-130) with the coin as an argument,
for the sampler tests (test infrastructure: may import oracle/).

  temperature 0      sample_argmax: the LAST maximum (sampler.rs:109-116)
  otherwise          x / T (f32 division); softmax with max = fold(NaN, f32::max), e = exp_f32_cached(x - max) through the
                     oracle's exp table (cpu_device.rs:108-115), a sequential f32 sum in index order, p = e / sum;
                     then sample_topp -- also when topp >= 1, because sample's call of sample_multi discards its result
                     (sampler.rs:46-49): candidates p >= (1 - topp) / (n - 1), stably sorted ASCENDING, cumulative until it
                     exceeds topp (that element included), r = coin * cumulative, the first cdf > r, else prob_index[last_idx].

np.cumsum(.., dtype=np.float32) accumulates left to right in f32, so it is the reference's loops' running sums."""
import numpy as np

from oracle import oracle as o

F32 = np.float32
_EXP = None


def exp_table() -> np.ndarray:
    global _EXP
    if _EXP is None:
        t = np.empty(65536, dtype=np.uint16)
        o.lib().co_init_exp_cache(o._p(t))
        _EXP = t
    return _EXP


def softmax_keys(logits, temperature):
    """(p, keys): the probabilities and the f16 bits of e (the device's sort keys)."""
    x = np.ascontiguousarray(logits, dtype=F32) / F32(temperature)
    mx = np.fmax.reduce(x) if x.size else F32(np.nan)  # f32::max ignores a NaN operand
    keys = exp_table()[o.f32_to_f16_bits((x - mx).astype(F32))]
    e = o.f16_bits_to_f32(keys)
    total = np.cumsum(e, dtype=F32)[-1]
    return (e / total).astype(F32), keys


class NoSample(Exception):
    """The reference panics here (NaN in the sort, or n0 == 0 underflowing n0 - 1)."""


def nucleus(logits, temperature, topp):
    """(order, cums): the candidates in the reference's sorted order and their running f32 sums."""
    p, keys = softmax_keys(logits, temperature)
    if np.any(keys > 0x3C00):
        raise NoSample("a NaN / +inf probability")
    n = p.size
    cutoff = (F32(1.0) - F32(topp)) / F32(n - 1)
    idx = np.nonzero(p >= cutoff)[0]
    if idx.size == 0:
        raise NoSample("no candidate")
    order = idx[np.argsort(p[idx], kind="stable")]
    return order, np.cumsum(p[order], dtype=F32)


def last_index(cums, topp):
    over = np.nonzero(cums > F32(topp))[0]
    return int(over[0]) if over.size else cums.size - 1


def topp_walk(sorted_p, topp, coin) -> int:
    """sample_topp's two loops over probabilities already in sorted order (sampler.rs:86-106): the position chosen."""
    cums = np.cumsum(np.asarray(sorted_p, dtype=F32), dtype=F32)
    last = last_index(cums, topp)
    r = F32(coin) * cums[last]
    hit = np.nonzero(cums[: last + 1] > r)[0]  # cdf walks the same elements in the same order: the same running sums
    return int(hit[0]) if hit.size else last  # else: prob_index[last_idx], "in case of rounding errors"


def sample(logits, temperature, topp, coin) -> int:
    if temperature == 0.0:
        return o.argmax_last(np.ascontiguousarray(logits, dtype=F32))
    p, _ = softmax_keys(logits, temperature)
    order, _ = nucleus(logits, temperature, topp)
    return int(order[topp_walk(p[order], topp, coin)])


def neighbourhood(logits, temperature, topp, coin, delta) -> set:
    """The tokens a sampler whose running sums are each within +-delta of the reference's can return for this coin: every
    element that can end the nucleus (its running sum within delta of crossing topp), and for each such end, every element
    up to it whose cdf interval meets [r - delta, r + delta] (and the end itself, the reference's rounding fallback)."""
    order, cums = nucleus(logits, temperature, topp)
    c = cums.astype(np.float64)
    prev = np.concatenate([[0.0], c[:-1]])
    t = float(F32(topp))
    ends = set(np.nonzero((c > t - delta) & (prev <= t + delta))[0].tolist())
    ends.add(last_index(cums, topp))
    if c[-1] <= t + delta:
        ends.add(c.size - 1)
    out = set()
    for L in ends:
        r = float(coin) * c[L]
        k = np.nonzero((c[: L + 1] >= r - delta) & (prev[: L + 1] <= r + delta))[0]
        out.update(int(order[i]) for i in k)
        if c[L] <= r + delta:
            out.add(int(order[L]))
    return out
