"""k_attn_flash (+ k_attn_flash_merge, and the ticket form) by itself, with dead rows behind the live positions: the K and V of a kv
head lie `seq_cap = seq + 37` rows apart, as in a decode context whose cache is longer than what has been appended, and the 37 rows
past `seq` hold a pattern.  The kernel issues whole groups of row loads per slice and clamps them inside the allocation; none of what
those loads bring may reach the output.  Every comparison is bit for bit: the pattern tail against a zero tail, both launch forms,
and the zero tail against the call without any tail (seq_cap == seq: the cache row stride differs, nothing else)."""
import numpy as np
import pytest

from tests.poison import PATTERNS, release_devices, same  # noqa: F401 (autouse fixture)

pytestmark = pytest.mark.gpu

TAIL = 37
# 1 .. a few rows (one slice, ragged row groups), either side of the 128-row slice threshold, several slices with a ragged last one
SEQS = (1, 2, 3, 5, 8, 31, 127, 128, 129, 257, 1000)


@pytest.mark.parametrize("n_heads,n_kv,hd", [(32, 8, 128), (8, 1, 64), (8, 2, 256), (14, 2, 64)])
def test_rows_past_the_live_positions_never_reach_the_output(ca, n_heads, n_kv, hd):
    dev = ca.HipTensorDevice(0)
    rng = np.random.default_rng(1000 * n_heads + hd)
    for seq in SEQS:
        q = (rng.standard_normal(n_heads * hd) / np.sqrt(hd)).astype(np.float32)
        k = rng.standard_normal((n_kv, seq, hd)).astype(np.float16).view(np.uint16)
        v = rng.standard_normal((n_kv, seq, hd)).astype(np.float16).view(np.uint16)
        cap = seq + TAIL

        def with_tail(a, fill):
            t = np.full((n_kv, cap, hd), fill, dtype=np.uint16)
            t[:, :seq] = a
            return t.reshape(-1)

        for slices in (1, 7, 32):
            ctx = (n_heads, n_kv, hd, seq, slices)
            tight, tight_ticket = dev.debug_flash_attention(q, k.reshape(-1), v.reshape(-1), n_heads, n_kv, hd, seq, slices)
            zero, zero_ticket = dev.debug_flash_attention(q, with_tail(k, 0), with_tail(v, 0), n_heads, n_kv, hd, seq, slices, seq_cap=cap)
            assert np.all(np.isfinite(zero)), ctx
            assert same(zero, tight) and same(zero_ticket, tight_ticket), (ctx, "a zero tail against no tail")
            assert same(zero, zero_ticket), (ctx, "merge launch against the ticket form")
            for f16 in sorted({p[0] for p in PATTERNS.values()}):
                name = hex(f16)
                got, got_ticket = dev.debug_flash_attention(q, with_tail(k, f16), with_tail(v, f16), n_heads, n_kv, hd, seq, slices,
                                                            seq_cap=cap)
                assert same(got, zero), (ctx, name, "one of the two launch forms")
                assert same(got_ticket, zero), (ctx, name, "the other launch form")
