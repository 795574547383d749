"""Shared pieces of the tests that hold the invariant of DESIGN.md 6: no launch's result depends on cache rows past the live
positions or on scratch bytes it did not write in the same step or pass (tests/test_hip_flash_poison.py, test_hip_step_poison.py,
test_hip_prefill_poison.py, test_hip_reuse_equals_fresh.py).  Every comparison of those files is bit for bit."""
import gc

import numpy as np
import pytest

# HipLlamaRunner.debug_poison's `what` (crabml_hip_llama_debug_poison, include/crabml_hip_debug.h)
CACHE_TAIL, STEP_SCRATCH, PASS_ROWS = 1, 2, 4

ZERO = (0x0000, 0x00000000)  # the baseline: what a fresh process mostly finds in its pages
# (f16 bits, f32 bits) -- NaN and the infinities catch "multiplied by zero instead of masked", the largest finite values catch "took
# part in a maximum or a sum".  The f32 side carries both the f16 value itself (65504) and f32's own largest finite value.
PATTERNS = {
    "nan": (0x7E00, 0x7FC00000),
    "+inf": (0x7C00, 0x7F800000),
    "-inf": (0xFC00, 0xFF800000),
    "+65504": (0x7BFF, 0x477FE000),
    "-65504": (0xFBFF, 0xC77FE000),
    "+max": (0x7BFF, 0x7F7FFFFF),
    "-max": (0xFBFF, 0xFF7FFFFF),
}

# flag bits (include/crabml_hip.h, include/crabml_hip_debug.h)
NO_LONG_ATTENTION, NO_TILE_ATTENTION, NO_STAGED_ATTENTION, Q8K_ATTN_PRODUCER, NO_PV_PRODUCER_WAVES = 64, 2048, 8192, 65536, 131072
PREFILL_INT8_GEMM, FLASH_TICKET, EXACT_ATTENTION = 524288, 2097152, 4194304


def variant_of(plan, pos):
    """the attention form that serves cache position `pos`, as CRABML_HIP_PLAN_ATTN_VARIANT names it: variant_of() of fused.hip over the
    words of debug_step_plan -- 0 one workgroup per head, 1 the exact long-context kernels, 16 + 1 k_attn_flash with the merge launch
    (or, plan["flash_ticket"], its ticket form throughout), 16 + 2 k_attn_flash with the merge inside the launch"""
    if not (plan["attn_long_ok"] and pos + 1 >= plan["attn_long_from"]):
        return 0
    v = 2 if plan["flash_ticket_until"] > 0 and pos + 1 < plan["flash_ticket_until"] else 1
    return v + (16 if plan["attn_flash"] else 0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def cache_rows(r, shape, kv_f16, n_rows, seq_len):
    """the live rows 0 .. n_rows - 1 of every layer's K and V cache, raw bytes"""
    out = []
    row = shape.head_dim * (2 if kv_f16 else 4)
    for layer in range(shape.n_layers):
        for v in (False, True):
            c = np.asarray(r.debug_kv(layer, v, kv_f16)).reshape(shape.n_kv_heads, seq_len, row)
            out.append(c[:, :n_rows].copy())
    return out


def same_cache(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def tokens_for(shape, n, salt=0):
    return [int((7 * i + 3 + 13 * salt) % shape.vocab) for i in range(n)]


@pytest.fixture(autouse=True)
def release_devices():
    """imported by the test files above: every device object of a test (one stream each) is gone before the next test starts -- a
    collected exception's traceback would otherwise keep a test's runners and device alive until some later collection, and the
    tensor-parallel tests further down the session want the hardware queues to themselves"""
    yield
    gc.collect()
