"""k_gemm_f16w -- the fast prompt pass's weight GEMM (gemm_f16w.hip) -- by itself, through crabml_hip_debug_gemm_f16w.

The kernel folds the block scales into f16 operands and sums in f32 inside the matrix core:
  A' = f16((q - 8) d) Q4_0 | f16(q d) Q8_0 | f16(n d + m) Q4_1 (one rounding) | f16(n c1 - c2), c1 = f16(d sc), c2 = f16(dmin m) Q4_K
       | f16((q - 32) f16(d sc)) Q6_K
  B' = f16(q d) of the quantized rows (Q8_K: q d in f32 first)
Restated here in numpy in ELEMENT order (the kernel's k-slot order is its own business: it has to pair the slots right to match), and
checked at three depths:
  1. exact integers: A' and B' small integers with sum |A' B'| < 2^24 per output, so that every f32 summation order is exact -- out
     must equal the float64 integer dot bit for bit (catches any slot pairing, lost k piece or mis-scaled group);
  2. the f16 operands summed in float64 (random blocks, row magnitudes 2^-14 .. 2^12: subnormal B' included);
  3. the operation itself: float64 of the dequantized weights times the dequantized quantized rows (what the int8 path computes),
     within a bound derived from the roundings (test_matches_the_dequantized_operation).
Plus the range edges: junk behind the live B', B' past 65504 (the overflow flag), weight scales that put A' past 65504 (refused)."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests.helpers import GEMV_REL
from tests.test_hip_kquant_ints import scale_min_k4

FMTS = ["Q4_0", "Q8_0", "Q4_1", "Q4_K", "Q6_K"]
HT = {"Q4_0": "Q4_0", "Q8_0": "Q8_0", "Q4_1": "Q4_1", "Q4_K": "Q4K", "Q6_K": "Q6K"}
ROWS = {"Q4_0": o.Q8_0, "Q8_0": o.Q8_0, "Q4_1": o.Q8_1, "Q4_K": o.Q8_K, "Q6_K": o.Q8_K}
KQ = ("Q4_K", "Q6_K")
U = 2.0 ** -11  # f16 unit roundoff (normal range)
SUB = 2.0 ** -25  # half the f16 subnormal spacing


def _f16(v):
    """one rounding of an exact float64 value to f16"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, np.float64).astype(np.float16)


def _u(v):
    """bound of one f16 rounding of the exact value v"""
    return np.maximum(U * np.abs(v), SUB)


def _nib(qs):
    """Q4_0 / Q4_1 nibbles of (nb, 16) bytes in element order: low nibbles = elements 0..15, high = 16..31"""
    return np.concatenate([qs & 15, qs >> 4], axis=1).astype(np.int64)


def weight_operands(raw, fmt, rows, k):
    """(A' f16 as float64, W exact float64, error bound of A' against W), each (len(rows), k), for the given weight rows"""
    typ = synth.TYPE_BY_NAME[fmt]
    be, bb = o.BLOCK_ELEMS[typ], o.BLOCK_BYTES[typ]
    rb = k // be * bb
    blk = np.stack([raw[r * rb:(r + 1) * rb] for r in rows]).reshape(-1, bb)
    f16at = lambda a, b: blk[:, a:b].copy().view(np.float16).astype(np.float64)[:, 0:1]  # noqa: E731
    if fmt in ("Q4_0", "Q8_0", "Q4_1"):
        d = f16at(0, 2)
        if fmt == "Q4_0":
            w = (_nib(blk[:, 2:]) - 8) * d
        elif fmt == "Q8_0":
            w = blk[:, 2:].view(np.int8).astype(np.int64) * d
        else:
            w = _nib(blk[:, 4:]) * d + f16at(2, 4)
        ap = _f16(w).astype(np.float64)
        ea = _u(w)
    elif fmt == "Q4_K":
        d, dmin = f16at(0, 2), f16at(2, 4)
        sc = np.zeros((blk.shape[0], 8), np.int64)
        mn = np.zeros_like(sc)
        for i in range(blk.shape[0]):
            sc[i], mn[i] = scale_min_k4(blk[i, 4:16])
        qs = blk[:, 16:].astype(np.int64).reshape(-1, 4, 32)
        n = np.stack([qs & 15, qs >> 4], axis=2).reshape(-1, 8, 32)  # sub-block 2 j: low nibbles of qs[32 j ..], 2 j + 1: high
        dsc, dm = (d * sc)[:, :, None], (dmin * mn)[:, :, None]
        c1, c2 = _f16(dsc).astype(np.float64), _f16(dm).astype(np.float64)
        w = (n * dsc - dm).reshape(-1, 256)
        ap = _f16(n * c1 - c2).astype(np.float64).reshape(-1, 256)
        # c1 and c2 one rounding each, n exact, then ONE rounding of n c1 - c2 (charged against |n c1| + |c2|, not |A'|)
        ea = (n * _u(dsc) + _u(dm) + _u(n * np.abs(c1) + np.abs(c2))).reshape(-1, 256)
    else:  # Q6_K: ql[128] | qh[64] | scales i8[16] | d f16
        d = f16at(208, 210)
        ql, qh = blk[:, :128].astype(np.int64), blk[:, 128:192].astype(np.int64)
        sc = blk[:, 192:208].view(np.int8).astype(np.int64)
        q = np.zeros((blk.shape[0], 256), np.int64)
        s = np.zeros_like(q)
        for h in range(2):
            L, H = ql[:, 64 * h:64 * h + 64], qh[:, 32 * h:32 * h + 32]
            for j, (lo, sh, hi) in enumerate(((L[:, :32] & 15, 0, 0), (L[:, 32:] & 15, 2, 2), (L[:, :32] >> 4, 4, 4), (L[:, 32:] >> 4, 6, 6))):
                e0 = 128 * h + 32 * j
                q[:, e0:e0 + 32] = lo | (((H >> sh) & 3) << 4)
                s[:, e0:e0 + 32] = np.repeat(sc[:, 8 * h + 2 * j:8 * h + 2 * j + 2], 16, axis=1)
        dsc = d * s
        c = _f16(dsc).astype(np.float64)
        w = (q - 32) * dsc
        ap = _f16((q - 32) * c).astype(np.float64)
        ea = np.abs(q - 32) * _u(dsc) + _u((q - 32) * c)
    nr = len(rows)
    return ap.reshape(nr, k), w.reshape(nr, k), ea.reshape(nr, k)


def row_operands(x, fmt, b, k):
    """(B' f16 as float64, B exact float64, error bound of B' against B, the rows' reference blocks), each (b, k)"""
    qt = ROWS[fmt]
    bb = o.BLOCK_BYTES[qt]
    blocks = [o.quantize(x[i * k:(i + 1) * k], qt).reshape(-1, bb) for i in range(b)]
    qb = np.stack(blocks)  # (b, nblocks, bb)
    if qt == o.Q8_K:
        d = qb[:, :, 0:4].copy().view(np.float32)  # (b, nsb, 1)
        q = qb[:, :, 4:260].view(np.int8)
        with np.errstate(over="ignore"):
            bp = (q.astype(np.float32) * d).astype(np.float16)  # q d in f32, then f16
        bx = q.astype(np.float64) * d.astype(np.float64)
        eb = _u(bx) * (1 + 2.0 ** -23) + 2.0 ** -24 * np.abs(bx)
    else:
        d = qb[:, :, 0:2].copy().view(np.float16).astype(np.float64)
        q = qb[:, :, (2 if qt == o.Q8_0 else 4):].view(np.int8)
        bx = q.astype(np.float64) * d
        bp = _f16(bx)
        eb = _u(bx)
    return bp.astype(np.float64).reshape(b, k), bx.reshape(b, k), eb.reshape(b, k), qb


def b_groups(bits, fmt, b, k):
    """B' bit patterns per slot group -- a block (order 0) or a super-block (K-quant orders) -- sorted: the multiset the kernel's
    k-slot order permutes"""
    g = 256 if fmt in KQ else 32
    return np.sort(np.asarray(bits, np.uint16).reshape(b, k // g, g), axis=2)


def upload(ca, hdev, raw, fmt, m, k):
    return ca.HipTensor.from_cpu(raw, [m, k], getattr(ca.GGMLType, HT[fmt]), hdev)


def run(ca, hdev, ws, x, b, k, force=(0, 0, 0, -1), rows_path=0, junk=0):
    hx = ca.HipTensor.new(np.ascontiguousarray(x, np.float32), [b, k], hdev)
    r = ws[0].debug_gemm_f16w(list(ws[1:]), hx, b, rows_path, junk, list(force))
    r["out"] = [np.asarray(v, np.float32).reshape(b, -1) for v in r["out"]]
    return r


# ---- tier 1: exact integers ---------------------------------------------------------------------------------------------------
def int_weights(rng, fmt, m, k):
    """blocks whose A' are small integers: d = 1 (Q4_K: dmin = 1, sub-scales 0..3, minimums 0..7; Q6_K: scales -2..2)"""
    typ = synth.TYPE_BY_NAME[fmt]
    nb = m * k // o.BLOCK_ELEMS[typ]
    one = np.array([1.0], np.float16).view(np.uint8)
    out = np.zeros((nb, o.BLOCK_BYTES[typ]), np.uint8)
    if fmt == "Q4_0":
        out[:, 0:2] = one
        out[:, 2:] = rng.integers(0, 256, (nb, 16))
    elif fmt == "Q8_0":
        out[:, 0:2] = one
        out[:, 2:] = rng.integers(-16, 17, (nb, 32)).astype(np.int8).view(np.uint8)
    elif fmt == "Q4_1":
        out[:, 0:2] = one
        out[:, 2:4] = (-rng.integers(0, 9, nb)).astype(np.float16).view(np.uint8).reshape(nb, 2)
        out[:, 4:] = rng.integers(0, 256, (nb, 16))
    elif fmt == "Q4_K":
        out[:, 0:2] = one
        out[:, 2:4] = one
        sc, mn = rng.integers(0, 4, (nb, 8)), rng.integers(0, 8, (nb, 8))
        out[:, 4:8], out[:, 8:12] = sc[:, :4], mn[:, :4]  # (values < 16: no high bits in bytes 0..7)
        out[:, 12:16] = sc[:, 4:] | (mn[:, 4:] << 4)
        out[:, 16:] = rng.integers(0, 256, (nb, 128))
    else:
        out[:, :192] = rng.integers(0, 256, (nb, 192))
        out[:, 192:208] = rng.integers(-2, 3, (nb, 16)).astype(np.int8).view(np.uint8)
        out[:, 208:210] = one
    return out.reshape(-1)


def int_rows(rng, fmt, b, k):
    """integer rows that the row quantizer keeps as they are: d = 1 (one +-127 per 32-element block; Q8_K: one -128 per super-block)"""
    x = rng.integers(-8, 9, (b, k)).astype(np.float32)
    if ROWS[fmt] == o.Q8_K:
        at = rng.integers(0, 256, (b, k // 256)) + 256 * np.arange(k // 256)
        np.put_along_axis(x, at, -128.0, axis=1)
    else:
        at = rng.integers(0, 32, (b, k // 32)) + 32 * np.arange(k // 32)
        np.put_along_axis(x, at, rng.choice([-127.0, 127.0], (b, k // 32)), axis=1)
    return x.reshape(-1)


def check_exact(ca, hdev, fmt, ms, k, b, force, seed, rows_path=0):
    rng = np.random.default_rng(seed)
    raws = [int_weights(rng, fmt, m, k) for m in ms]
    x = int_rows(rng, fmt, b, k)
    ws = [upload(ca, hdev, raw, fmt, m, k) for raw, m in zip(raws, ms)]
    r = run(ca, hdev, ws, x, b, k, force, rows_path)
    bp, bx, _, _ = row_operands(x, fmt, b, k)
    assert np.array_equal(bp, x.reshape(b, k).astype(np.float64)), "the integer rows must quantize to themselves"
    for j, (raw, m) in enumerate(zip(raws, ms)):
        ap = weight_operands(raw, fmt, range(m), k)[0]
        assert np.all(ap == np.round(ap))
        assert (np.abs(bp) @ np.abs(ap).T).max() < 2 ** 24, "every f32 summation order must be exact"
        ref = bp @ ap.T
        got = r["out"][j].astype(np.float64)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, f"{fmt} m={ms} k={k} b={b} force={force} used={r['used']} matrix {j}: {len(bad)} outputs differ, first (row, col) " \
                              f"{tuple(bad[0])}: {got[tuple(bad[0])]} vs {ref[tuple(bad[0])]}"
    return r


# every (F, T) instance at ksplit 1 over the shapes (m, k, b) in turn; then ksplit 2 / 4 / 8
SHAPES_Q = [(4, 96, 16), (60, 160, 17), (100, 288, 31), (1024, 2080, 33), (60, 4096, 64), (100, 14336, 65), (1024, 288, 129),
            (4, 2080, 200), (100, 160, 512)]
SHAPES_K = [(4, 256, 16), (60, 512, 17), (100, 768, 31), (1024, 2048, 33), (60, 4096, 64), (100, 14336, 65), (1024, 256, 129),
            (4, 1024, 200), (100, 512, 512)]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_exact_integer_operands_give_the_integer_dot_bit_for_bit(ca, hdev, fmt):
    shapes = SHAPES_K if fmt in KQ else SHAPES_Q
    i = 0
    for F in (1, 2):
        for T in (2, 4, 8):
            for _ in range(2):
                m, k, b = shapes[i % len(shapes)]
                r = check_exact(ca, hdev, fmt, [m], k, b, (F, T, 1, 0), 1000 * i + k)
                assert r["used"] == (F, T, 1, 0)
                i += 1
    for ks in (2, 4, 8):  # (a ragged k: the last piece holds the chunk with the padding slots)
        for (m, k, b) in ([(100, 4096, 33), (60, 2048, 129)] if fmt in KQ else [(100, 4096, 33), (60, 2080, 129)]):
            if k == 2080 and ks == 8:
                continue  # 17 chunks: an eighth piece would be empty
            r = check_exact(ca, hdev, fmt, [m], k, b, (2, 8, ks, 0), ks * 7 + k)
            assert r["used"][2] == ks
    # three matrices of different m in one launch (q | k | v), both B' writers
    k3 = 512 if fmt in KQ else 288
    for rows_path in (0, 1):
        check_exact(ca, hdev, fmt, [100, 60, 4], k3, 65, (1, 8, 1, 0), 77 + rows_path, rows_path)
        check_exact(ca, hdev, fmt, [1024, 64, 100], 4096, 17, (2, 2, 2, 0), 78 + rows_path, rows_path)


# ---- tier 2: f16 operands, float64 sum -------------------------------------------------------------------------------------
def wide_rows(rng, b, k):
    """rows whose 32-element blocks have magnitudes 2^-14 .. 2^12 (some B' subnormal)"""
    mag = 2.0 ** rng.uniform(-14, 12, (b, k // 32, 1))
    return (rng.standard_normal((b, k // 32, 32)) * mag).astype(np.float32).reshape(-1)


def check_f16_operands(ca, hdev, fmt, m, k, b, force, seed, rows=None, x=None, rows_path=0, raw=None):
    rng = np.random.default_rng(seed)
    if raw is None:
        raw = synth.random_blocks(rng, m * k, synth.TYPE_BY_NAME[fmt])
    if x is None:
        x = wide_rows(rng, b, k)
    w = upload(ca, hdev, raw, fmt, m, k)
    r = run(ca, hdev, [w], x, b, k, force, rows_path)
    bp, bx, eb, _ = row_operands(x, fmt, b, k)
    assert np.array_equal(b_groups(r["xh"], fmt, b, k), b_groups(bp.astype(np.float16).view(np.uint16), fmt, b, k)), "B' != f16(q d)"
    rows = np.arange(m) if rows is None else np.asarray(rows)
    ap, wx, ea = weight_operands(raw, fmt, rows, k)
    got = r["out"][0][:, rows].astype(np.float64)
    assert np.all(np.isfinite(got))
    mag = np.abs(bp) @ np.abs(ap).T
    err2 = np.abs(got - bp @ ap.T)
    assert np.all(err2 <= GEMV_REL * mag + 1e-30), f"{fmt} ({m},{k},{b}) {force}: tier 2 worst {np.max(err2 / (mag + 1e-30)):.3g} of sum |A'B'|"
    # tier 3 (the derivation: test_matches_the_dequantized_operation)
    bound = (np.abs(bx) + eb) @ ea.T + eb @ np.abs(wx).T + GEMV_REL * mag
    err3 = np.abs(got - bx @ wx.T)
    assert np.all(err3 <= bound), f"{fmt} ({m},{k},{b}) {force}: tier 3 worst {np.max(err3 / bound):.3g} of the bound"
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_f16_operands_summed_in_float64(ca, hdev, fmt):
    shapes = SHAPES_K if fmt in KQ else SHAPES_Q
    for i, F in enumerate((1, 2)):
        for j, T in enumerate((2, 4, 8)):
            m, k, b = shapes[(3 * i + j + 4) % len(shapes)]
            check_f16_operands(ca, hdev, fmt, m, k, b, (F, T, 1, 0), 31 * i + j + k)
    for ks in (2, 4, 8):
        check_f16_operands(ca, hdev, fmt, 100, 4096, 64, (1, 4, ks, 0), 5 * ks)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_matches_the_dequantized_operation(ca, hdev, fmt):
    """Tier 3 at the 8B shapes, through the launcher's own choice of launch form (sampled weight rows).

    Against float64 of W (the dequantized weights) times B (the dequantized quantized rows) -- what the int8 path computes.  The
    bound per output is derived from the roundings, not fitted: u(v) = max(2^-11 |v|, 2^-25) bounds one f16 rounding of v.
      B' - B:  u(q d); Q8_K rows add 2^-24 |q d| for the product's own f32 rounding.
      A' - W:  Q4_0 / Q8_0 / Q4_1: u(W) (the exact product or n d + m, rounded once);
               Q4_K: |n| u(d sc) + u(dmin m) + u(|n c1| + |c2|) (c1 = f16(d sc), c2 = f16(dmin m) rounded once each, then the fma
               n c1 - c2 once: charged against |n c1| + |c2|, not |A'|);
               Q6_K: |q - 32| u(d sc) + u((q - 32) c).
      |A'B' - WB| <= |A' - W| (|B| + |B' - B|) + |W| |B' - B| per product, summed over k; the f32 accumulation adds the tier-2 term
      GEMV_REL sum |A'B'|."""
    rng = np.random.default_rng(3)
    for (m, k, b) in ((14336, 4096, 136), (4096, 14336, 512)):
        rows = np.unique(np.concatenate([[0, 1, 63, 64, 127, m - 1], rng.integers(0, m, 40)]))
        x = (rng.standard_normal(b * k) * rng.uniform(0.1, 4.0)).astype(np.float32)
        check_f16_operands(ca, hdev, fmt, m, k, b, (0, 0, 0, -1), m + b, rows=rows, x=x)


# ---- gate | up epilogue -------------------------------------------------------------------------------------------------------
def silu_mul(g, u):
    """f16w_silu_mul: h = (g / (1 + e)) * u in f32, e = the reference's f16 exp table at f16(-g) (silu.rs:6-13)"""
    from tests.sampler_ref import exp_table
    e = o.f16_bits_to_f32(exp_table()[o.f32_to_f16_bits((-g).astype(np.float32))])
    return (g / (np.float32(1.0) + e)) * u


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_gate_up_epilogue_is_silu_mul_of_the_plain_launch(ca, hdev, fmt):
    rng = np.random.default_rng(11)
    for (m, k, b, T) in ((128, 512, 33, 2), (1024, 4096, 65, 4), (192, 2048, 200, 8)):
        typ = synth.TYPE_BY_NAME[fmt]
        ws = [upload(ca, hdev, synth.random_blocks(rng, m * k, typ), fmt, m, k) for _ in range(2)]
        x = (rng.standard_normal(b * k) * 2.0).astype(np.float32)
        plain = run(ca, hdev, ws, x, b, k, (2, T, 1, 0))
        g, u = plain["out"]
        h = run(ca, hdev, ws, x, b, k, (2, T, 1, 1))
        assert h["used"][3] == 1
        assert np.array_equal(h["out"][0].view(np.uint32), silu_mul(g, u).view(np.uint32)), f"{fmt} ({m},{k},{b}) T={T}"
        if fmt in KQ:
            continue
        # h left as ffn_down's row planes: the fields of o.quantize of that h, and its B' = f16(q d)
        hp = run(ca, hdev, ws, x, b, k, (2, T, 1, 2))
        assert hp["used"][3] == 2
        off_d, off_aux, total = hp["hq_layout"]
        planes = np.asarray(hp["hq"]).reshape(b, total)
        qt = ROWS[fmt]
        hh = h["out"][0]
        ref_xh = np.zeros((b, m), np.uint16)
        for r in range(b):
            blk = o.quantize(hh[r], qt).reshape(m // 32, -1)
            q = blk[:, 2 if qt == o.Q8_0 else 4:].view(np.int8)
            d = blk[:, 0:2].copy().view(np.uint16)[:, 0]
            assert np.array_equal(planes[r, :m].view(np.int8).reshape(m // 32, 32), q), (fmt, r)
            assert np.array_equal(planes[r, off_d:off_d + m // 16].view(np.uint16), d), (fmt, r)
            if qt == o.Q8_1:
                assert np.array_equal(planes[r, off_aux:off_aux + m // 16].view(np.uint16), blk[:, 2:4].copy().view(np.uint16)[:, 0])
            else:
                assert np.array_equal(planes[r, off_aux:off_aux + m // 8].view(np.int32), q.astype(np.int32).sum(axis=1))
            ref_xh[r] = _f16(q.astype(np.float64) * d.view(np.float16).astype(np.float64)[:, None]).view(np.uint16).reshape(-1)
        assert np.array_equal(b_groups(hp["hxh"], fmt, b, m), b_groups(ref_xh, fmt, b, m)), f"{fmt}: ffn_down's B'"


# ---- range edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_junk_behind_the_live_rows_does_not_matter(ca, hdev, fmt):
    """xh filled with 0, +-inf, NaN and 65504 before the rows are written: the outputs keep their bits (the k-slots past a ragged
    row's end multiply zero weights by whatever follows the last column)"""
    rng = np.random.default_rng(17)
    for (m, k, b, force) in ((100, 288, 33, (1, 8, 1, 0)), (60, 2080, 17, (2, 2, 4, 0)), (64, 160, 200, (0, 0, 0, -1)),
                             (100, 512, 31, (2, 4, 2, 0))):
        if fmt in KQ and k % 256:
            continue
        raw = synth.random_blocks(rng, m * k, synth.TYPE_BY_NAME[fmt])
        w = upload(ca, hdev, raw, fmt, m, k)
        x = (rng.standard_normal(b * k)).astype(np.float32)
        for rows_path in (0, 1):
            base = None
            for junk in (0x0000, 0x7C00, 0xFC00, 0x7E00, 0x7BFF):
                out = run(ca, hdev, [w], x, b, k, force, rows_path, junk)["out"][0]
                assert np.all(np.isfinite(out)), f"{fmt} ({m},{k},{b}) junk {junk:#06x}: {np.sum(~np.isfinite(out))} non-finite outputs"
                if base is None:
                    base = out
                assert np.array_equal(out.view(np.uint32), base.view(np.uint32)), f"{fmt} ({m},{k},{b}) junk {junk:#06x}"


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_overflow_flag_is_raised_exactly_when_a_b_value_is_inf(ca, hdev, fmt):
    rng = np.random.default_rng(23)
    m, k, b = 64, 512, 33
    raw = synth.random_blocks(rng, m * k, synth.TYPE_BY_NAME[fmt])
    w = upload(ca, hdev, raw, fmt, m, k)
    for big in (1.0, 6.0e4, 65504.0, 65519.0, 65520.0, 65600.0, 7.0e4, 1.0e6, 8.0e6):
        x = rng.standard_normal(b * k).astype(np.float32)
        x[5 * k + 300] = -big
        x[20 * k + 7] = big * 0.75
        bp = row_operands(x, fmt, b, k)[0]
        inf = bool(np.isinf(bp).any())
        for rows_path in (0, 1):
            r = run(ca, hdev, [w], x, b, k, (1, 4, 1, 0), rows_path)
            assert r["overflow"] == inf, f"{fmt} |x| = {big}: flag {r['overflow']}, B' has inf: {inf}"
            assert np.array_equal(b_groups(r["xh"], fmt, b, k), b_groups(bp.astype(np.float16).view(np.uint16), fmt, b, k))
    assert inf, "the largest row must overflow"


BIG_SCALE = {"Q4_0": (8192.0, 8000.0), "Q8_0": (600.0, 500.0), "Q4_1": (4500.0, 4000.0), "Q4_K": (70.0, 60.0), "Q6_K": (17.0, 15.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_weight_scales_that_put_a_past_f16_are_refused(ca, hdev, fmt):
    """one block whose scale can make |A'| > 65504 (Q4_0 8 |d|, Q8_0 128 |d|, Q4_1 15 |d| + |m|, Q4_K 15 f16(63 d) + f16(63 dmin),
    Q6_K 32 |f16(d sc)|): the launcher does not take the matrix; a scale just inside the range is taken and stays finite"""
    rng = np.random.default_rng(29)
    m, k, b = 64, 512, 33
    typ = synth.TYPE_BY_NAME[fmt]
    bb = o.BLOCK_BYTES[typ]
    x = rng.standard_normal(b * k).astype(np.float32)
    for scale, refused in zip(BIG_SCALE[fmt], (True, False)):
        raw = synth.random_blocks(rng, m * k, typ).reshape(-1, bb).copy()
        at = {"Q6_K": 208}.get(fmt, 0)
        raw[7, at:at + 2] = np.array([scale], np.float16).view(np.uint8)
        if fmt == "Q6_K":
            raw[7, 192:208] = np.array([127] * 16, np.int8).view(np.uint8)
        if fmt == "Q4_1":
            raw[7, 2:4] = np.array([0.0], np.float16).view(np.uint8)
        w = upload(ca, hdev, raw.reshape(-1), fmt, m, k)
        hx_fn = lambda: run(ca, hdev, [w], x, b, k, (1, 4, 1, 0))  # noqa: E731
        if refused:
            with pytest.raises(Exception, match="refused"):
                hx_fn()
        else:
            out = hx_fn()["out"][0]
            assert np.all(np.isfinite(out)), fmt


def test_restated_operands_are_the_reference_dot():
    """The numpy restatement (element order, exact W, B) reproduces the oracle's vec_dot of the same blocks: the GPU tests above
    compare against the reference's own operands"""
    rng = np.random.default_rng(41)
    for fmt in FMTS:
        k = 1024
        typ = synth.TYPE_BY_NAME[fmt]
        raw = synth.random_blocks(rng, 3 * k, typ)
        x = rng.standard_normal(2 * k).astype(np.float32)
        ap, wx, ea = weight_operands(raw, fmt, range(3), k)
        bp, bx, eb, qb = row_operands(x, fmt, 2, k)
        rb = k // o.BLOCK_ELEMS[typ] * o.BLOCK_BYTES[typ]
        for r in range(3):
            for i in range(2):
                ref = o.vec_dot(raw[r * rb:(r + 1) * rb], typ, qb[i].reshape(-1), k)
                mine = float(wx[r] @ bx[i])
                tol = 1e-5 * float(np.abs(wx[r]) @ np.abs(bx[i]))
                if fmt == "Q4_1":  # the reference adds m_w s_x with the rows' s = f16(d_x sum q) rounded (buf_q8_1.rs): exact here
                    mw = raw[r * rb:(r + 1) * rb].reshape(-1, 20)[:, 2:4].copy().view(np.float16).astype(np.float64)[:, 0]
                    sx = qb[i][:, 2:4].copy().view(np.float16).astype(np.float64)[:, 0]
                    tol += float(np.abs(mw) @ _u(sx))
                assert abs(mine - ref) <= tol, (fmt, r, i, mine, ref)
        assert np.all(np.abs(ap - wx) <= ea) and np.all(np.abs(bp - bx) <= eb), fmt
        # the integer tier's blocks restate as integers, and its rows quantize to themselves
        wi = int_weights(rng, fmt, 2, k)
        ai = weight_operands(wi, fmt, range(2), k)[0]
        assert np.all(ai == np.round(ai)) and np.abs(ai).max() <= 64
        xi = int_rows(rng, fmt, 2, k)
        assert np.array_equal(row_operands(xi, fmt, 2, k)[0], xi.reshape(2, k).astype(np.float64)), fmt
