"""The checkers of k_gemm_f16w -- the fast prompt pass's weight GEMM (gemm_f16w.hip) -- by itself, through crabml_hip_debug_gemm_f16w,
for the tests of the kernel (tests/test_hip_f16w_gemm*.py), of the prompt pass that runs it (tests/prefill_pass_ref.py) and of the
restatements themselves.  What a format's A' is stands ONCE, in its row of tests/weight_formats.py (f16w); here, by the format's name:

  weight_operands   (A', W, the bound of A' against W) of the given weight rows, in ELEMENT order;
  row_operands      B' = f16(q d) of the quantized rows (Q8_K: q d in f32 first), B, its bound, the reference's blocks;
  b_groups          B' bit patterns per slot group, sorted: the multiset the kernel's k-slot order permutes;
  check_exact       tier 1: A' and B' small integers with sum |A' B'| < 2^24 per output, so that every f32 summation order is exact --
                    out must equal the float64 integer dot bit for bit (catches any slot pairing, lost k piece or mis-scaled group);
  check_f16_operands  tier 2: the f16 operands summed in float64 (random blocks, row magnitudes 2^-14 .. 2^12: subnormal B' included);
                    tier 3: float64 of the dequantized weights times the dequantized quantized rows (what the int8 path computes),
                    within a bound derived from the roundings (test_hip_f16w_gemm.test_matches_the_dequantized_operation).
Also here: Q5_K's map from the lanes' loads to B' slot order 3, and the Q5_0 / Q5_1 blocks of the edge-level and refused-matrix cases."""
import numpy as np

from crabml_amd import synth
from oracle import oracle as o
from tests.helpers import GEMV_REL
from tests.weight_formats import BY_NAME, _f16, _u


def kq(fmt):
    return BY_NAME[fmt].kq


def weight_operands(raw, fmt, rows, k, wrong=None):
    """(A' f16 as float64, W exact float64, error bound of A' against W), each (len(rows), k), for the given weight rows; wrong: a
    restatement that is subtly wrong in the named way (the format's f16w.wrong)"""
    F = BY_NAME[fmt]
    nb, rb = k // F.block_elems, k // F.block_elems * F.block_bytes
    raw = np.ascontiguousarray(raw).view(np.uint8)
    blk = np.stack([raw[r * rb:(r + 1) * rb] for r in rows]).reshape(-1, F.block_bytes)
    return tuple(v.reshape(len(rows), k) for v in F.f16w.operands(blk, len(rows), nb, wrong))


def int_weights(rng, fmt, m, k):
    """blocks whose A' are small integers (the format's f16w.int_blocks)"""
    F = BY_NAME[fmt]
    return F.f16w.int_blocks(rng, m * k // F.block_elems).reshape(-1)


def code_blocks(rng, fmt):
    """64 super-blocks that between them hold every scale code of the format: 16 rows of k = 1024"""
    return BY_NAME[fmt].f16w.code_blocks(rng)


def row_operands(x, fmt, b, k):
    """(B' f16 as float64, B exact float64, error bound of B' against B, the rows' reference blocks), each (b, k)"""
    qt = BY_NAME[fmt].rhs
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
    """B' bit patterns per slot group -- a block of the reading weight's format: 32 elements (order 0) or a super-block (the K-quant
    orders) -- sorted: the multiset the kernel's k-slot order permutes"""
    g = BY_NAME[fmt].block_elems
    return np.sort(np.asarray(bits, np.uint16).reshape(b, k // g, g), axis=2)


def upload(ca, hdev, raw, fmt, m, k):
    return ca.HipTensor.from_cpu(raw, [m, k], getattr(ca.GGMLType, BY_NAME[fmt].ht), hdev)


def run(ca, hdev, ws, x, b, k, force=(0, 0, 0, -1), rows_path=0, junk=0):
    hx = ca.HipTensor.new(np.ascontiguousarray(x, np.float32), [b, k], hdev)
    r = ws[0].debug_gemm_f16w(list(ws[1:]), hx, b, rows_path, junk, list(force))
    r["out"] = [np.asarray(v, np.float32).reshape(b, -1) for v in r["out"]]
    return r


# ---- tier 1: exact integers ---------------------------------------------------------------------------------------------------
def int_rows(rng, fmt, b, k):
    """integer rows that the row quantizer keeps as they are: d = 1 (one +-127 per 32-element block; Q8_K: one -128 per super-block)"""
    x = rng.integers(-8, 9, (b, k)).astype(np.float32)
    if BY_NAME[fmt].rhs == o.Q8_K:
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


# ---- tiers 2 and 3: f16 operands, float64 sum; the dequantized operation -----------------------------------------------------
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
    # tier 3 (the derivation: test_hip_f16w_gemm.test_matches_the_dequantized_operation)
    bound = (np.abs(bx) + eb) @ ea.T + eb @ np.abs(wx).T + GEMV_REL * mag
    err3 = np.abs(got - bx @ wx.T)
    assert np.all(err3 <= bound), f"{fmt} ({m},{k},{b}) {force}: tier 3 worst {np.max(err3 / bound):.3g} of the bound"
    return r


# ---- Q5_K: the lanes' loads against B' slot order 3 (the order Q2_K / Q3_K read, which Q5_K shares) --------------------------------
def order3_pos(E):
    """f16w_pos_q8k(3, 0, E) (f16w_rows.hpp) restated: the position, in halfs from the super-block's start, of element E = 128 h + 32 j + l
    in B' slot order 3 -- chunk j / 2, lane group g = 2 h + l / 16, step s = (l / 4) % 4, slots 4 (j & 1) .. in the order 0, 2, 1, 3"""
    E = np.asarray(E)
    l, j = E & 31, (E >> 5) & 3
    g, s, k, hi, cc = 2 * (E >> 7) + (l >> 4), (l >> 2) & 3, l & 3, j & 1, j >> 1
    return (4 * cc + g) * 32 + 8 * s + 4 * hi + ((k >> 1) | ((k & 1) << 1))


def lane_slots():
    """What the kernel's lanes put into the A' slots, as (element [256], position [256]): in chunk c of a super-block lane group g loads
    the 16-byte piece g & 1 of pair p = 2 (g >> 1) + c -- bytes qs[32 p + 16 (g & 1) + 4 s + b], dword s in step s -- and unpack_q5_k_f16
    writes, to the step's slots 0..7, the low nibbles of bytes 0, 2, 1, 3 and then the high nibbles of bytes 0, 2, 1, 3, each with bit
    2 p + hi of qh[16 (g & 1) + 4 s + b].  The element of (p, hi, l) is 64 p + 32 hi + l; the slot's position is chunk c, group g, step s,
    slot e: (4 c + g) * 32 + 8 s + e -- where B' must hold the same element."""
    elem, pos, qh_bit = [], [], []
    for c in range(2):
        for g in range(4):
            p = 2 * (g >> 1) + c
            for s in range(4):
                for e in range(8):
                    hi, b = e >> 2, (0, 2, 1, 3)[e & 3]
                    l = 16 * (g & 1) + 4 * s + b
                    elem.append(64 * p + 32 * hi + l)
                    pos.append((4 * c + g) * 32 + 8 * s + e)
                    qh_bit.append((l, 4 * (g >> 1) + 2 * c + hi))  # the kernel's shift 4 (g >> 1) + 2 c, then bit hi
    return np.array(elem), np.array(pos), qh_bit


# ---- Q5_0 / Q5_1: edge levels, and a matrix the range check refuses ----------------------------------------------------------------
def edge_level_blocks(rng, fmt, m, k):
    """random blocks with scales of either sign, and among them blocks whose fifth bits are all set, all clear and alternating, with the
    nibbles at 0 and at 15: levels 0, 15, 16 and 31 next to each other"""
    typ = synth.TYPE_BY_NAME[fmt]
    raw = synth.random_blocks(rng, m * k, typ).reshape(-1, o.BLOCK_BYTES[typ]).copy()
    h = 2 if fmt == "Q5_0" else 4
    raw[::2, 1] ^= 0x80
    for i, (qh, qs) in enumerate(((0xFF, 0xFF), (0x00, 0x00), (0x55, 0xF0), (0xAA, 0x0F), (0xFF, 0x00), (0x00, 0xFF))):
        raw[i::16, h:h + 4] = qh
        raw[i::16, h + 4:] = qs
    return raw.reshape(-1)


def refuse_matrix(model, wname, block=37):
    """one block of the named Q5_0 / Q5_1 tensor rewritten so that the f16 GEMM's range check refuses the matrix while every weight of
    the block is exactly 0 (the edge values of tests/test_hip_f16w_gemm_q5_01.EDGE):
      Q5_0: d = 4096, qh = 0xFFFFFFFF, qs = 0 -- every level is 16, (16 - 16) d = 0, yet 16 |d| = 65536 > 65504;
      Q5_1: d = 2114, m = 0, qh = 0, qs = 0 -- every level is 0, 0 d + 0 = 0, yet f16(31 * 2114 = 65534) is inf.
    The matrix then takes the row-by-row GEMV inside a pass whose other matrices take the GEMM, and its values stay ordinary"""
    t = model.tensors[wname]
    fmt = synth.TYPE_NAMES[t.typ]
    assert fmt in ("Q5_0", "Q5_1"), (wname, fmt)
    blk = np.array(t.data, dtype=np.uint8).reshape(-1, o.BLOCK_BYTES[t.typ])
    assert block < blk.shape[0]
    blk[block] = 0
    if fmt == "Q5_0":
        blk[block, 0:2] = np.array([4096.0], np.float16).view(np.uint8)
        blk[block, 2:6] = 0xFF
    else:
        blk[block, 0:2] = np.array([2114.0], np.float16).view(np.uint8)
    t.data = blk.reshape(-1)
    w = weight_operands(t.data, fmt, [block * 32 // t.shape[1]], t.shape[1])[1].reshape(-1, 32)[block % (t.shape[1] // 32)]
    assert np.all(w == 0.0), w
    return model
