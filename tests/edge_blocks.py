"""Weight blocks and activation rows at the edges of their fields, and a float64 restatement of every format's dequantization.

synth.random_blocks draws every block scale positive and inside one decade, Q6_K group scales from -64..63, Q8_K quants without -128,
and uniform bytes never saturate a sub-block.  edge_blocks starts from random_blocks (whose default byte stream stays as it is: the
bench and the golden files depend on it) and overwrites fields:

  "sign"       the sign bit of d flipped in a random half of the blocks; dmin / m (and Q8_K's f32 d) likewise, independently;
               magnitudes unchanged; from 8 blocks on, a few blocks carry d = +0 and d = -0.
  "range"      per block |d| from {2^-24 (smallest f16 subnormal), 1023 * 2^-24 (largest subnormal), 2^-14, 1.0, TOP}, random sign;
               dmin / m drawn independently from the same set.  TOP = 65504: no format's dequantized element leaves f32 with it
               (the largest is Q6_K's 65504 * 128 * 32 = 2.7e8).  Q4_1 / Q5_1's m stops at 64: the reference multiplies m_w by the
               row's s_x = f16(d_x sum q) IN f16 (buf_q4_1.rs:266-280), |s_x| <= sum |x| <= 32 * 16 for the rows of edge_rows
               (|x| <= 16), and 64 * 512 * (1 + 2^-7) stays below 65504 -- Inf / NaN are out of scope.
               Q8_K's f32 d: {2^-126, 1e-30, 1.0, 1e30}, random sign.
  "saturated"  every integer field at an end of its range, block by block, in every combination of the ends (see _saturate).
  "mixed"      every block drawn independently from the three kinds above or left as random_blocks made it.

Block layouts: the comments of synth.random_blocks."""
import numpy as np

from crabml_amd import synth
from oracle import oracle as o

FORMATS = ["Q4_0", "Q8_0", "Q4_1", "Q5_0", "Q5_1", "Q2_K", "Q3_K", "Q4_K", "Q5_K", "Q6_K", "Q8_K"]
KINDS = ["sign", "range", "saturated", "mixed"]
ROW_KINDS = ["normal", "constant", "one_hot_neg", "alternating"]
# byte offsets of the f16 scale fields: (d, dmin-or-m or None); Q8_K's d is an f32 at 0
SCALE_AT = {"Q4_0": (0, None), "Q8_0": (0, None), "Q4_1": (0, 2), "Q5_0": (0, None), "Q5_1": (0, 2), "Q2_K": (80, 82), "Q3_K": (108, None),
            "Q4_K": (0, 2), "Q5_K": (172, 174), "Q6_K": (208, None)}
X_MAX = 16.0  # |x| of every row edge_rows returns
# build_model seeds of the mixed-sign models behind the launch pins (tests/test_hip_*_launches.py) and their CPU cap evaluation
MIXED_SIGN_SEEDS = {"fused": 38, "fused_k": 48, "prefill": 50, "prefill_k": 72}
F16_TOP, M_TOP = 65504.0, 64.0


def _fields(fmt):
    d, m = SCALE_AT[fmt]
    return [d] if m is None else [d, m]


def scale_fields(raw, fmt):
    """the f16 scale fields of every block as float64: {"d": (nb,), "m": (nb,) where the format has dmin / m}; Q8_K: its f32 d"""
    typ = synth.TYPE_BY_NAME[fmt]
    blk = np.ascontiguousarray(raw).view(np.uint8).reshape(-1, o.BLOCK_BYTES[typ])
    if fmt == "Q8_K":
        return {"d": blk[:, 0:4].copy().view(np.float32)[:, 0].astype(np.float64)}
    out = {}
    for name, at in zip(("d", "m"), _fields(fmt)):
        out[name] = blk[:, at:at + 2].copy().view(np.float16)[:, 0].astype(np.float64)
    return out


def negate_scales(raw, fmt):
    """a copy with the sign bit of EVERY d / dmin / m flipped: the matrix -W exactly (the integer fields untouched)"""
    typ = synth.TYPE_BY_NAME[fmt]
    blk = np.ascontiguousarray(raw).view(np.uint8).reshape(-1, o.BLOCK_BYTES[typ]).copy()
    if fmt == "Q8_K":
        blk[:, 3] ^= 0x80
    else:
        for at in _fields(fmt):
            blk[:, at + 1] ^= 0x80
    return blk.reshape(-1)


def _half(rng, nb):
    """a 0 / 1 flag per block, set in exactly nb // 2 of them (both values occur from two blocks on)"""
    f = np.zeros(nb, np.uint8)
    f[rng.permutation(nb)[:nb // 2]] = 1
    return f


def _sign(rng, blk, fmt, top=None):
    nb = blk.shape[0]
    if fmt == "Q8_K":
        blk[:, 3] ^= _half(rng, nb) << 7
        return
    for at in _fields(fmt):
        blk[:, at + 1] ^= _half(rng, nb) << 7
    if nb >= 8:  # d = +0 and d = -0, one block in 16 each (at least one)
        z = rng.permutation(nb)[:2 * max(1, nb // 16)]
        at = SCALE_AT[fmt][0]
        blk[z, at] = 0
        blk[z[0::2], at + 1] = 0x00
        blk[z[1::2], at + 1] = 0x80


def range_magnitudes(fmt, field, top=None):
    """the |scale| set of the "range" kind (docstring above); `top` replaces the largest f16 member (for consumers with a range of
    their own: the f16 GEMM refuses matrices whose folded operands would leave f16)"""
    if fmt == "Q8_K":
        return np.array([2.0 ** -126, 1e-30, 1.0, 1e30], np.float32)
    if top is None:
        top = M_TOP if (fmt in ("Q4_1", "Q5_1") and field == 1) else F16_TOP
    return np.array([2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14, 1.0, top], np.float16)


def _cover(rng, nb, n):
    """nb indices into n choices: every choice taken (from n blocks on), in random order"""
    return rng.permutation(np.arange(nb) % n) if nb >= n else rng.integers(0, n, nb)


def _range(rng, blk, fmt, top=None):
    nb = blk.shape[0]
    if fmt == "Q8_K":
        mags = range_magnitudes(fmt, 0)
        # (sign, magnitude) pairs covered together: both signs of every magnitude occur from 8 blocks on
        c = _cover(rng, nb, 2 * mags.size)
        d = mags[c // 2] * np.where(c % 2 == 1, np.float32(-1), np.float32(1))
        blk[:, 0:4] = d.astype(np.float32).reshape(nb, 1).view(np.uint8)
        return
    for i, at in enumerate(_fields(fmt)):
        mags = range_magnitudes(fmt, i, top)
        c = _cover(rng, nb, 2 * mags.size)
        v = (mags[c // 2].view(np.uint16) | ((c % 2).astype(np.uint16) << 15)).astype(np.uint16)
        blk[:, at:at + 2] = v.reshape(nb, 1).view(np.uint8)


def _k4_scales(sc_top, mn_top):
    """the 12 scale bytes of a Q4_K / Q5_K block whose eight 6-bit scales are all 63 (or 0) and whose mins are all 63 (or 0):
    scales live in bytes 0..3 (all 8 bits: 6 low of j < 4, 2 high of j >= 4) and the low nibbles of bytes 8..11, mins in bytes 4..7
    and the high nibbles (util.rs:19-27)"""
    q = np.zeros(12, np.uint8)
    if sc_top:
        q[0:4] = 0xFF
        q[8:12] |= 0x0F
    if mn_top:
        q[4:8] = 0xFF
        q[8:12] |= 0xF0
    return q


def _saturate(rng, blk, fmt, top=None):
    """Every integer field at an end of its range.  Per block one combination of independent top / bottom choices, all combinations
    covered (from as many blocks on as there are combinations):
      Q4_0 / Q4_1  nibbles 15 | 0                                   Q8_0   quants 127 | -128
      Q5_0 / Q5_1  nibbles 15 | 0  x  high bits all set | clear     Q8_K   quants 127 | -128 (bsums follow)
      Q2_K  quants 3 | 0  x  scale nibbles 15 | 0  x  min nibbles 15 | 0
      Q3_K  low bits 3 | 0  x  hmask all | none  x  6-bit scales 63 | 0 (+31 | -32)
      Q4_K  nibbles 15 | 0  x  scales 63 | 0  x  mins 63 | 0        Q5_K   the same x high bits all | none
      Q6_K  quants 63 | 0  x  int8 scales all 127 | all -128 | each 127 or -128 at random"""
    nb = blk.shape[0]
    ff = lambda bit: np.where(bit, 0xFF, 0x00).astype(np.uint8)[:, None]  # noqa: E731
    if fmt in ("Q4_0", "Q4_1"):
        c = _cover(rng, nb, 2)
        blk[:, (2 if fmt == "Q4_0" else 4):] = ff(c & 1)
    elif fmt == "Q8_0":
        c = _cover(rng, nb, 2)
        blk[:, 2:] = np.where(c & 1, 127, -128).astype(np.int8).view(np.uint8)[:, None]
    elif fmt in ("Q5_0", "Q5_1"):
        c = _cover(rng, nb, 4)
        h = 2 if fmt == "Q5_0" else 4
        blk[:, h:h + 4] = ff(c & 1)
        blk[:, h + 4:] = ff(c & 2)
    elif fmt == "Q8_K":
        c = _cover(rng, nb, 2)
        q = np.repeat(np.where(c & 1, 127, -128).astype(np.int8)[:, None], 256, axis=1)
        blk[:, 4:260] = q.view(np.uint8)
        blk[:, 260:] = q.reshape(nb, 16, 16).astype(np.int16).sum(axis=2).astype(np.int16).view(np.uint8).reshape(nb, 32)
    elif fmt == "Q2_K":
        c = _cover(rng, nb, 8)
        blk[:, 16:80] = ff(c & 1)
        blk[:, 0:16] = (np.where(c & 2, 0x0F, 0) | np.where(c & 4, 0xF0, 0)).astype(np.uint8)[:, None]
    elif fmt == "Q3_K":
        c = _cover(rng, nb, 8)
        blk[:, 32:96] = ff(c & 1)
        blk[:, 0:32] = ff(c & 2)
        blk[:, 96:108] = ff(c & 4)
    elif fmt in ("Q4_K", "Q5_K"):
        c = _cover(rng, nb, 8 if fmt == "Q4_K" else 16)
        sc = np.stack([_k4_scales(bool(v & 2), bool(v & 4)) for v in c])
        if fmt == "Q4_K":
            blk[:, 4:16] = sc
            blk[:, 16:] = ff(c & 1)
        else:
            blk[:, 160:172] = sc
            blk[:, 0:128] = ff(c & 1)
            blk[:, 128:160] = ff(c & 8)
    elif fmt == "Q6_K":
        c = _cover(rng, nb, 6)
        blk[:, 0:192] = ff(c & 1)
        s = c // 2
        each = np.where(rng.integers(0, 2, (nb, 16)) == 1, 127, -128)
        sc = np.where((s == 0)[:, None], 127, np.where((s == 1)[:, None], -128, each)).astype(np.int8)
        blk[:, 192:208] = sc.view(np.uint8)
    else:
        raise ValueError(fmt)


_APPLY = {"sign": _sign, "range": _range, "saturated": _saturate}


def edge_blocks(rng, fmt, m, k, kind, top=None):
    """raw GGML bytes (uint8) of an (m, k) matrix in format `fmt` (a name of FORMATS) whose blocks are of the given kind"""
    typ = synth.TYPE_BY_NAME[fmt]
    bb = o.BLOCK_BYTES[typ]
    base = synth.random_blocks(rng, m * k, typ).reshape(-1, bb).copy()
    if kind in _APPLY:
        _APPLY[kind](rng, base, fmt, top)
        return base.reshape(-1)
    assert kind == "mixed", kind
    nb = base.shape[0]
    pick = _cover(rng, nb, 4)  # 0: as random_blocks made it
    out = base.copy()
    for i, name in enumerate(("sign", "range", "saturated"), start=1):  # each kind covers its combinations within its own blocks
        alt = base[pick == i].copy()
        _APPLY[name](rng, alt, fmt, top)
        out[pick == i] = alt
    return out.reshape(-1)


def edge_rows(rng, k, kind):
    """one f32 activation row of k elements, |x| <= X_MAX.  Per 256-element super-block (the rhs quantizer's unit for the K-quants;
    the 32-element quantizers see eight blocks of the same content):
      "normal"       standard normal times a factor in 0.1 .. 2.
      "constant"     every element +a or every element -a: buf_q8_k.rs:84-131 scales by -128 / (the signed max-abs element), so EVERY
                     quant is -128 and every 16-sum -2048, whichever the sign.  Every second super-block has its leading element
                     negated -- the one change that turns the others into +128, clamped to 127: all its other quants are 127 and 15 of
                     its 16 sums are 2032.
      "one_hot_neg"  one element at -a, the rest at +a 127 / 128: one quant -128, the others 127.
      "alternating"  +-a 127 / 128 alternating (quants +-127, 16-sums 0) and the leading element at -a (the one -128; its 16-sum is -1):
                     a super-block cannot have sums of exactly 0 everywhere with |q| = 128 in it, and it always has one.
    a is a power of two or 3 times one, 2^-3 .. 12."""
    nsb = (k + 255) // 256
    if kind == "normal":
        x = rng.standard_normal(k) * rng.uniform(0.1, 2.0)
        return np.clip(x, -X_MAX, X_MAX).astype(np.float32)
    a = (rng.choice([1.0, 3.0], nsb) * 2.0 ** rng.integers(-3, 3, nsb)).astype(np.float32)
    x = np.zeros((nsb, 256), np.float32)
    if kind == "constant":
        c = (np.arange(nsb) + int(rng.integers(0, 4))) % 4  # sign x variant, all four from four super-blocks on
        x[:] = (a * np.where(c & 1, np.float32(1), np.float32(-1)))[:, None]
        odd = (c & 2) != 0
        x[odd, 0] = -x[odd, 0]
    elif kind == "one_hot_neg":
        x[:] = (a * np.float32(127.0 / 128.0))[:, None]
        x[np.arange(nsb), rng.integers(0, 256, nsb)] = -a
    elif kind == "alternating":
        x[:] = (a * np.float32(127.0 / 128.0))[:, None] * np.where(np.arange(256) % 2 == 0, np.float32(-1), np.float32(1))[None, :]
        x[:, 0] = -a
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x.reshape(-1)[:k])


def _q5_levels(qh4, qs):
    """the 32 levels 0..31 of Q5_0 / Q5_1 blocks in element order (buf_q5_0.rs:22-37): element i < 16 = low nibble of qs[i] | bit i
    of qh << 4, element 16 + i = high nibble | bit 16 + i << 4"""
    qh = qh4.copy().view("<u4")[:, 0].astype(np.int64)
    bits = (qh[:, None] >> np.arange(32)[None, :]) & 1
    q = qs.astype(np.int64)
    return np.concatenate([q & 15, q >> 4], axis=1) | (bits << 4)


def _q3k_scales(s12):
    """the sixteen 6-bit scales of Q3_K blocks (buf_q3_k.rs:44-55): low nibbles of bytes 0..7 then their high nibbles, two more bits
    from bytes 8..11 (scale j: byte 8 + j % 4, bits 2 (j / 4) ..)"""
    s = s12.astype(np.int64)
    lo = np.concatenate([s[:, 0:8] & 15, s[:, 0:8] >> 4], axis=1)
    j = np.arange(16)
    hi = (s[:, 8 + j % 4] >> (2 * (j // 4))) & 3
    return lo | (hi << 4)


def _two_bit_planes(qs64):
    """the 256 two-bit values of 64 bytes in Q2_K / Q3_K element order: per half of 32 bytes, four shifts, 32 bytes each"""
    q = qs64.astype(np.int64).reshape(-1, 2, 1, 32)
    return ((q >> (2 * np.arange(4))[None, None, :, None]) & 3).reshape(-1, 256)


def dequant_f64(raw, fmt):
    """float64 of every element of the blocks `raw`, in ELEMENT order (element i is what the dot products pair with activation i),
    computed exactly from the fields: one rounding to f32 gives the reference's dequantized value, whose expressions round at most
    once (products of an 11-bit scale, a 6- or 8-bit sub-scale and a level fit f32; the roundings are Q4_1 / Q5_1 n d + m, the K-quant
    n d sc - dmin m, Q6_K's 25-bit product, Q8_K's f32 d times q).  Q4_1: the reference's OWN dequantize writes the nibbles
    interleaved (buf_q4_1.rs:19-30) while its vec_dot pairs them in element order; this is element order."""
    from tests.test_hip_f16w_gemm import weight_operands
    from tests.test_hip_kquant_ints import scale_min_k4
    typ = synth.TYPE_BY_NAME[fmt]
    bb = o.BLOCK_BYTES[typ]
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    blk = raw.reshape(-1, bb)
    nb = blk.shape[0]
    if fmt in ("Q4_0", "Q8_0", "Q4_1", "Q4_K", "Q6_K"):
        with np.errstate(invalid="ignore"):  # (its f16 operands, not used here, overflow on "range" blocks)
            return weight_operands(raw, fmt, [0], nb * o.BLOCK_ELEMS[typ])[1].reshape(-1)
    f16at = lambda a: blk[:, a:a + 2].copy().view(np.float16).astype(np.float64)[:, 0:1]  # noqa: E731
    if fmt == "Q5_0":
        return ((_q5_levels(blk[:, 2:6], blk[:, 6:]) - 16) * f16at(0)).reshape(-1)
    if fmt == "Q5_1":
        return (_q5_levels(blk[:, 4:8], blk[:, 8:]) * f16at(0) + f16at(2)).reshape(-1)
    if fmt == "Q8_K":
        return (blk[:, 0:4].copy().view(np.float32).astype(np.float64) * blk[:, 4:260].view(np.int8).astype(np.float64)).reshape(-1)
    if fmt == "Q2_K":
        sc = np.repeat(blk[:, 0:16].astype(np.int64), 16, axis=1)
        return ((f16at(80) * (sc & 15)) * _two_bit_planes(blk[:, 16:80]) - f16at(82) * (sc >> 4)).reshape(-1)
    if fmt == "Q3_K":
        # bit p = 4 half + shift index of hmask[l] belongs to element 32 p + l (the mask bit moves on across the halves)
        hbit = ((blk[:, 0:32].astype(np.int64)[:, None, :] >> np.arange(8)[None, :, None]) & 1).reshape(-1, 256)
        lev = _two_bit_planes(blk[:, 32:96]) - 4 * (1 - hbit)
        sc = np.repeat(_q3k_scales(blk[:, 96:108]) - 32, 16, axis=1)
        return ((f16at(108) * sc) * lev).reshape(-1)
    if fmt == "Q5_K":
        d, dmin = f16at(172), f16at(174)
        sc = np.zeros((nb, 8), np.int64)
        mn = np.zeros_like(sc)
        for i in range(nb):
            sc[i], mn[i] = scale_min_k4(blk[i, 160:172])
        qs = blk[:, 0:128].astype(np.int64).reshape(-1, 4, 32)
        n = np.stack([qs & 15, qs >> 4], axis=2).reshape(-1, 8, 32)
        hb = ((blk[:, 128:160].astype(np.int64)[:, None, :] >> np.arange(8)[None, :, None]) & 1)  # sub-block j: bit j of qh[l]
        n = n + 16 * hb
        return ((d * sc)[:, :, None] * n - (dmin * mn)[:, :, None]).reshape(-1)
    raise ValueError(fmt)


def dequant_rows_f64(xq, qt):
    """float64 of quantized activation rows (Q8_0 / Q8_1 / Q8_K blocks): q d, exact"""
    bb = o.BLOCK_BYTES[qt]
    blk = np.ascontiguousarray(xq).view(np.uint8).reshape(-1, bb)
    if qt == o.Q8_K:
        return (blk[:, 0:4].copy().view(np.float32).astype(np.float64) * blk[:, 4:260].view(np.int8).astype(np.float64)).reshape(-1)
    d = blk[:, 0:2].copy().view(np.float16).astype(np.float64)
    return (d * blk[:, (2 if qt == o.Q8_0 else 4):].view(np.int8).astype(np.float64)).reshape(-1)


def f16_product_slack(raw, fmt, xq, m, k):
    """Per weight row, how far the REFERENCE's Q4_1 / Q5_1 dot may sit from the float64 dot of the dequantized operands, from its own
    f16 roundings (buf_q4_1.rs:266-280, buf_q5_1.rs:141-160; zero for every other format):
      sum over blocks of  u(d_w d_x) |sum n q|  +  u(m_w s_x)  +  |m_w| u(d_x sum q),   u(v) = max(2^-11 |v|, 2^-25)
    -- h_mul(d_w, d_x) and h_mul(m_w, s_x) round to f16 (normal: 2^-11 relative; subnormal: half a spacing, 2^-25), and the row's
    s_x is itself f16(d_x sum q)."""
    if fmt not in ("Q4_1", "Q5_1"):
        return np.zeros(m)
    typ = synth.TYPE_BY_NAME[fmt]
    u = lambda v: np.maximum(2.0 ** -11 * np.abs(v), 2.0 ** -25)  # noqa: E731
    xb = np.ascontiguousarray(xq).view(np.uint8).reshape(-1, 36)
    dx = xb[:, 0:2].copy().view(np.float16)[:, 0].astype(np.float64)
    sx = xb[:, 2:4].copy().view(np.float16)[:, 0].astype(np.float64)
    qsum = xb[:, 4:].view(np.int8).astype(np.int64).sum(axis=1)
    f = scale_fields(raw, fmt)
    dw, mw = f["d"].reshape(m, -1), f["m"].reshape(m, -1)
    rb = k // 32 * o.BLOCK_BYTES[typ]
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    sumi = np.stack([o.block_dots(raw[r * rb:(r + 1) * rb], typ, xq, k) for r in range(m)]).astype(np.float64)
    return (u(dw * dx) * np.abs(sumi) + u(mw * sx) + np.abs(mw) * u(dx * qsum)).sum(axis=1)


def reference_dequantize(raw, fmt):
    """o.dequantize in ELEMENT order (Q4_1's interleaving undone: position 2 i holds element i, 2 i + 1 element 16 + i)"""
    v = o.dequantize(raw, synth.TYPE_BY_NAME[fmt])
    if fmt == "Q4_1":
        v = v.reshape(-1, 16, 2).transpose(0, 2, 1).reshape(-1)
    return v


def flip_scale_signs(model, rng):
    """a copy of a synth.RawModel with the "sign" kind applied to every quantized tensor (the magnitudes, and with them the growth of
    the residual stream, stay as synth made them)"""
    out = synth.RawModel(model.shape, model.wtype)
    for name, t in model.tensors.items():
        fmt = synth.TYPE_NAMES.get(t.typ)
        data = t.data
        if fmt in FORMATS:
            blk = np.array(data, dtype=np.uint8).reshape(-1, o.BLOCK_BYTES[t.typ])
            _sign(rng, blk, fmt)
            data = blk.reshape(-1)
        out.tensors[name] = synth.RawTensor(data, list(t.shape), t.typ)
    return out


def mixed_sign_model(shape, wtype, seed, **kw):
    """synth.build_model(shape, wtype, seed, ...) with flip_scale_signs applied (its generator seeded from the model's): the one
    builder of the mixed-sign cases, so that the CPU evaluation of the checkers' excused-share caps and the GPU pins see the same bytes"""
    model = synth.build_model(synth.SHAPES[shape] if isinstance(shape, str) else shape, wtype, seed=seed, **kw)
    return flip_scale_signs(model, np.random.default_rng([seed, 1]))
