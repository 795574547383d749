"""Every weight-format kernel at the edges of its block fields (tests/edge_blocks.py: negative, zero, subnormal and largest block
scales; saturated quants, sub-scales and mins; activation rows whose Q8_K quants and 16-sums sit at the ends of their ranges).

The gates are the suite's own, on the new inputs -- nothing is fitted here:
  1. debug_block_dots == o.block_dots;  2. copy_rows_from of the quantized table == the oracle's, bit for bit;
  3. strict-order device: matmul_vec == the oracle bit for bit, one rhs row and three;
  4. fast device: |got - oracle| <= gemv_order_bound * GEMV_REL * (8 for Q4_1, Q5_1, Q2_K, Q4_K, Q5_K; else 1) + 1e-30
     (tests/test_hip_gemv.py), finite outputs, and the same bound against float64 of dequant_f64(W) . dequant(quantized x);
     the matrix with every scale sign flipped gives the negated output bit for bit;
  5. debug_superblock_ints / debug_gemm_ints == the reference's integers (tests/test_hip_kquant_ints.py);
  6. b >= 16 rows on the matrix cores: bit-exact (Q4_0, Q8_0, Q4_1, Q8_K) or row by row under the x 8 bound (Q4_K, Q6_K).
The oracle is the reference's arithmetic with i16_wrap = 0; tests/test_edge_blocks.py shows that the saturated
blocks on constant rows are inputs where that differs from the wrapped i16.

Float64 witness of gate 4, Q4_1 / Q5_1 only: the reference's dot rounds d_w d_x and m_w s_x to f16 (2^-11 relative, 25 times GEMV_REL,
on ANY blocks), so its own distance from the float64 dot is not covered by the re-association bound.  The witness adds
edge_blocks.f16_product_slack, the sum of those roundings' half-spacings -- derived from the number format, nothing observed.

Shapes are the smallest at which each mapping can go wrong: fewer rows than a wave's, odd counts, 2 / 9 / 65 blocks and 1 / 3 / 16
super-blocks per row, and 8193 rows (the two-rows-per-wave form every launch takes from 8192 rows, its last wave with one live row)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import edge_blocks as eb
from tests import test_hip_f16w_gemm as f16w
from tests.helpers import GEMV_REL, gemv_order_bound, record_observed
from tests.test_hip_gemv import HT
from tests.test_hip_kquant_ints import ref_ints_q4k, ref_ints_q6k, ref_q6k_offset_parts

pytestmark = pytest.mark.gpu

SHAPES_32 = [(3, 64), (37, 288), (130, 2080), (8193, 64)]
SHAPES_256 = [(3, 256), (37, 768), (130, 4096), (8193, 256)]
KQUANTS = ("Q2_K", "Q3_K", "Q4_K", "Q5_K", "Q6_K", "Q8_K")
X8 = ("Q4_1", "Q5_1", "Q2_K", "Q4_K", "Q5_K")
OBSERVED = "weight_edges_observed.json"


def shapes_for(fmt):
    return SHAPES_256 if fmt in KQUANTS else SHAPES_32


def row_kinds_for(m):
    """all four activation kinds; the 8193-row shape (what it adds is the row mapping, not the block content): two"""
    return eb.ROW_KINDS if m < 8192 else ["normal", "constant"]


_ODEV = []


def odev():
    if not _ODEV:
        _ODEV.append(o.OracleDevice(thread_num=4))
    return _ODEV[0]


@functools.lru_cache(maxsize=None)
def case(fmt, kind, m, k):
    """one matrix of the kind and its activation rows, with the oracle's outputs: computed once, shared by the gates, never written"""
    typ = synth.TYPE_BY_NAME[fmt]
    rng = np.random.default_rng([eb.FORMATS.index(fmt), eb.KINDS.index(kind), m, k])
    raw = eb.edge_blocks(rng, fmt, m, k, kind)
    xs = {a: eb.edge_rows(rng, k, a) for a in row_kinds_for(m)}
    ow = o.OracleTensor.from_bytes(raw, typ, [m, k], odev())
    ref = {a: ow.matmul_vec(o.OracleTensor.new(x, [k], odev())).export() for a, x in xs.items()}
    for a in ref:
        assert np.all(np.isfinite(ref[a])), (fmt, kind, m, k, a, "the reference itself must stay finite: Inf / NaN are out of scope")
    return SimpleNamespace(fmt=fmt, typ=typ, m=m, k=k, raw=raw, xs=xs, ow=ow, ref=ref, rb=k // o.BLOCK_ELEMS[typ] * o.BLOCK_BYTES[typ])


@functools.lru_cache(maxsize=None)
def bounds(fmt, kind, m, k):
    """per activation kind: (gate 4's bound, the float64 witness and its extra slack), from the oracle's dequantization and dequant_f64"""
    c = case(fmt, kind, m, k)
    w64 = eb.dequant_f64(c.raw, fmt).reshape(m, k)
    qt = o.rhs_dtype(c.typ)
    out = {}
    for a, x in c.xs.items():
        xq = o.quantize(x, qt)
        bound = gemv_order_bound(c.raw, c.typ, x, m, k) * GEMV_REL * (8 if fmt in X8 else 1) + 1e-30
        out[a] = (bound, w64 @ eb.dequant_rows_f64(xq, qt), eb.f16_product_slack(c.raw, fmt, xq, m, k))
    return out


def upload(ca, dev, c, raw=None):
    return ca.HipTensor.from_cpu(c.raw if raw is None else raw, [c.m, c.k], getattr(ca.GGMLType, HT[c.fmt]), dev)


@pytest.fixture(scope="module")
def sdev(ca):
    return ca.HipTensorDevice(0, False, 0, True)


@pytest.mark.parametrize("kind", eb.KINDS)
@pytest.mark.parametrize("fmt", eb.FORMATS)
def test_block_dots_and_dequantized_rows_are_bit_exact(ca, hdev, fmt, kind):
    """gates 1 and 2"""
    for (m, k) in shapes_for(fmt):
        c = case(fmt, kind, m, k)
        w = upload(ca, hdev, c)
        rows = sorted({0, m // 2, m - 1})
        for a, x in c.xs.items():
            hx = ca.HipTensor.new(x, [k], hdev)
            xq = o.quantize(x, o.rhs_dtype(c.typ))
            for row in rows:
                got = w.debug_block_dots(row, hx)
                ref = o.block_dots(c.raw[row * c.rb:(row + 1) * c.rb], c.typ, xq, k)
                assert np.array_equal(got, ref), f"{fmt} {kind} ({m},{k}) x {a} row {row}"
        pick = [m - 1, 0, m // 2]
        dst = ca.HipTensor.alloc([3, k], ca.GGMLType.F32, hdev)
        dst.copy_rows_from(w, pick)
        odst = o.OracleTensor.alloc([3, k], o.F32, odev())
        odst.copy_rows_from(c.ow, pick)
        assert np.array_equal(dst.export().view(np.uint32), odst.export().view(np.uint32)), f"{fmt} {kind} ({m},{k}) rows"


@pytest.mark.parametrize("kind", eb.KINDS)
@pytest.mark.parametrize("fmt", eb.FORMATS)
def test_strict_order_gemv_is_bit_exact(ca, sdev, fmt, kind):
    """gate 3: the comparison of test_hip_gemv._strict_gemv_equals_oracle, one rhs row of every kind, then three rows in one call"""
    for (m, k) in shapes_for(fmt):
        c = case(fmt, kind, m, k)
        w = upload(ca, sdev, c)
        for a, x in c.xs.items():
            got = w.matmul_vec(ca.HipTensor.new(x, [k], sdev)).export()
            assert np.array_equal(got.view(np.uint32), c.ref[a].view(np.uint32)), f"{fmt} {kind} ({m},{k}) x {a}: " \
                f"{int(np.sum(got.view(np.uint32) != c.ref[a].view(np.uint32)))} of {m} rows differ"
        three = list(c.xs)[-3:] if len(c.xs) >= 3 else list(c.xs) + ["normal"]
        xb = np.concatenate([c.xs[a] for a in three])
        gb = w.matmul_vec(ca.HipTensor.new(xb, [3, k], sdev)).export().reshape(3, m)
        for i, a in enumerate(three):
            assert np.array_equal(gb[i].view(np.uint32), c.ref[a].view(np.uint32)), f"{fmt} {kind} ({m},{k}) batched row {i} ({a})"


@pytest.mark.parametrize("kind", eb.KINDS)
@pytest.mark.parametrize("fmt", eb.FORMATS)
def test_fast_gemv_stays_inside_the_reassociation_bound(ca, hdev, fmt, kind):
    """gate 4 (the module docstring has the witness's extra term for Q4_1 / Q5_1)"""
    worst = {"oracle": 0.0, "float64": 0.0}
    for (m, k) in shapes_for(fmt):
        c = case(fmt, kind, m, k)
        w = upload(ca, hdev, c)
        wn = upload(ca, hdev, c, eb.negate_scales(c.raw, fmt)) if kind in ("sign", "mixed") else None
        for a, x in c.xs.items():
            bound, f64, slack = bounds(fmt, kind, m, k)[a]
            hx = ca.HipTensor.new(x, [k], hdev)
            got = w.matmul_vec(hx).export()
            assert np.all(np.isfinite(got)), f"{fmt} {kind} ({m},{k}) x {a}"
            e1 = np.abs(got.astype(np.float64) - c.ref[a].astype(np.float64))
            e2 = np.abs(got.astype(np.float64) - f64)
            worst["oracle"] = max(worst["oracle"], float(np.max(e1 / bound)))
            worst["float64"] = max(worst["float64"], float(np.max(e2 / (bound + slack))))
            print(f"{fmt} {kind} ({m},{k}) x {a}: err/bound oracle {np.max(e1 / bound):.3g} float64 {np.max(e2 / (bound + slack)):.3g}")
            assert np.all(e1 <= bound), f"{fmt} {kind} ({m},{k}) x {a}: max err/bound {np.max(e1 / bound):.3f} against the oracle"
            assert np.all(e2 <= bound + slack), f"{fmt} {kind} ({m},{k}) x {a}: max err/bound {np.max(e2 / (bound + slack)):.3f} against float64"
            if wn is not None:
                # -W: f32 negation is exact and the integers are the same, so no tolerance.  Compared as VALUES: equal non-zero
                # floats have equal bits, and an output that is exactly zero (rows whose blocks all have d = +-0, or saturated
                # blocks whose quants and mins are 0) is +0 for W and for -W alike -- a sum of zeros of both signs rounds to +0
                neg = wn.matmul_vec(hx).export()
                assert np.array_equal(neg, -got), f"{fmt} {kind} ({m},{k}) x {a}: {int(np.sum(neg != -got))} of {m} outputs of -W are " \
                    f"not the negation, first row {int(np.flatnonzero(neg != -got)[0])}"
    record_observed({f"gemv/{fmt}/{kind}": worst}, OBSERVED)


INT_FMTS = {"Q4_K": "Q4K", "Q6_K": "Q6K"}
INT_ROWS = ("constant", "one_hot_neg")


@pytest.mark.parametrize("kind", ["saturated", "mixed"])
@pytest.mark.parametrize("fmt", list(INT_FMTS))
def test_single_row_kernels_integers_at_the_top_of_their_factors(ca, hdev, fmt, kind):
    """gate 5, the production single-row loops (both Q4_K header forms): saturated sub-scales and mins against rows whose 16-sums are
    -2048 / 2032 reach the top of the __mul24 factors"""
    for (m, k) in SHAPES_256:
        c = case(fmt, kind, m, k)
        w = upload(ca, hdev, c)
        for a in INT_ROWS:
            if a not in c.xs:
                continue
            x = c.xs[a]
            hx = ca.HipTensor.new(x, [k], hdev)
            xq = o.quantize(x, o.Q8_K)
            full = w.matmul_vec(hx).export()
            for row in sorted({0, m // 2, m - 1}):
                ref = (ref_ints_q4k if fmt == "Q4_K" else ref_ints_q6k)(c.raw[row * c.rb:(row + 1) * c.rb], xq, k)
                for variant in ((0, 1) if fmt == "Q4_K" else (0,)):
                    got, val = w.debug_superblock_ints(row, hx, variant)
                    assert np.array_equal(np.asarray(got).reshape(-1, 2).astype(np.int64), ref), f"{fmt} {kind} ({m},{k}) x {a} row {row} variant {variant}"
                    if variant == 0 and m < 8192:
                        assert np.float32(val).view(np.uint32) == full[row].view(np.uint32)


BATCHED = [(37, 512, 16), (37, 512, 17), (130, 1024, 40)]
BATCHED_32 = [(37, 288, 16), (37, 288, 17), (130, 1024, 40)]


@functools.lru_cache(maxsize=None)
def batch_case(fmt, kind, m, k, b):
    """b rows cycling through the four activation kinds, and the oracle's (b, m) outputs"""
    c = case(fmt, kind, m, k) if (m, k) in shapes_for(fmt) else None
    typ = synth.TYPE_BY_NAME[fmt]
    rng = np.random.default_rng([eb.FORMATS.index(fmt), eb.KINDS.index(kind), m, k, b])
    raw = c.raw if c is not None else eb.edge_blocks(rng, fmt, m, k, kind)
    x = np.concatenate([eb.edge_rows(rng, k, eb.ROW_KINDS[i % 4]) for i in range(b)])
    ow = o.OracleTensor.from_bytes(raw, typ, [m, k], odev())
    ref = ow.matmul_vec(o.OracleTensor.new(x, [b, k], odev())).export().reshape(b, m)
    assert np.all(np.isfinite(ref))
    return SimpleNamespace(fmt=fmt, typ=typ, m=m, k=k, b=b, raw=raw, x=x, ref=ref, rb=k // o.BLOCK_ELEMS[typ] * o.BLOCK_BYTES[typ])


@pytest.mark.parametrize("kind", ["saturated", "mixed"])
@pytest.mark.parametrize("fmt", list(INT_FMTS))
def test_matrix_core_gemm_integers_at_the_ends_of_the_byte_split(ca, hdev, fmt, kind):
    """gate 5, k_gemm_mfma_q4k / k_gemm_mfma_q6k: a saturated column of 16-sums puts the high byte of bsum = 64 a + b at a = +-64"""
    for (m, k, b) in BATCHED:
        c = batch_case(fmt, kind, m, k, b)
        w = upload(ca, hdev, c)
        hx = ca.HipTensor.new(c.x, [b, k], hdev)
        ints, out = w.debug_gemm_ints(hx, b)
        nsb = k // 256
        ints = np.asarray(ints).reshape(b, m, nsb, 2).astype(np.int64)
        plain = w.matmul_vec(hx).export().reshape(b, m)
        assert np.array_equal(np.asarray(out).reshape(b, m).view(np.uint32), plain.view(np.uint32))  # the dump run IS the product GEMM
        for bi in range(min(b, 8)):  # two rows of every activation kind
            xq = o.quantize(c.x[bi * k:(bi + 1) * k], o.Q8_K)
            for row in sorted({0, 17, m - 1}):
                wr = c.raw[row * c.rb:(row + 1) * c.rb]
                if fmt == "Q4_K":
                    assert np.array_equal(ints[bi, row], ref_ints_q4k(wr, xq, k)), (fmt, kind, m, k, b, bi, row)
                else:
                    ref = ref_ints_q6k(wr, xq, k)[:, 0]
                    off = ref_q6k_offset_parts(wr, xq, k)
                    assert np.array_equal(ints[bi, row, :, 1], off), (fmt, kind, m, k, b, bi, row)
                    assert np.array_equal(ints[bi, row, :, 0] - 32 * ints[bi, row, :, 1], ref), (fmt, kind, m, k, b, bi, row)


@pytest.mark.parametrize("kind", eb.KINDS)
@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0", "Q4_1", "Q8_K", "Q4_K", "Q6_K"])
def test_batched_rhs_on_the_matrix_cores(ca, hdev, fmt, kind):
    """gate 6: bit-exact where test_batched_rhs_on_the_matrix_cores_is_bit_exact asserts it for random blocks, Q4_K / Q6_K row by row
    under the x 8 bound of test_batched_rhs_q4_k_on_the_matrix_cores / ..._q6_k_...; every batch holds rows of all four kinds"""
    worst = 0.0
    for (m, k, b) in (BATCHED if fmt in KQUANTS else BATCHED_32):
        c = batch_case(fmt, kind, m, k, b)
        w = upload(ca, hdev, c)
        got = w.matmul_vec(ca.HipTensor.new(c.x, [b, k], hdev))
        assert got.shape() == [b, m]
        got = got.export().reshape(b, m)
        assert np.all(np.isfinite(got)), f"{fmt} {kind} m={m} k={k} b={b}"
        if fmt in ("Q4_K", "Q6_K"):
            for r in range(b):
                bound = gemv_order_bound(c.raw, c.typ, c.x[r * k:(r + 1) * k], m, k) * GEMV_REL * 8 + 1e-30
                err = np.abs(got[r].astype(np.float64) - c.ref[r].astype(np.float64))
                worst = max(worst, float(np.max(err / bound)))
                assert np.all(err <= bound), f"{fmt} {kind} m={m} k={k} b={b} row {r} ({eb.ROW_KINDS[r % 4]}): {np.max(err / bound):.3f} of the bound"
        else:
            bad = np.argwhere(got.view(np.uint32) != c.ref.view(np.uint32))
            assert bad.size == 0, f"{fmt} {kind} m={m} k={k} b={b}: {len(bad)} outputs differ, first (rhs row, weight row) {tuple(bad[0])}: " \
                                  f"{got[tuple(bad[0])]!r} vs {c.ref[tuple(bad[0])]!r}"
    record_observed({f"mfma/{fmt}/{kind}": {"oracle": worst}}, OBSERVED)


# ---- gate 7: k_gemm_f16w (the fast prompt pass's GEMM) through crabml_hip_debug_gemm_f16w ---------------------------------------
F16W_TOP = 1.0  # the "range" set's largest member here: the launcher refuses what would put a folded operand A' past f16


@pytest.mark.parametrize("kind", ["sign", "range", "mixed"])
@pytest.mark.parametrize("fmt", f16w.FMTS)
def test_f16_gemm_operands_on_signed_and_subnormal_scales(ca, hdev, fmt, kind):
    """check_f16_operands' tier 2 (f16 operands summed in float64) and tier 3 (the dequantized operation) as they stand: both are
    derived from the roundings and do not know a scale's sign; u(v) = max(2^-11 |v|, 2^-25) already charges a subnormal A' half its
    spacing.  "range" / "mixed": d down to 2^-24 -- such matrices are taken, and a kernel that flushed f16 subnormals would lose their
    blocks whole."""
    for i, (m, k, b, force) in enumerate(((60, 512, 17, (1, 4, 1, 0)), (100, 768, 33, (2, 8, 1, 0)), (36, 256, 40, (0, 0, 0, -1)))):
        if fmt not in f16w.KQ:
            k = {512: 160, 768: 288, 256: 96}[k]
        rng = np.random.default_rng([eb.FORMATS.index(fmt), eb.KINDS.index(kind), i])
        raw = eb.edge_blocks(rng, fmt, m, k, kind, top=F16W_TOP)
        f16w.check_f16_operands(ca, hdev, fmt, m, k, b, force, 100 + i, raw=raw)


@pytest.mark.parametrize("fmt", f16w.FMTS)
def test_negative_weight_scales_that_put_a_past_f16_are_refused(ca, hdev, fmt):
    """test_weight_scales_that_put_a_past_f16_are_refused with the NEGATED pair: the first scale still refused, the second still taken
    and finite -- a matrix whose only out-of-range block is negative is refused like its positive twin (the upload scan compares
    magnitudes)"""
    rng = np.random.default_rng(29)
    m, k, b = 64, 512, 33
    typ = synth.TYPE_BY_NAME[fmt]
    bb = o.BLOCK_BYTES[typ]
    x = rng.standard_normal(b * k).astype(np.float32)
    for scale, refused in zip(f16w.BIG_SCALE[fmt], (True, False)):
        for twin in (-1.0, 1.0):
            raw = synth.random_blocks(rng, m * k, typ).reshape(-1, bb).copy()
            at = {"Q6_K": 208}.get(fmt, 0)
            raw[7, at:at + 2] = np.array([twin * scale], np.float16).view(np.uint8)
            if fmt == "Q6_K":
                raw[7, 192:208] = np.array([127] * 16, np.int8).view(np.uint8)
            if fmt == "Q4_1":
                raw[7, 2:4] = np.array([0.0], np.float16).view(np.uint8)
            w = f16w.upload(ca, hdev, raw.reshape(-1), fmt, m, k)
            if refused:
                with pytest.raises(Exception, match="refused"):
                    f16w.run(ca, hdev, [w], x, b, k, (1, 4, 1, 0))
            else:
                out = f16w.run(ca, hdev, [w], x, b, k, (1, 4, 1, 0))["out"][0]
                assert np.all(np.isfinite(out)), (fmt, twin)


# ---- whole models with mixed-sign blocks on the strict device -----------------------------------------------------------------
STRICT_MODELS = {"Q4_0": (synth.Q4_0, {}), "Q8_0": (synth.Q8_0, {}), "Q4_1": (synth.Q4_1, {}), "Q4_K": (synth.Q4_K, {"output_type": synth.Q6_K}),
                 "Q4_K_M": (synth.Q4_K, {"k_m_mix": True}), "Q5_K": (synth.Q5_K, {"k_m_mix": True}), "Q6_K": (synth.Q6_K, {})}


@pytest.mark.parametrize("fmt", list(STRICT_MODELS))
def test_strict_device_runs_mixed_sign_models_bit_identically(ca, fmt):
    """the bodies the launch pins take (tests/test_hip_*_launches.py, test_hip_q5k_fused.py, test_hip_q6k_fused.py) with
    edge_blocks.flip_scale_signs applied: a 23-token prompt pass and 8 decode steps on the strict-order device equal the oracle's token
    loop bit for bit, logits and KV bytes (the comparisons of tests/test_hip_prefill.py and tests/test_hip_fused.py)"""
    from tests.test_hip_prefill import PROMPT, kv_equal, oracle_run
    wtype, kw = STRICT_MODELS[fmt]
    model = eb.mixed_sign_model("tiny-gqa", wtype, 90, **kw)
    steps = [21, 22, 7, 9, 11, 13, 500, 31]
    ref, orr = oracle_run(model, True, PROMPT + steps)
    dev = ca.HipTensorDevice(0, False, 0, True)
    conf, w = synth.to_hip(model, dev)
    r = ca.HipLlamaRunner(conf, w, dev, 64, True)
    n = len(PROMPT)
    lg = r.prefill(PROMPT)
    assert r.kv_cache_len() == n
    assert np.array_equal(lg.view(np.uint32), ref[n - 1].view(np.uint32)), f"{fmt}: the prompt pass's logits"
    for i, t in enumerate(steps):
        assert np.array_equal(r.forward(t, n + i).view(np.uint32), ref[n + i].view(np.uint32)), f"{fmt}: decode step {i}"
    assert kv_equal(r, orr, model, n + len(steps), True), f"{fmt}: KV bytes"
