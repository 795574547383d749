"""The launches of ONE chunk pass of the fast prompt path (prefill_chunk_pass, crabml_amd/csrc/fused.hip) restated in float64, ONE
FUNCTION PER LAUNCH, on all rows of the pass.

Every function takes the bytes its launch read -- from the tap, HipLlamaRunner.debug_prefill_tap / crabml_hip_llama_debug_prefill_tap,
whose fields are named as in include/crabml_hip_debug.h -- and the model's raw weights, and compares what the launch left with the
exact value within a bound derived from roundings (tests/fused_step_ref.py: U = 2^-24, row_dots, norm_interval, QuantIntervals,
silu_mul_interval) or one the project already states for that kernel:

  embedding       pf_x in front of layer 0 = the reference's dequantized row of token r, bit for bit.
  norm launch     x_out = x_in + (pending + piece 1 + ...) in float64, one rounding per add (the kernels add the pieces to the pending
                  output in piece order, then the sum to x: prefill_rows.hpp); without anything pending x is untouched, bit for bit.
                  planes: the interval check of norm_interval(x_out) -- the exact norm, sqrtf(sum / n + eps), (v / rms) * w.
                  B': f16(q d) of the tapped planes, bit for bit, as a sorted multiset per 32-element block.
  f16 GEMM        out (+ the k pieces, summed in float64) against the float64 sum of A' B', A' from the raw weights and B' = f16(q d)
                  from the tapped planes, within GEMV_REL sum |A' B'|: tier 2 of tests/test_hip_f16w_gemm.py.
  int8 GEMM/GEMV  row_dots' bound on the tapped planes (k_gemm_mfma: sumf = fma((float)sumi * d_w, d_x, sumf) for Q4_0 / Q8_0 -- one
                  rounding fewer per block than the two row_dots charges; Q4_1: f16(d_w d_x) * sumi + f16(m s), the f16 products
                  row_dots restates; gemm_mfma.hip).
  k_qkv_epi_rows  from the stored pf_q / pf_k / pf_v: the Qwen2 bias (one rounding), rope at position pos0 + r with the reference's own
                  cos / sin (three roundings), the q scale (one more); K / V cache rows [pos0, pos0 + B) = the f16 codes between the
                  interval's ends (f32 cache: within the bound); every cache byte outside those rows = the snapshot taken before.
  attention       the exact kernels: row r = oracle_attention at position pos0 + r, bit for bit (the long-row kernels past 1024 cached
                  positions: inside the hull of the reference's f16 chain over every admissible softmax row sum, long_row_hull).
                  k_attn_flash_rows: float64 causal attention on the same f16 inputs within FLASH_ROWS_REL of max|out|
                  (tests/test_hip_flash_attention.py).
                  planes: the reference quantizer of the stored rows, byte for byte.
  SiLU * mul      g and u stored: h's planes pass the interval check of silu_mul_interval(g, 0, u, 0).  h stored (the GEMM's epilogue):
                  h inside silu_mul_interval of the exact g, u with the GEMM's bound; planes = the reference quantizer of h, byte for
                  byte.  Only planes leave the launch (h_done == 2): h comes from a twin context with PREFILL_SEPARATE_F16_ROWS, whose
                  h is checked as above, and the planes must be the reference quantizer of THAT h byte for byte.
  the tail        last layer: pf_x = x + ffn_down (one rounding); the final norm reads row B - 1 of it; the classifier's planes pass
                  the interval check; the logits are within row_dots' bound.

Host cost: `Sample` picks weight rows and prompt rows of the GEMM checks before any device value is looked at (None = every row).

Q8_K-ROW PASSES (Q4_K / Q5_K / Q6_K layer matrices, the Q4_K_M / Q5_K_M mixes).  Which kernel a matrix took is READ from the plan
(kernel_q .. kernel_down: 1 k_gemm_f16w, 2 the int8 matrix-core GEMM, 3 the wave-per-row GEMV), never inferred: in a Q5_K_M layer v
takes the f16 GEMM while q takes the GEMV, and plan["f16w"] says 1 either way.  With the f32 rows the tap stores (n1.xn / n2.xn, hid.h,
cls.xn) no K launch needs an interval excuse:

  norm launch     both arms (k_norm_f32_rows + quantizer; k_norm_quant_rows_k): x as above; xn inside norm_interval(x_out); the Q8_K
                  planes = the reference quantizer of the STORED xn, byte for byte (d with its sign, the first holder of the maximum,
                  ties away from zero, the sixteen 16-element sums); the class-major plane = the permutation of q.
  B'              f16(f32(q d)) with d the plane's f32 -- TWO roundings, restated as such (not f16 of the float64 product) --, as a
                  sorted multiset per super-block (b_groups of the reading weight's format; n1.xh.v against attn_v's).  The k-slot
                  order itself is held by the GEMM check, which multiplies by A' in element order.
  f16 GEMM        GEMV_REL sum |A' B'| with A' = f16(n c1 - c2), c1 = f16(d sc), c2 = f16(dmin m) (Q4_K), f16((q - 32) f16(d sc)) (Q6_K):
                  weight_operands of tests/test_hip_f16w_gemm.py.
  row-by-row GEMV fused_step_ref.row_dots / q5k_step_ref.row_dots: (8 nsb + C_K) U sum A over the kernels' pieces.
  int8 GEMM       k_gemm_mfma_q4k, per super-block and output: the integers isum = sum_j sc_j dot_j (|isum| <= 256 * 15 * 127 * 63 = 3.1e7,
                  past 2^24: its conversion to f32 ROUNDS) and msum = sum_j m_j bsum_j (<= 8 * 63 * 32 * 127 = 2.0e6: exact), then
                  F += (d_w d8) (float)isum - (dmin_w d8) (float)msum with -ffp-contract=off: 2 conversions (one of which can round), 2
                  scale products, 2 products, 1 subtraction, 1 add into the accumulator = 8 operations, at most 7 roundings.  With
                  A_sb = |d_w d8 isum| + |dmin_w d8 msum| the term is off by at most 3 U |d_w d8 isum| + 3 U |dmin_w d8 msum| + U |term|
                  <= 4 U A_sb (1 + 3 U), and the nsb adds (in super-block order) by U times a partial sum of |terms| each:
                      |f32 - exact| <= (nsb + 4) U sum_sb A_sb (1 + small).
                  k_gemm_mfma_q6k: v = (float)(sum_g sc_g dot_g - 32 sum_g sc_g bsum_g) (|v| < 2^25: may round), F += (d_w d8) v: 1
                  conversion, 1 scale product, 1 product, 1 add: (nsb + 3) U sum_sb |d_w d8 v|.
                  row_dots' bound is (8 nsb + C_K) U sum over the 8 PIECES of a super-block of A_piece, and sum_pieces A_piece >= A_sb
                  (the pieces' integers add up to the super-block's: triangle inequality on both parts).  8 nsb + 3 >= 2 (nsb + 4) - 3
                  for every nsb >= 1, so row_dots' bound DOMINATES the derived one with a factor of at least 11 / 5 (nsb = 1) and
                  towards 8 for long rows: it is used for the int8 GEMM as it stands (C_K not raised); no new constant.  It stays
                  a sharp check of what it must see: one quant off by a step moves a dot by |w_i| d8, one sub-block's minimum term by
                  dmin m |bsum| d8 -- both orders of magnitude above (8 nsb + 3) 6e-8 of the row's sum A.
  SiLU * mul      h_done == 0: g and u within their GEMM bounds; hid.h (pf_g after k_gateup_epi) inside silu_mul_interval(g, 0, u, 0) of the
                  stored g and u; planes = the reference quantizer of the stored h, byte for byte.  h_done == 1 as above.  h_done == 2 (the
                  row quantizer inside the GEMM) exists for Q8_0 / Q8_1 rows only: a Q8_K tap that says 2 fails.
  the tail        cls.xn inside norm_interval(last.x); the classifier's planes = the reference quantizer of cls.xn byte for byte."""
import functools
from dataclasses import dataclass

import numpy as np

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests import q5k_step_ref as Q5
from tests.fused_step_ref import U, Result, check_f32
from tests.helpers import GEMV_REL
from tests.test_hip_f16w_gemm import b_groups, weight_operands

FLASH_ROWS_REL = 1.5e-3  # tests/test_hip_flash_attention.py: k_attn_flash_rows against float64 on the same f16 inputs, of max|out|
ATTN_FLASH_ROWS, ATTN_TILE, ATTN_LONG_ROWS, ATTN_PER_ROW = 1, 2, 3, 4  # CRABML_HIP_PFPLAN_ATTN_KERNEL
KERNEL_F16W, KERNEL_INT8, KERNEL_GEMV = 1, 2, 3  # CRABML_HIP_PFPLAN_KERNEL_*
KERNEL_WORD = {"attn_q": "kernel_q", "attn_k": "kernel_k", "attn_v": "kernel_v", "attn_output": "kernel_wo", "ffn_gate": "kernel_gate",
               "ffn_up": "kernel_up", "ffn_down": "kernel_down"}
F16W_FMT = {synth.Q4_0: "Q4_0", synth.Q8_0: "Q8_0", synth.Q4_1: "Q4_1", synth.Q4_K: "Q4_K", synth.Q6_K: "Q6_K"}  # formats k_gemm_f16w takes


@dataclass
class Form:
    kv_f16: bool
    seq_cap: int


@dataclass
class Sample:
    """the weight rows and prompt rows the GEMM checks look at: the first and the last 64-row tile of every matrix and `extra` random
    rows between; the first and the last column tile of the pass (the row at pos0 is row 0) and `extra` rows between.  A launch's column
    tile is 16 T rows with T = 2, 4 or 8, so 128 rows from either end hold the first and the last tile whatever T the launcher chose"""
    extra: int = 24
    seed: int = 1
    col_tile: int = 128

    def wrows(self, m):
        rng = np.random.default_rng(self.seed + m)
        return np.unique(np.concatenate([np.arange(min(64, m)), np.arange(max(0, (m - 1) // 64 * 64), m), rng.integers(0, m, self.extra)]))

    def prows(self, b):
        rng = np.random.default_rng(self.seed + 7 * b)
        t = self.col_tile
        return np.unique(np.concatenate([np.arange(min(t, b)), np.arange(max(0, b - t), b), rng.integers(0, b, self.extra)]))


def _w(model, name):
    return model.tensors[name]


def _f32(model, name):
    return np.ascontiguousarray(model.tensors[name].data).view(np.float32)


def rows_of(tap, name, cols):
    return np.asarray(tap[name]).reshape(-1, cols)


def act_rows(tap, name):
    """the tapped planes of every row -> [parse_act per row]; a Q8_K set with its class-major plane (field name + ".qp", which the Q4_K
    int8 kernels read) put back in element order as "qp_q" (fused_step_ref.tap_act)"""
    qt = tap["qtype"][name]
    n = tap["plan"]["rows"] if name != "cls.act" else 1
    raw = np.asarray(tap[name]).reshape(n, -1)
    acts = [R.parse_act(raw[r], qt) for r in range(n)]
    if qt == o.Q8_K and name + ".qp" in tap:
        qp = np.ascontiguousarray(tap[name + ".qp"]).view(np.int8).astype(np.int64).reshape(n, -1)
        for r, a in enumerate(acts):
            a["qp_q"] = R.from_class_major(qp[r]).reshape(a["q"].shape)
    return acts


def b_prime(acts):
    """B' of the rows' blocks, element order: (f16 bits [B, k], float64 values).  Q8_0 / Q8_1 rows: f16(q d), one rounding (7 bits x
    11 bits is exact in f32).  Q8_K rows: d is an f32, so f16(f32(q d)) -- the product rounded to f32, THEN to f16: two roundings, and
    not the same value as f16 of the exact product wherever the f32 rounding lands on an f16 tie"""
    with np.errstate(over="ignore"):
        if acts[0]["qt"] == o.Q8_K:
            h = np.stack([(a["q"].astype(np.float32) * a["d"].astype(np.float32)[:, None]).reshape(-1) for a in acts]).astype(np.float16)
        else:
            h = np.stack([(a["q"] * a["d"][:, None]).reshape(-1) for a in acts]).astype(np.float16)
    return h.view(np.uint16), h.astype(np.float64)


# ---- embedding ----
def check_embedding(tap, model, tokens, ctx):
    res = Result("embedding")
    emb, dim = _w(model, "token_embd.weight"), model.shape.dim
    want = np.stack([o.dequantize(emb.data, emb.typ, int(t) * dim, dim) for t in tokens])
    got = rows_of(tap, "in.x", dim)
    same = got.view(np.uint32) == want.view(np.uint32)
    if not same.all():
        r, i = np.argwhere(~same)[0]
        res.fails.append(f"{ctx} embedding: row {r} element {i}: {got[r, i]!r} != the reference's {want[r, i]!r} ({int((~same).sum())} differ)")
    return res


# ---- the norm launches ----
def norm_intervals(x, w, eps, n):
    """norm_interval for every row of x [B, n]"""
    parts = [R.norm_interval(x[r], w, eps, n) for r in range(x.shape[0])]
    return tuple(np.stack([p[i] for p in parts]) for i in range(3))


def check_xh(res, tap, xh_name, act_name, ctx, model=None, wname=None):
    """wname: the weight whose GEMM reads this B' (its format decides the slot groups: a 32-element block, a K-quant super-block)"""
    if xh_name not in tap:
        return
    acts = act_rows(tap, act_name)
    bits, _ = b_prime(acts)
    b, k = bits.shape
    fmt = "Q4_0"
    if acts[0]["qt"] == o.Q8_K:
        fmt = F16W_FMT.get(_w(model, wname).typ)
        if fmt not in ("Q4_K", "Q6_K"):
            res.fails.append(f"{ctx} {res.launch}: {xh_name} is present, but {wname} is of a format the f16 GEMM does not take")
            return
    got = np.asarray(tap[xh_name], dtype=np.uint16).reshape(b, k)
    same = np.all(b_groups(got, fmt, b, k) == b_groups(bits, fmt, b, k), axis=2)
    if not same.all():
        r, blk = np.argwhere(~same)[0]
        res.fails.append(f"{ctx} {res.launch}: {xh_name} row {r} block {blk}: B' is not f16(q d) of the tapped planes ({int((~same).sum())} blocks)")


def check_in_interval(res, got, lo, hi, what, ctx):
    """every row of the stored f32 values lies inside [lo, hi] (as an f32 value: distance from the middle against the half width)"""
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        res.fails.append(f"{ctx} {res.launch}: {what}: non-finite values")
        return
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    res.ratio(np.abs(got - mid).reshape(-1), half.reshape(-1) + 1e-37, what, ctx)


def check_norm(tap, model, l, which, ctx):
    """which = "n1" (the layer's first norm launch: x_in = in.x, pending = in.tmp + in.parts, attn_norm, the model's eps) or "n2" (after
    wo: x_in = n1.x, pending = wo.tmp + wo.parts, ffn_norm, the literal 1e-5 of llama2.rs:611)"""
    res = Result("norm " + which)
    s = model.shape
    dim = s.dim
    if which == "n1":
        x_in, pend, parts = "in.x", "in.tmp", "in.parts"
        wn, eps = _f32(model, f"blk.{l}.attn_norm.weight"), s.rms_eps
    else:
        x_in, pend, parts = "n1.x", "wo.tmp", "wo.parts"
        wn, eps = _f32(model, f"blk.{l}.ffn_norm.weight"), 1e-5
    x0 = rows_of(tap, x_in, dim)
    x1 = rows_of(tap, which + ".x", dim)
    if pend in tap:
        terms = [rows_of(tap, pend, dim).astype(np.float64)]
        if parts in tap:
            terms += list(np.asarray(tap[parts], dtype=np.float64).reshape(-1, x0.shape[0], dim))
        exact = x0.astype(np.float64) + sum(terms)
        mag = np.abs(x0.astype(np.float64)) + sum(np.abs(t) for t in terms)
        check_f32(res, x1.reshape(-1), exact.reshape(-1), (len(terms) * U * mag + 1e-37).reshape(-1), "x", ctx)
    else:
        same = x0.view(np.uint32) == x1.view(np.uint32)
        if not same.all():
            res.fails.append(f"{ctx} {res.launch}: x changed with nothing pending ({int((~same).sum())} elements)")
    name = which + ".act"
    lo, hi, ref = norm_intervals(x1, wn, eps, dim)
    if which + ".xn" in tap:  # the f32 norm is stored (k_norm_f32_rows, k_norm_quant_rows_k): no interval excuse
        xn = rows_of(tap, which + ".xn", dim)
        check_in_interval(res, xn, lo, hi, "xn", ctx)
        check_planes_of(res, tap, name, xn, "act_dim (of the stored xn)", ctx)
    elif tap["qtype"][name] == o.Q8_K:
        res.fails.append(f"{ctx} {res.launch}: a Q8_K-row pass stores {which}.xn in both arms; the tap has none")
    else:
        R.QuantIntervals(lo, hi, ref, tap["qtype"][name]).check(tap[name], res, "act_dim", ctx)
    first, second = ("attn_q", "attn_v") if which == "n1" else ("ffn_gate", None)
    check_xh(res, tap, which + ".xh", name, ctx, model, f"blk.{l}.{first}.weight")
    if second:
        check_xh(res, tap, which + ".xh.v", name, ctx, model, f"blk.{l}.{second}.weight")
    return res


# ---- the GEMMs ----
def kernel_of(tap, wname):
    """the kernel the plan says this matrix took (KERNEL_*); 0 where the tapped layer never got there"""
    return tap["plan"][KERNEL_WORD[wname.split(".")[2]]]


def gemm_reference(tap, model, wname, act_name, sample=None, drop_last_block=False, wrong=None):
    """(exact [rows, m], bound, prompt rows, weight rows) of W . planes for the kernel the plan names for this matrix.
    drop_last_block / wrong: a kernel that is subtly wrong (the checker's own tests; wrong: fused_step_ref / q5k_step_ref k_pieces)"""
    t = _w(model, wname)
    m, k = t.shape
    acts = act_rows(tap, act_name)
    pr = np.arange(len(acts)) if sample is None else sample.prows(len(acts))
    wr = np.arange(m) if sample is None else sample.wrows(m)
    acts = [acts[r] for r in pr]
    kern = kernel_of(tap, wname)
    assert kern in (KERNEL_F16W, KERNEL_INT8, KERNEL_GEMV), (wname, tap["plan"])
    if kern == KERNEL_F16W:  # (the f16 GEMM read B'; otherwise the int8 kernels read the planes)
        assert wrong is None
        ap = weight_operands(np.ascontiguousarray(t.data).view(np.uint8).reshape(-1), F16W_FMT[t.typ], list(wr), k)[0]
        _, bp = b_prime(acts)
        if drop_last_block:
            bp = bp.copy()
            bp[:, -synth.BLOCK_ELEMS[t.typ]:] = 0.0
        return bp @ ap.T, GEMV_REL * (np.abs(bp) @ np.abs(ap).T) + 1e-30, pr, wr
    with Q5.q5k_rows():  # (Q5_K rows through q5k_step_ref; every other format dispatches back)
        e, b = R.row_dots_many(t, acts, wr, drop_last_block=drop_last_block, wrong=wrong)
    return e, b + 1e-30, pr, wr


def gemm_out(tap, out_name, parts_name, m, pr, wr):
    """the GEMM's stored output, with the pieces it left to a later launch added in float64"""
    got = rows_of(tap, out_name, m).astype(np.float64)
    if parts_name and parts_name in tap:
        got = got + np.asarray(tap[parts_name], dtype=np.float64).reshape(-1, got.shape[0], m).sum(axis=0)
    return got[np.ix_(pr, wr)]


def check_gemm(res, tap, model, wname, act_name, out_name, parts_name, what, ctx, sample=None):
    e, b, pr, wr = gemm_reference(tap, model, wname, act_name, sample)
    got = gemm_out(tap, out_name, parts_name, _w(model, wname).shape[0], pr, wr)
    check_f32(res, got.reshape(-1), e.reshape(-1), b.reshape(-1), what, ctx)
    return e, b, pr, wr


def check_qkv_gemm(tap, model, l, ctx, sample=None):
    res = Result("q|k|v gemm")
    for nm, wn in (("q", "attn_q"), ("k", "attn_k"), ("v", "attn_v")):
        check_gemm(res, tap, model, f"blk.{l}.{wn}.weight", "n1.act", nm, None, nm, ctx, sample)
    return res


# ---- k_qkv_epi_rows ----
@functools.lru_cache(maxsize=None)
def _rope_cs(pos, hd, rope_dim, neox):
    return R.rope_cs(pos, hd, rope_dim, neox)


def epi_reference(tap, model, l):
    """exact roped / scaled q, roped k, v of every row from the stored GEMM outputs, and their bounds: {name: (exact [B, n], bound)}"""
    s = model.shape
    hd, qwen2 = s.head_dim, s.arch == "qwen2"
    rope_dim = s.rope_dim if s.rope_dim is not None else hd
    pos0, B = tap["plan"]["pos0"], tap["plan"]["rows"]
    out = {}
    for nm, wname, n in (("q", "attn_q", s.dim), ("k", "attn_k", s.kv_dim), ("v", "attn_v", s.kv_dim)):
        e = rows_of(tap, nm, n).astype(np.float64)
        b = np.zeros_like(e)
        if qwen2:
            e = e + _f32(model, f"blk.{l}.{wname}.bias").astype(np.float64)[None, :]
            b = np.abs(e) * U
        if nm != "v":
            e, b = e.reshape(B, -1, hd).copy(), b.reshape(B, -1, hd).copy()
            for r in range(B):
                ia, ib, c, sn = _rope_cs(pos0 + r, hd, rope_dim, qwen2)
                a0, b0, ba, bb = e[r][:, ia].copy(), e[r][:, ib].copy(), b[r][:, ia].copy(), b[r][:, ib].copy()
                e[r][:, ia], e[r][:, ib] = a0 * c - b0 * sn, a0 * sn + b0 * c
                b[r][:, ia] = ba * np.abs(c) + bb * np.abs(sn) + 3 * U * (np.abs(a0 * c) + np.abs(b0 * sn))
                b[r][:, ib] = ba * np.abs(sn) + bb * np.abs(c) + 3 * U * (np.abs(a0 * sn) + np.abs(b0 * c))
            if nm == "q":
                scale = float(np.float32(1.0) / np.sqrt(np.float32(hd)))
                e = e * scale
                b = b * scale + np.abs(e) * U
        out[nm] = (e.reshape(B, -1), b.reshape(B, -1))
    return out


def cache_view(raw, form, n_kv, hd):
    return np.ascontiguousarray(raw).view(np.uint16 if form.kv_f16 else np.float32).reshape(n_kv, form.seq_cap, hd)


def check_epi(tap, kv_before, kv_after, model, l, form, ctx):
    """kv_before / kv_after: (K raw, V raw) of the layer from debug_kv, before and after the pass"""
    res = Result("k_qkv_epi_rows")
    s = model.shape
    pos0, B = tap["plan"]["pos0"], tap["plan"]["rows"]
    ref = epi_reference(tap, model, l)
    e, b = ref["q"]
    check_f32(res, tap["qr"], e.reshape(-1), b.reshape(-1) + 1e-30, "q", ctx)
    for nm, before, after in (("k", kv_before[0], kv_after[0]), ("v", kv_before[1], kv_after[1])):
        e, b = ref[nm]
        cv = cache_view(after, form, s.n_kv_heads, s.head_dim)
        got = cv[:, pos0:pos0 + B, :].transpose(1, 0, 2).reshape(B, -1)
        if form.kv_f16:
            ok = R.f16_code_between(got, e - b, e + b)
            if not ok.all():
                r, i = np.argwhere(~ok)[0]
                res.fails.append(f"{ctx} {res.launch}: {nm} cache row {r} (position {pos0 + r}) element {i}: f16 {R.f16v(got[r, i:i + 1])[0]:.6g} outside "
                                 f"f16([{e[r, i] - b[r, i]:.6g}, {e[r, i] + b[r, i]:.6g}]) ({int((~ok).sum())} of {ok.size})")
        else:
            check_f32(res, got.reshape(-1), e.reshape(-1), b.reshape(-1) + 1e-37, nm, ctx)
        bv = cache_view(before, form, s.n_kv_heads, s.head_dim)
        keep = np.ones(form.seq_cap, dtype=bool)
        keep[pos0:pos0 + B] = False
        same = cv[:, keep, :].view(np.uint8) == bv[:, keep, :].view(np.uint8)
        if not same.all():
            h, p = np.argwhere(~same)[0][:2]
            res.fails.append(f"{ctx} {res.launch}: {nm} cache: a row outside [{pos0}, {pos0 + B}) changed (kv head {h}, position "
                             f"{int(np.flatnonzero(keep)[p])})")
    return res


# ---- attention ----
def f64_causal_attention(q, kc_raw, vc_raw, n_heads, n_kv, hd, seq_cap, pos0, B):
    """float64 softmax(q K^T) V of row r over positions 0 .. pos0 + r on the kernel's inputs: q rounded to f16 (as the kernel and the
    reference, batch_matmul.rs:39, take it) and the f16 cache rows.  Nothing else is rounded -- the kernel's f16 probabilities are part of
    the error FLASH_ROWS_REL allows, as in tests/test_hip_flash_attention.py, whose reference this restates for a pass at pos0"""
    q16 = np.asarray(q, dtype=np.float32).astype(np.float16).astype(np.float64).reshape(B, n_heads, hd)
    kf = np.ascontiguousarray(kc_raw).view(np.float16).astype(np.float64).reshape(n_kv, seq_cap, hd)[:, :pos0 + B]
    vf = np.ascontiguousarray(vc_raw).view(np.float16).astype(np.float64).reshape(n_kv, seq_cap, hd)[:, :pos0 + B]
    grp = n_heads // n_kv
    out = np.zeros((B, n_heads, hd))
    mask = np.arange(pos0 + B)[None, :] > (pos0 + np.arange(B))[:, None]
    for h in range(n_heads):
        sc = q16[:, h, :] @ kf[h // grp].T
        sc[mask] = -np.inf
        p = np.exp(sc - sc.max(axis=1, keepdims=True))
        out[:, h, :] = (p / p.sum(axis=1, keepdims=True)) @ vf[h // grp]
    return out.reshape(-1)


SEQ_SUM_MAX = 1024  # softmax_row (fused_common.hpp): the row sum is the reference's scalar loop up to here, a block tree beyond


def oracle_probabilities(q, kc_raw, n_heads, n_kv, hd, seq_cap, pos, kv_f16):
    """the reference's f32 softmax row of every head at position pos (the first two ops of fused_step_ref.oracle_attention) [n_heads, pos + 1]"""
    odev = o.OracleDevice(thread_num=1)
    kc = o.OracleTensor.from_bytes(np.ascontiguousarray(kc_raw).view(np.uint8), o.F16 if kv_f16 else o.F32, [n_kv, seq_cap, hd], odev).resize(1, pos + 1)
    qt = o.OracleTensor.new(np.ascontiguousarray(q, dtype=np.float32).copy(), [n_heads, 1, hd], odev)
    return qt.batch_matmul(kc.transpose([0, 2, 1])).softmax_inplace(2).export().reshape(n_heads, pos + 1)


def long_row_hull(q, kc_raw, vc_raw, n_heads, n_kv, hd, seq_cap, pos, rel=None):
    """(lo, hi) [n_heads * hd] of what the exact long-row kernels (k_attn_scores / k_attn_softmax / k_attn_pv_rows) may leave for a row of
    pos + 1 > SEQ_SUM_MAX cached positions, f16 cache.  They are the reference's arithmetic at every rounding point but one: the softmax
    row sum S of the n = pos + 1 exponentials (non-negative f32 values) is a block tree, not the scalar loop.  Either order is within
    (n - 1) U of the exact sum, so S' / S_ref lies in 1 +- 2 n U; the true division e / S rounds once on either side: p' lies in
    p_ref (1 +- rel), rel = (2 n + 4) U.  Both ends are rounded to f16 (quantize_f32_f16 of the lhs, batch_matmul.rs:39; rounding is
    monotone), and the reference's serial f16 chain acc = f16(acc + f16(p v)) over the positions in order is run on the lower and on the
    upper end of every product -- every step is monotone in its operands, so the chain's value for ANY admissible S lies between them.
    Where no probability sits near an f16 rounding boundary lo == hi == the reference's own output, bit for bit (rel = 0: always)."""
    n = pos + 1
    rel = (2 * n + 4) * U if rel is None else rel
    p = oracle_probabilities(q, kc_raw, n_heads, n_kv, hd, seq_cap, pos, True).astype(np.float64)
    plo, phi = (p * (1 - rel)).astype(np.float16).astype(np.float64), (p * (1 + rel)).astype(np.float16).astype(np.float64)
    v = np.ascontiguousarray(vc_raw).view(np.float16).reshape(n_kv, seq_cap, hd)[:, :n].astype(np.float64)
    v = np.repeat(v, n_heads // n_kv, axis=0)  # [n_heads, n, hd]
    lo, hi = np.zeros((n_heads, hd), dtype=np.float16), np.zeros((n_heads, hd), dtype=np.float16)
    for t in range(n):
        a, b = (plo[:, t, None] * v[:, t, :]).astype(np.float16), (phi[:, t, None] * v[:, t, :]).astype(np.float16)  # (exact in f64: one rounding)
        lo = (lo.astype(np.float64) + np.minimum(a, b).astype(np.float64)).astype(np.float16)
        hi = (hi.astype(np.float64) + np.maximum(a, b).astype(np.float64)).astype(np.float16)
    return lo.astype(np.float64).reshape(-1), hi.astype(np.float64).reshape(-1)


def check_attention(tap, kv_after, model, l, form, ctx):
    res = Result("attention")
    s = model.shape
    pos0, B, kern = tap["plan"]["pos0"], tap["plan"]["rows"], tap["plan"]["attn_kernel"]
    q, got = rows_of(tap, "qr", s.dim), rows_of(tap, "attn", s.dim)
    if kern == ATTN_FLASH_ROWS:
        ref = f64_causal_attention(q, kv_after[0], kv_after[1], s.n_heads, s.n_kv_heads, s.head_dim, form.seq_cap, pos0, B)
        check_f32(res, got.reshape(-1), ref, np.full(ref.shape, FLASH_ROWS_REL * np.max(np.abs(ref))), "attn (flash rows)", ctx)
    else:  # the reference's arithmetic, bit for bit -- but for the long-row kernels' rows past SEQ_SUM_MAX positions: long_row_hull
        for r in range(B):
            if kern == ATTN_LONG_ROWS and pos0 + r + 1 > SEQ_SUM_MAX and form.kv_f16:
                lo, hi = long_row_hull(q[r], kv_after[0], kv_after[1], s.n_heads, s.n_kv_heads, s.head_dim, form.seq_cap, pos0 + r)
                check_f32(res, got[r], (lo + hi) / 2, (hi - lo) / 2, f"attn (long rows) row {r}", ctx)
                continue
            ref = R.oracle_attention(q[r], kv_after[0], kv_after[1], s.n_heads, s.n_kv_heads, s.head_dim, form.seq_cap, pos0 + r, form.kv_f16)
            same = got[r].view(np.uint32) == ref.view(np.uint32)
            if not same.all():
                i = int(np.flatnonzero(~same)[0])
                res.fails.append(f"{ctx} {res.launch}: row {r} (position {pos0 + r}) element {i}: {got[r, i]!r} != the reference's {ref[i]!r} "
                                 f"({int((~same).sum())} of {same.size} differ)")
                break
    check_planes_of(res, tap, "attn.act", got, "act_attn", ctx)
    check_xh(res, tap, "attn.xh", "attn.act", ctx, model, f"blk.{l}.attn_output.weight")
    return res


def check_planes_of(res, tap, name, values, what, ctx):
    """the tapped planes are the reference quantizer of rows we hold, byte for byte (a Q8_K set: d with its sign, the quants, the sixteen
    16-element sums); its class-major plane (name + ".qp") the permutation of its q"""
    qt = tap["qtype"][name]
    raw = np.asarray(tap[name]).reshape(values.shape[0], -1)
    for r in range(values.shape[0]):
        exp = o.quantize(np.ascontiguousarray(values[r], dtype=np.float32), qt)
        if not np.array_equal(exp, raw[r]):
            i = int(np.flatnonzero(exp != raw[r])[0])
            res.fails.append(f"{ctx} {res.launch}: {what} row {r} differs from the reference quantizer at byte {i} (block {i // synth.BLOCK_BYTES[qt]})")
            return
    if qt == o.Q8_K:
        if name + ".qp" not in tap:
            res.fails.append(f"{ctx} {res.launch}: {what}: the Q8_K planes came without their class-major plane")
            return
        qp = np.ascontiguousarray(tap[name + ".qp"]).view(np.int8).reshape(values.shape[0], -1)
        for r in range(values.shape[0]):
            a = R.parse_act(raw[r], qt)
            n0 = len(res.fails)
            R.check_q8k_own(res, a, qp[r], f"{what} row {r}", ctx)
            if len(res.fails) > n0:
                return


# ---- wo / ffn_down ----
def check_wo(tap, model, l, ctx, sample=None):
    res = Result("wo")
    check_gemm(res, tap, model, f"blk.{l}.attn_output.weight", "attn.act", "wo.tmp", "wo.parts", "wo", ctx, sample)
    return res


def check_down(tap, model, l, ctx, sample=None):
    res = Result("ffn_down")
    check_gemm(res, tap, model, f"blk.{l}.ffn_down.weight", "hid.act", "down.tmp", "down.parts", "ffn_down", ctx, sample)
    if "down.x" in tap:  # k_res_epi right behind it: x = ffn_down + x, one rounding
        dim = model.shape.dim
        x0, t = rows_of(tap, "n2.x", dim).astype(np.float64), rows_of(tap, "down.tmp", dim).astype(np.float64)
        check_f32(res, tap["down.x"], (x0 + t).reshape(-1), (U * (np.abs(x0) + np.abs(t)) + 1e-37).reshape(-1), "x", ctx)
    return res


# ---- gate | up ----
def check_gateup(tap, model, l, ctx, sample=None, twin=None):
    """twin: the tap of the same pass in a context created with PREFILL_SEPARATE_F16_ROWS (h_done == 2 only: the h this launch never stores)"""
    res = Result("gate|up")
    hidden = model.shape.hidden
    h_done = tap["plan"]["h_done"]
    qt = tap["qtype"]["hid.act"]
    if qt == o.Q8_K and h_done == 2:
        res.fails.append(f"{ctx} gate|up: h_done == 2 (the row quantizer inside the GEMM) does not exist for Q8_K rows")
        return res
    if h_done == 0:
        for nm, wn in (("g", "ffn_gate"), ("u", "ffn_up")):
            check_gemm(res, tap, model, f"blk.{l}.{wn}.weight", "n2.act", nm, None, nm, ctx, sample)
        g, u = np.asarray(tap["g"], dtype=np.float64), np.asarray(tap["u"], dtype=np.float64)
        lo, hi, ref = R.silu_mul_interval(g, 0.0, u, 0.0)
        if "hid.h" in tap:  # k_gateup_epi left h as f32 (over g): no interval excuse
            h = rows_of(tap, "hid.h", hidden)
            check_in_interval(res, h, lo.reshape(h.shape), hi.reshape(h.shape), "h", ctx)
            check_planes_of(res, tap, "hid.act", h, "act_hid (of the stored h)", ctx)
        elif qt == o.Q8_K:
            res.fails.append(f"{ctx} gate|up: a Q8_K-row pass that leaves g and u stores hid.h; the tap has none")
        else:
            R.QuantIntervals(lo, hi, ref, qt).check(tap["hid.act"], res, "act_hid", ctx)
    else:
        src = tap if h_done == 1 else twin
        if src is None:
            res.fails.append(f"{ctx} gate|up: h_done == 2 needs the twin tap")
            return res
        if src["plan"]["h_done"] != 1 or src["plan"]["rows"] != tap["plan"]["rows"]:
            res.fails.append(f"{ctx} gate|up: the twin does not store h ({src['plan']})")
            return res
        if h_done == 2 and not np.array_equal(np.asarray(src["n2.act"]), np.asarray(tap["n2.act"])):
            res.fails.append(f"{ctx} gate|up: the twin's gate | up launch read other planes")
            return res
        g, bg, pr, wr = gemm_reference(src, model, f"blk.{l}.ffn_gate.weight", "n2.act", sample)[:4]
        u, bu = gemm_reference(src, model, f"blk.{l}.ffn_up.weight", "n2.act", sample)[:2]
        lo, hi, _ = R.silu_mul_interval(g, bg, u, bu)
        h = rows_of(src, "g", hidden)
        hs = h[np.ix_(pr, wr)].astype(np.float64)
        # (as an f32 value inside the hull: distance from its middle against its half width)
        check_f32(res, hs.reshape(-1), ((lo + hi) / 2).reshape(-1), ((hi - lo) / 2).reshape(-1) + 1e-37, "h", ctx)
        check_planes_of(res, tap, "hid.act", h, "act_hid (of the stored h)", ctx)
    check_xh(res, tap, "hid.xh", "hid.act", ctx, model, f"blk.{l}.ffn_down.weight")
    return res


# ---- the tail ----
def check_tail(tap, model, l, ctx):
    res = Result("final norm + classifier")
    s = model.shape
    last = np.asarray(tap["last.x"], dtype=np.float32)
    if l == s.n_layers - 1:
        want = rows_of(tap, "down.x", s.dim)[-1]
        if not np.array_equal(last.view(np.uint32), want.view(np.uint32)):
            res.fails.append(f"{ctx} {res.launch}: the final norm did not read row B - 1 of pf_x")
    lo, hi, ref = R.norm_interval(last, _f32(model, "output_norm.weight"), s.rms_eps, s.dim)
    if "cls.xn" in tap:  # the final norm's f32 row is stored: no interval excuse
        xn = np.asarray(tap["cls.xn"], dtype=np.float32).reshape(1, -1)
        check_in_interval(res, xn, lo[None, :], hi[None, :], "cls.xn", ctx)
        check_planes_of(res, tap, "cls.act", xn, "cls.act (of the stored cls.xn)", ctx)
    elif tap["qtype"]["cls.act"] == o.Q8_K:
        res.fails.append(f"{ctx} {res.launch}: a Q8_K classifier row comes with cls.xn; the tap has none")
    else:
        R.QuantIntervals(lo, hi, ref, tap["qtype"]["cls.act"]).check(tap["cls.act"], res, "cls.act", ctx)
    t = model.tensors["output.weight"] if "output.weight" in model.tensors else model.tensors["token_embd.weight"]
    with Q5.q5k_rows():
        e, b = R.row_dots(t, act_rows(tap, "cls.act")[0])
    check_f32(res, tap["logits"], e, b + 1e-30, "logits", ctx)
    return res


def check_pass(tap, tokens, kv_before, kv_after, model, l, form, ctx, sample=None, twin=None):
    """every launch of the tapped layer of one pass (and its tail) -> {launch: Result}"""
    assert tap["plan"]["rows"] == len(tokens)
    out = {}
    if l == 0:
        out["embedding"] = check_embedding(tap, model, tokens, ctx)
    out["norm n1"] = check_norm(tap, model, l, "n1", ctx)
    out["q|k|v gemm"] = check_qkv_gemm(tap, model, l, ctx, sample)
    out["k_qkv_epi_rows"] = check_epi(tap, kv_before, kv_after, model, l, form, ctx)
    out["attention"] = check_attention(tap, kv_after, model, l, form, ctx)
    out["wo"] = check_wo(tap, model, l, ctx, sample)
    out["norm n2"] = check_norm(tap, model, l, "n2", ctx)
    out["gate|up"] = check_gateup(tap, model, l, ctx, sample, twin)
    out["ffn_down"] = check_down(tap, model, l, ctx, sample)
    out["tail"] = check_tail(tap, model, l, ctx)
    return out


failures = R.failures
