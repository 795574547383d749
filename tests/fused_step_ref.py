"""The five launches of the fast fused decode step (enqueue_segment_t, crabml_amd/csrc/fused.hip: k_qkv, attention, k_gemv_res_nq
for wo, k_gateup_q, k_gemv_res_nq for ffn_down, then the classifier) restated in float64, ONE FUNCTION PER LAUNCH.

Every function takes the bytes its launch read -- from the tap, HipLlamaRunner.debug_tap / crabml_hip_llama_debug_tap -- and the
model's raw weights (synth.RawModel), computes the exact value of every output and a rigorous bound on what f32 arithmetic in any
order may do to it, and compares with what the launch left.  Between launches there is flip noise (one ulp in, one quant out:
tests/helpers.FAST_TOL); inside one launch, given its input bytes, the output is determined up to f32 re-association, so the
bounds here are derived from roundings, never from what a device was seen to do:

  U = 2^-24, the unit roundoff of f32 (round to nearest).

  row dot of nb blocks (Q4_0 / Q8_0): the kernel's block term is ((float)sumi * d_w) * d_x -- sumi is an exact integer, two
      roundings -- and the nb terms are added in some order, at most nb - 1 roundings: |f32 - exact| <= (nb + C_DOT) U sum_b |t_b|
      with C_DOT = 3 (two for the term, minus one, plus two spare for the second-order terms: nb^2 U^2 << 2 U for any row here).
      That is the bound used.  sum_b |t_b| <= sum_i |w_i x_i| on the dequantized operands, so for every row of up to 332 blocks
      (10624 elements) it lies BELOW the project's re-association bound GEMV_REL * sum_i |w_i x_i| (tests/helpers.py: 2e-5 = 335 U),
      and for longer rows (ffn_down at hidden 14336 has 448 blocks) it is the derived replacement.
  Q4_1: the term is f16(d_w d_x) * sumi + f16(m s) (buf_q4_1.rs:276: the f16 products are part of the expression and restated
      exactly), two roundings on |f16(d_w d_x) sumi| + |f16(m s)|: bound (nb + C_DOT) U sum_b (|f16(d_w d_x) sumi| + |f16(m s)|), never
      more than 8 GEMV_REL sum_i |w_i x_i| (the x8 of tests/test_hip_gemv.py: the two parts of a term cancel).
  1 / rms of the deferred (hop-free) form, RmsTail / rms_finish (gemv_core.hpp): rsq(sum_c s_c * inv_n + eps) with inv_n the f32
      1.0f / (float)n the host hands over and s_c the n / 32 chunk sums THE LAUNCH READ (the tapped rsums; that they are the sums of
      squares of the stored row is the producing launch's check).  The restatement uses the same f32 inv_n and eps, so only the
      kernel's own roundings count: ceil(n / 2048) lane adds, 6 tree levels, one multiply, one add, all terms positive -- a relative
      error of the argument of at most (ceil(n / 2048) + 8) U =: R_INV(n) U; the reciprocal square root halves it and v_rsq_f32
      adds one ulp (2 U): rel(1 / rms) <= (R_INV(n) / 2 + 2) U, 6.5 U for every row up to 2048 elements.
  the exact norm, sqrtf(sum / (float)n + eps) then (v / rms) * w (norm_quant_block, nq_epilogue; n is exact in f32): the sum of
      squares comes from x itself -- a square is one rounding, a chunk 31 more adds, the tree over the chunk sums ceil(n / 2048) + 6,
      the division and the add two more: (32 + ceil(n / 2048) + 6 + 2) U =: R_SS(n) U on the argument, (R_SS(n) / 2 + 1) U on rms, two
      more roundings for the division and the product.
  rope: r0 = a c - b s, r1 = a s + b c with the reference's own f32 c, s: an input bound (b_a, b_b) goes through as b_a |c| + b_b |s|,
      the three roundings add 3 U (|a c| + |b s|).

Quantized rows whose f32 input the device never stores (act_hid; act_dim in the exact-norm form) get the INTERVAL CHECK
(QuantIntervals): the reference quantizer (buf_q8_0.rs:87-134) divides by the f32 scale dd = max|v| / 127 and stores f16(dd), so
per block (1) the device's d is one of the f16 codes between f16(dd_lo) and f16(dd_hi), (2) every quant is trunc(v / dd) for some
v and dd of the intervals -- equality with the reference's quant wherever the interval of v / dd holds no integer, either
neighbour where it does, never more than one step --, (3) the share of elements excused under (2) is computed from the reference
alone and capped at EXCUSED_CAP per (launch, shape) before the device's values are looked at.

THE K-QUANT STEP (enqueue_segment_k: k_qkv<Q4_K>, attention, k_gemv_res_nq<Q4_K, SPLIT, QIN> for wo, k_gateup_k_lds, the same for
ffn_down, the classifier; k_gemv_res / k_gateup and the stand-alone norm and quantizer launches without the norm epilogue and for Q4_1
layers in front of a classifier of another format).  check_layer dispatches on the plan words the enqueue code wrote (path = 2):

  Q4_K row dot (q4k_term, gemv_core.hpp): a lane's PIECE (pair p, class half h) is 16 bytes of nibbles -- of each of the two 32-groups
      of a 64-element pair the 16 elements e with e % 8 in 4 h .. 4 h + 3, dwords 4 h .. 4 h + 3 of the class-major planes; k_pieces
      regroups weights and q8 by e % 8 to form exactly these -- with exact integers isum = sc_lo sum(q4 q8 | low) + sc_hi sum(q4 q8 |
      high) < 2^22 and msum = m_lo bsum_lo + m_hi bsum_hi < 2^19 (bsums: entries 4 p + h and 4 p + 2 + h of the plane the launch read,
      the contiguous halves, which is all the minimum term needs; q8: the CLASS-MAJOR plane qp it read, put back in element order), and the
      f32 term f32(d_w d8) isum - f32(dmin_w d8) msum: the two scale products, the two products with the integers and the subtraction,
      FIVE roundings (the build has -ffp-contract=off; a fused multiply-add would only remove some).  With A = |d_w d8 isum| + |dmin_w
      d8 msum| the term is off by at most (2 U |dd isum| + 2 U |dmin msum|)(1 + U) + U |term| <= 3 U A (1 + 2 U).  The 8 nsb terms of a
      row are then added in some order -- a lane's pieces in ascending order, the 64 lanes through a tree, the leading pieces of the
      prologue forms first --, n - 1 additions, each off by at most U times a partial sum of |terms| <= U sum A (1 + 3 U):
      |f32 - exact| <= (n_terms + C_K) U sum A with C_K = 3: three for the term, minus one, plus one for every second-order term
      (n_terms^2 U^2 < 0.02 U for the longest row here, 448 pieces).
  Q6_K row dot (rows_partial_q6k): a piece is the low nibbles of scale group g and the high nibbles of group g + 4, with exact integers
      a = sc_g sum((q6 - 32) q8), b = sc_{g+4} sum(..) below 2^24 (the -32 as -32 bsum of the plane the launch read) and the f32 term
      f32(d_w d8) * f32((float)a + (float)b): THREE roundings on A = |d_w d8| (|a| + |b|); the same sum: (n_terms + C_K) U sum A.
      Both bounds lie below 8 GEMV_REL sum_i |w_i x_i| on every row of the shapes tested (asserted by tests/test_fused_step_ref.py;
      the Q6_K one below GEMV_REL sum_i |w_i x_i| itself up to 41 super-blocks, as A <= sum |w_i x_i| there); for longer rows
      (ffn_down at hidden 14336: 56 super-blocks, 448 terms) they are the derived replacement.
  Q8_K planes whose f32 input is stored (act_attn, act_hid, the planes behind a stand-alone norm launch) are the reference quantizer's
      bytes (o.quantize: d, q, bsums), and qp the class-major permutation of q (byte 4 (e % 8) + e / 8 of a 32-group holds element e:
      q8k_store_class_major, devutil.hpp).  Where the consuming kernel quantizes in its prologue (qmode 1) nothing is stored: the
      checker takes o.quantize of the tapped f32 row as the rhs, so a wrong in-LDS quantizer shows as a row-dot failure.
  Q8_K planes whose f32 input is never stored (the norm epilogue of wo / ffn_down) get QuantIntervalsK: the reference (buf_q8_k.rs:84-131)
      takes mx = the first element of maximal |v|, scale = -128 / mx (one rounding), q = min(round_half_away(scale v), 127) (one
      rounding of the product), d = 1 / scale (one more).  From [lo, hi] per element: the max-holder is one of the elements whose
      upper magnitude reaches M = max of the lower magnitudes, |mx| in [M, the largest upper magnitude among them], separately for
      either sign of mx (d has the opposite sign of mx: the device's d names the class, which must be an admissible one); |scale| in
      128 / |mx| (1 +- U), |d| in 1 / |scale| (1 +- U); scale v over the corners (1 +- U) gives [q_lo, q_hi]: equality with the
      reference's quant where q_lo == q_hi, else either neighbour and never more than one step; bsums and qp are exact functions of
      the device's own q.  The excused share comes from the reference alone and is capped by EXCUSED_CAP.  A product exactly on a
      half-integer and a maximum held by elements of either sign are what an interval excuses: that ties round AWAY from zero and that
      the FIRST holder wins is held only where the f32 row is stored (the byte comparison above), not for these planes.
  wo in x_only form (k_norm_in, the default fast Q4_K step) leaves x and split_wo sums of squares per 32-row chunk: 16 (two parts) or
      32 (one) squares and their adds, all positive: within 33 U of the sum of squares of the stored x, part by part.
  gate | up NORMIN normalizes and quantizes in LDS; its planes never reach memory.  A twin context with NO_K_NORM_IN on the same
      tokens leaves them: wo.x must be bit-equal between the two taps, the twin's planes pass QuantIntervalsK, and the NORMIN launch's h
      is held to act(g) * u of THOSE planes within the dot bounds passed through the activation's hull.  One quant off by a step moves a
      row dot by |w_i| d8, orders of magnitude above the bound: that is what pins "bit for bit the planes wo used to leave".
      (The twin's own chunk sums live in epoch-stamped granules and are not tapped; the NORMIN launch's sums are held to the stored x.)"""
import math
from dataclasses import dataclass, field

import numpy as np

from crabml_amd import synth
from oracle import oracle as o
from tests.helpers import GEMV_REL

U = 2.0 ** -24
C_DOT = 3
C_K = 3      # K-quant row dots: see the module docstring
EXCUSED_CAP = 0.20
FLASH_REL = 2e-5  # tests/test_hip_flash_attention.py: k_attn_flash against float64 on the same f16 inputs, of max|out|


def r_ss(n):
    """relative error factor (in U) of the f32 sum of squares of n elements in 32-element chunks (see the module docstring)"""
    return 32 + math.ceil(n / 2048) + 6 + 2


@dataclass
class Form:
    """which form of the step a context runs (the launch plan, from the code's own predicates in fused.hip)"""
    defer: bool            # hop-free norm: c->plan.defer_norm (Q4_0 / Q8_0, norm epilogue, not EXACT_NORM)
    kv_f16: bool
    seq_cap: int
    flash_from: int = 0    # > 0: cached positions (pos + 1) from which k_attn_flash runs (c->plan.attn_long_from with attn_flash)


@dataclass
class Result:
    launch: str
    fails: list = field(default_factory=list)
    worst: float = 0.0     # max error / bound over the launch's f32 outputs
    excused: dict = field(default_factory=dict)  # plane name -> excused share (interval check)

    def ratio(self, err, bound, what, ctx):
        err, bound = np.asarray(err, dtype=np.float64).reshape(-1), np.asarray(bound, dtype=np.float64).reshape(-1)
        r = err / np.maximum(bound, 1e-300)
        if r.size:
            self.worst = max(self.worst, float(np.max(r)))
            bad = np.flatnonzero(~(r <= 1.0))
            if bad.size:
                i = int(bad[np.argmax(r[bad])])
                self.fails.append(f"{ctx} {self.launch}: {what} row {i}: error {err[i]:.4g} > bound {bound[i]:.4g} ({bad.size} of {r.size} rows)")

    def ok(self):
        return not self.fails


def shrink_residual(model, log2=7):
    """Every block scale of token_embd, attn_output and ffn_down times 2^-log2, in place: the residual stream of the model shrinks
    by that factor (what feeds it does; the normalized activations do not change).  RMSNorm's eps moves 1 / rms by
    0.5 * eps / (mean square + eps) relative.  The synthetic models' residual stream has a mean square of 0.3 .. 200: taking 1e-6 for
    1e-5 there changes 1 / rms by 1.3e-5 at the low end (about 250 f32 ulps), by one ulp near 40 and by nothing from ~75 on --
    mostly inside what re-association alone may do to a row dot.  On the shrunk model (mean square 2e-5 .. 1e-2) it is 3e-4 .. 0.2:
    the model on which a wrong eps cannot pass in any launch."""
    f = np.float16(2.0 ** -log2)
    for name, t in model.tensors.items():
        if not (name == "token_embd.weight" or name.endswith("attn_output.weight") or name.endswith("ffn_down.weight")):
            continue
        assert t.typ in (synth.Q4_0, synth.Q8_0, synth.Q4_1, synth.Q4_K, synth.Q6_K), name
        blk = t.data.reshape(-1, synth.BLOCK_BYTES[t.typ])
        for lo in {synth.Q4_1: (0, 2), synth.Q4_K: (0, 2), synth.Q6_K: (208,)}.get(t.typ, (0,)):  # d | m; d | dmin; Q6_K's d behind the quants
            d = blk[:, lo:lo + 2].copy().view(np.float16)
            blk[:, lo:lo + 2] = (d * f).astype(np.float16).view(np.uint8)
    return model


# ---- block byte layouts (the reference's: buf_q8_0.rs:8-13, buf_q8_1.rs:73-79, buf_q8_k.rs:6-12, buf_q4_0.rs, buf_q4_1.rs, buf_q6_k.rs) ----
def f16v(bits):
    return np.ascontiguousarray(bits).view(np.float16).astype(np.float64)


def _u16(b):
    return np.ascontiguousarray(b).view(np.uint16)[..., 0]


def parse_act(raw, qt):
    """activation blocks -> dict(d [nb] f64, q [nb, be] int64, s [nb] f64 (Q8_1), d_bits)"""
    raw = np.ascontiguousarray(raw).view(np.uint8)
    if qt == o.Q8_0:
        b = raw.reshape(-1, 34)
        return {"qt": qt, "d": f16v(_u16(b[:, 0:2])), "d_bits": _u16(b[:, 0:2]), "q": np.ascontiguousarray(b[:, 2:]).view(np.int8).astype(np.int64)}
    if qt == o.Q8_1:
        b = raw.reshape(-1, 36)
        return {"qt": qt, "d": f16v(_u16(b[:, 0:2])), "d_bits": _u16(b[:, 0:2]), "s": f16v(_u16(b[:, 2:4])), "s_bits": _u16(b[:, 2:4]),
                "q": np.ascontiguousarray(b[:, 4:]).view(np.int8).astype(np.int64)}
    if qt == o.Q8_K:
        b = raw.reshape(-1, 292)
        return {"qt": qt, "d": np.ascontiguousarray(b[:, 0:4]).view(np.float32)[:, 0].astype(np.float64),
                "q": np.ascontiguousarray(b[:, 4:260]).view(np.int8).astype(np.int64),
                "bsums": np.ascontiguousarray(b[:, 260:292]).view(np.int16).astype(np.int64)}
    raise ValueError(qt)


_CM = np.array([4 * (e % 8) + e // 8 for e in range(32)])  # element e of a 32-group -> its byte in the class-major plane (devutil.hpp)


def class_major(q):
    """quants in element order -> the class-major plane qp (any shape whose size is a multiple of 32)"""
    g = np.asarray(q).reshape(-1, 32)
    out = np.empty_like(g)
    out[:, _CM] = g
    return out.reshape(np.shape(q))


def from_class_major(p):
    g = np.asarray(p).reshape(-1, 32)
    return g[:, _CM].reshape(np.shape(p))


def tap_act(tap, name):
    """the activation blocks of field `name` as the consuming launch read them: a Q8_K set with its class-major plane (field
    name + ".qp", which the Q4_K rows read) put back in element order as "qp_q" """
    a = parse_act(tap[name], tap["qtype"][name])
    if a["qt"] == o.Q8_K and name + ".qp" in tap:
        a["qp_q"] = from_class_major(np.ascontiguousarray(tap[name + ".qp"]).view(np.int8).astype(np.int64)).reshape(a["q"].shape)
    return a


def act_values(a):
    """dequantized activation, f64 (exact)"""
    return (a["q"] * a["d"][:, None]).reshape(-1)


def weight_rows(t, r0, r1):
    """rows [r0, r1) of a weight tensor (synth.RawTensor) -> per-format dict of exact integer / f64 fields, [rows, nb, ...]"""
    rows, k = t.shape
    typ = t.typ
    bb, be = synth.BLOCK_BYTES[typ], synth.BLOCK_ELEMS[typ]
    nb = k // be
    b = np.ascontiguousarray(t.data).view(np.uint8).reshape(rows, nb, bb)[r0:r1]
    if typ == synth.Q8_0:
        return {"typ": typ, "d": f16v(_u16(b[:, :, 0:2])), "q": np.ascontiguousarray(b[:, :, 2:]).view(np.int8).astype(np.float64)}
    if typ in (synth.Q4_0, synth.Q4_1):
        qs = b[:, :, (2 if typ == synth.Q4_0 else 4):]
        nib = np.concatenate([qs & 0x0F, qs >> 4], axis=2).astype(np.float64)  # element j < 16: low nibble of byte j; j >= 16: high nibble of byte j - 16
        w = {"typ": typ, "d": f16v(_u16(b[:, :, 0:2]))}
        if typ == synth.Q4_0:
            w["q"] = nib - 8.0
        else:
            w["q"] = nib
            w["m"] = f16v(_u16(b[:, :, 2:4]))
        return w
    if typ == synth.Q6_K:  # ql[128] | qh[64] | scales i8[16] | d f16 (buf_q6_k.rs:11-18); element order of dequantize (buf_q6_k.rs:93-120)
        ql, qh = b[:, :, 0:128].astype(np.int64), b[:, :, 128:192].astype(np.int64)
        sc = np.ascontiguousarray(b[:, :, 192:208]).view(np.int8).astype(np.float64)
        q = np.empty(b.shape[:2] + (256,), dtype=np.float64)
        scale = np.empty_like(q)
        for half in range(2):
            lq, hq = ql[:, :, 64 * half:64 * half + 64], qh[:, :, 32 * half:32 * half + 32]
            for j, (lo, sh) in enumerate(((lq[:, :, 0:32] & 0xF, 0), (lq[:, :, 32:64] & 0xF, 2), (lq[:, :, 0:32] >> 4, 4), (lq[:, :, 32:64] >> 4, 6))):
                base = 128 * half + 32 * j
                q[:, :, base:base + 32] = (lo | (((hq >> sh) & 3) << 4)) - 32
                for g in range(2):
                    scale[:, :, base + 16 * g:base + 16 * g + 16] = sc[:, :, 8 * half + 2 * j + g][:, :, None]
        return {"typ": typ, "d": f16v(_u16(b[:, :, 208:210])), "q": q * scale, "q6": q, "sc": sc}
    if typ == synth.Q4_K:  # d f16 | dmin f16 | scales[12] | qs[128] (buf_q4_k.rs:13-19); the 6-bit fields: util.rs:19-27; order: buf_q4_k.rs:24-47
        s12 = b[:, :, 4:16].astype(np.int64)
        sc, mn = np.empty(b.shape[:2] + (8,)), np.empty(b.shape[:2] + (8,))
        for j in range(4):
            sc[:, :, j], mn[:, :, j] = s12[:, :, j] & 63, s12[:, :, j + 4] & 63
            sc[:, :, j + 4] = (s12[:, :, j + 8] & 0xF) | ((s12[:, :, j] >> 6) << 4)
            mn[:, :, j + 4] = (s12[:, :, j + 8] >> 4) | ((s12[:, :, j + 4] >> 6) << 4)
        qs = b[:, :, 16:144].reshape(b.shape[0], b.shape[1], 4, 32)
        q = np.stack([qs & 0x0F, qs >> 4], axis=3).reshape(b.shape[0], b.shape[1], 256).astype(np.float64)  # pair p: 32 low nibbles, 32 high
        return {"typ": typ, "d": f16v(_u16(b[:, :, 0:2])), "dmin": f16v(_u16(b[:, :, 2:4])), "sc": sc, "mn": mn, "q": q}
    raise ValueError(f"weight type {typ}")


def k_values(w):
    """the dequantized elements of K-quant weight rows (weight_rows), f64, [rows, nsb * 256] -- sum |w_i x_i| of the project's bound"""
    if w["typ"] == synth.Q6_K:
        return (w["q"] * w["d"][:, :, None]).reshape(w["q"].shape[0], -1)
    r, nsb = w["d"].shape
    v = (w["d"][:, :, None] * w["sc"])[:, :, :, None] * w["q"].reshape(r, nsb, 8, 32) - (w["dmin"][:, :, None] * w["mn"])[:, :, :, None]
    return v.reshape(r, -1)


def k_pieces(w, act, wrong=None):
    """Q4_K / Q6_K weight rows (weight_rows) against one row's Q8_K blocks: per piece of every row (the kernels' 16-byte unit, 8 per
    super-block) the exact term and the magnitude A its roundings act on -> (terms, A), each [rows, nsb, 8].  wrong: a kernel that is
    subtly wrong in the named way (the checker's own tests)"""
    typ = w["typ"]
    r, nsb = w["d"].shape
    d8, bs = act["d"], act["bsums"].astype(np.float64)
    assert d8.size == nsb, (d8.size, nsb)
    if typ == synth.Q4_K:
        # a lane's piece (pair p, class half h) takes, of either 32-group of the pair, the elements e with e % 8 in 4 h .. 4 h + 3 (dwords
        # 4 h .. of the class-major planes: q4k_loadx / q4k_ints): [32-group g, e / 8, class half h, class within the half]
        x = act.get("qp_q", act["q"]).astype(np.float64).reshape(nsb, 8, 4, 2, 4)
        S = np.einsum("rsgahi,sgahi->rsgh", w["q"].reshape(r, nsb, 8, 4, 2, 4), x)
        sc, mn = w["sc"].copy(), w["mn"].copy()
        if wrong == "scale_neighbour":
            sc[:, 0, 2] = w["sc"][:, 0, 3]
        if wrong == "min_neighbour":
            mn[:, 0, 2] = w["mn"][:, 0, 3]
        T = sc[:, :, :, None] * S
        # (the minimum term only needs every bsums entry once per super-block: piece (p, h) takes entries 4 p + h and 4 p + 2 + h, the
        # CONTIGUOUS halves h of its two groups, as q4k_loadx does)
        M = mn[:, :, :, None] * bs.reshape(nsb, 8, 2)[None]
        isum, msum = T[:, :, 0::2] + T[:, :, 1::2], M[:, :, 0::2] + M[:, :, 1::2]  # piece (pair p, half h): groups 2 p and 2 p + 1
        a = (w["d"] * d8[None])[:, :, None, None] * isum
        b = (w["dmin"] * d8[None])[:, :, None, None] * msum
        terms = a - b
        if wrong == "dmin_plus":
            terms[:, 0, 1, 0] = (a + b)[:, 0, 1, 0]
        return terms.reshape(r, nsb, 8), (np.abs(a) + np.abs(b)).reshape(r, nsb, 8)
    assert typ == synth.Q6_K
    x = act["q"].astype(np.float64).reshape(nsb, 16, 16)
    # sum (q6 - 32) q8 as the kernel forms it: the 6-bit levels against q8, minus 32 times the bsums entry it read
    G = np.einsum("rsgi,sgi->rsg", w["q6"].reshape(r, nsb, 16, 16) + 32.0, x) - 32.0 * bs[None]
    sc = w["sc"]
    if wrong == "q6_scale_shift":
        sc = sc.copy()
        sc[:, 0, 5] = w["sc"][:, 0, 6]
    G = (sc * G).reshape(r, nsb, 2, 2, 4)  # group 8 h + 4 hi + j; a piece: the low nibbles of group 8 h + j, the high of 8 h + 4 + j
    dd = (w["d"] * d8[None])[:, :, None, None]
    return (dd * (G[:, :, :, 0] + G[:, :, :, 1])).reshape(r, nsb, 8), (np.abs(dd) * (np.abs(G[:, :, :, 0]) + np.abs(G[:, :, :, 1]))).reshape(r, nsb, 8)


def _chunk_dots(w, typ, act, k, drop_last_block, wrong=None):
    """(exact, bound) of the weight rows `w` (weight_rows) against one row's activation blocks: row_dots' arithmetic"""
    if typ == synth.Q4_1:
        assert act["qt"] == o.Q8_1
        nb = k // 32
        keep = np.ones(nb)
        if drop_last_block:
            keep[-1] = 0.0
        xq = act["q"].astype(np.float64)
        xd = (act["q"] * act["d"][:, None]).astype(np.float64)
        sumi = np.einsum("rbi,bi->rb", w["q"], xq)
        P = (w["d"] * act["d"][None, :]).astype(np.float16).astype(np.float64)  # f16 products, rounded once (the exact product fits f64)
        M = (w["m"] * act["s"][None, :]).astype(np.float16).astype(np.float64)
        exact = ((P * sumi + M) * keep).sum(axis=1)
        deq = np.einsum("rbi,bi->r", np.abs(w["q"] * w["d"][:, :, None] + w["m"][:, :, None]), np.abs(xd))
        terms = (np.abs(P * sumi) + np.abs(M)).sum(axis=1)
        return exact, np.minimum(8 * GEMV_REL * deq, (nb + C_DOT) * U * terms)
    if typ in (synth.Q4_K, synth.Q6_K):  # x Q8_K: the bound of the module docstring, (n_terms + C_K) U sum A
        assert act["qt"] == o.Q8_K
        terms, A = k_pieces(w, act, wrong)
        if drop_last_block:  # (a K-quant row's block is a super-block)
            terms = terms[:, :-1]
        return terms.sum(axis=(1, 2)), (A.shape[1] * 8 + C_K) * U * A.sum(axis=(1, 2))
    # Q4_0 / Q8_0 x Q8_0: products of exact small integers and f16 scales
    x = act_values(act)
    assert x.size == k, (x.size, k)
    if drop_last_block:
        x = x.copy()
        x[-32:] = 0.0
    nblk = k // 32
    x3 = x.reshape(nblk, 32)
    wd = (w["q"] * w["d"][:, :, None]).reshape(w["q"].shape[0], nblk, 32)  # exact in f64
    terms = np.einsum("rbi,bi->rb", wd, x3)
    return terms.sum(axis=1), (nblk + C_DOT) * U * np.abs(terms).sum(axis=1)


def row_dots(t, act, chunk=256, drop_last_block=False, wrong=None):
    """W . x for every row of t against the activation blocks `act`: (exact f64 [rows], bound f64 [rows]) -- the bound of the module
    docstring for an f32 evaluation of the reference's block expression in ANY order of the blocks.  drop_last_block: the dot
    without each row's last 32 elements (a K-quant row's: last super-block), what a kernel whose block loop stops one early computes;
    wrong: the name of another wrong kernel of k_pieces (both: the checker's own tests)"""
    e, b = row_dots_many(t, [act], None, chunk, drop_last_block, wrong)
    return e[0], b[0]


def row_dots_many(t, acts, wrows=None, chunk=256, drop_last_block=False, wrong=None):
    """row_dots for several rhs rows (the prompt pass): (exact [len(acts), rows], bound) -- the weight rows are unpacked once per chunk.
    wrows: the weight rows to take (sorted indices; None = all)"""
    rows, k = t.shape
    sel = np.arange(rows) if wrows is None else np.asarray(wrows)
    exact, bound = np.empty((len(acts), sel.size)), np.empty((len(acts), sel.size))
    for r0 in range(0, rows, chunk):
        at = np.flatnonzero((sel >= r0) & (sel < r0 + chunk))
        if at.size == 0:
            continue
        w = weight_rows(t, r0, min(rows, r0 + chunk))
        w = {key: (v[sel[at] - r0] if isinstance(v, np.ndarray) else v) for key, v in w.items()}
        for i, act in enumerate(acts):
            exact[i, at], bound[i, at] = _chunk_dots(w, t.typ, act, k, drop_last_block, wrong)
    return exact, bound


# ---- rope: the reference's own f32 cos / sin, from the oracle's rope_inplace on unit pairs ----
def rope_cs(pos, hd, rope_dim, neox):
    """(first elements [np], second elements [np], cos [np], sin [np]) of one head's pairs at `pos`; other elements are not rotated"""
    odev = o.OracleDevice(thread_num=1)
    x = np.zeros(hd, dtype=np.float32)
    if neox:
        ia = np.arange(rope_dim // 2)
        ib = ia + hd // 2
    else:
        ia = np.arange(0, rope_dim, 2)
        ib = ia + 1
    x[ia] = 1.0
    t = o.OracleTensor.new(x, [1, 1, hd], odev)
    t.rope_inplace(o.ROPE_NEOX if neox else o.ROPE_LLAMA, pos, rope_dim)
    out = t.export().reshape(hd)
    return ia, ib, out[ia].astype(np.float64), out[ib].astype(np.float64)


def f16_code_between(bits, lo, hi):
    """per element: the f16 value with code `bits` lies between f16(lo) and f16(hi) (rounding is monotone)"""
    v = f16v(np.asarray(bits, dtype=np.uint16))
    with np.errstate(over="ignore"):
        a, b = np.asarray(lo).astype(np.float16).astype(np.float64), np.asarray(hi).astype(np.float16).astype(np.float64)
    return (v >= a) & (v <= b)


# ---- the interval check ----
class QuantIntervals:
    """The reference's truncating quantizer (Q8_0: buf_q8_0.rs:87-134, Q8_1: buf_q8_1.rs:90-129) on a row known to an interval
    [lo, hi] per element (ref = the exact value).  Everything here comes from the reference alone; check() then looks at a device's blocks."""

    def __init__(self, lo, hi, ref, qt):
        self.qt = qt
        lo, hi, ref = (np.asarray(a, dtype=np.float64).reshape(-1, 32) for a in (lo, hi, ref))
        mag_hi = np.maximum(np.abs(lo), np.abs(hi))
        mag_lo = np.where((lo <= 0) & (hi >= 0), 0.0, np.minimum(np.abs(lo), np.abs(hi)))
        # dd = amax / 127 in f32: one rounding
        self.dd_lo = mag_lo.max(axis=1) / 127.0 * (1 - 2 * U)
        self.dd_hi = mag_hi.max(axis=1) / 127.0 * (1 + 2 * U)
        dlo, dhi = self.dd_lo[:, None], self.dd_hi[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.stack([lo / dlo, lo / dhi, hi / dlo, hi / dhi])
            c = np.where(np.isnan(c), 0.0, c)
            r_lo, r_hi = c.min(axis=0), c.max(axis=0)
            r_lo = r_lo - np.abs(r_lo) * 2 * U  # the f32 division
            r_hi = r_hi + np.abs(r_hi) * 2 * U
            r_lo, r_hi = np.clip(r_lo, -128, 127), np.clip(r_hi, -128, 127)  # (Q8_1 clamps; a Q8_0 ratio never leaves [-127, 127] by more than its rounding)
            self.q_lo, self.q_hi = np.trunc(r_lo), np.trunc(r_hi)
            dref = np.abs(ref).max(axis=1)[:, None] / 127.0
            self.q_ref = np.trunc(np.where(dref > 0, ref / np.where(dref > 0, dref, 1.0), 0.0))
        self.excused = self.q_lo != self.q_hi
        self.share = float(np.mean(self.excused))
        with np.errstate(over="ignore"):
            self.single_code = self.dd_lo.astype(np.float16) == self.dd_hi.astype(np.float16)

    def check(self, raw, res, name, ctx):
        res.excused[name] = self.share
        if self.share > EXCUSED_CAP:
            res.fails.append(f"{ctx} {res.launch}: {name}: excused share {self.share:.3f} > {EXCUSED_CAP} (from the reference alone)")
            return
        a = parse_act(raw, self.qt)
        okd = f16_code_between(a["d_bits"], self.dd_lo, self.dd_hi)
        if not okd.all():
            i = int(np.flatnonzero(~okd)[0])
            res.fails.append(f"{ctx} {res.launch}: {name} block {i}: scale {a['d'][i]:.6g} outside f16([{self.dd_lo[i]:.6g}, {self.dd_hi[i]:.6g}]) "
                             f"({int((~okd).sum())} blocks)")
        q = a["q"].astype(np.float64)
        okq = (q >= self.q_lo) & (q <= self.q_hi) & (np.abs(q - self.q_ref) <= 1)
        if not okq.all():
            bi, ei = np.argwhere(~okq)[0]
            res.fails.append(f"{ctx} {res.launch}: {name} row {int(bi) * 32 + int(ei)}: quant {int(q[bi, ei])} not in "
                             f"[{int(self.q_lo[bi, ei])}, {int(self.q_hi[bi, ei])}] (reference {int(self.q_ref[bi, ei])}; {int((~okq).sum())} elements)")
        if self.qt == o.Q8_1:
            lo, hi = self.s_interval(a)
            v = a["s"]
            oks = (v >= lo) & (v <= hi)
            if not oks.all():
                res.fails.append(f"{ctx} {res.launch}: {name} block {int(np.flatnonzero(~oks)[0])}: s is not f16(sum q * d) of the block's own quants and scale")

    def s_interval(self, a):
        """Q8_1: s = f16((float)sum q * dd) on the device's own quants (buf_q8_1.rs:121-127).  The kernel multiplies by the f32 dd, of
        which the block keeps f16(dd): dd lies in the reference's interval AND rounds to the device's own d code, i.e. within half an
        f16 step of it -- the intersection, times the exact integer sum, one f32 rounding, then the f16 codes of the two ends
        (a single code except where the product straddles a rounding boundary) -> (lo, hi) as f16 values"""
        d16 = np.ascontiguousarray(a["d_bits"]).view(np.float16)
        with np.errstate(over="ignore", invalid="ignore"):
            below = (np.nextafter(d16, np.float16(-np.inf)).astype(np.float64) + a["d"]) / 2
            above = (np.nextafter(d16, np.float16(np.inf)).astype(np.float64) + a["d"]) / 2
        dlo, dhi = np.maximum(self.dd_lo, below), np.minimum(self.dd_hi, above)
        sq = a["q"].sum(axis=1).astype(np.float64)
        e1, e2 = sq * dlo, sq * dhi
        e_lo, e_hi = np.minimum(e1, e2), np.maximum(e1, e2)
        e_lo, e_hi = e_lo - np.abs(e_lo) * U, e_hi + np.abs(e_hi) * U
        with np.errstate(over="ignore"):
            return e_lo.astype(np.float16).astype(np.float64), e_hi.astype(np.float16).astype(np.float64)


def _round_half_away(v):
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def q8k_reference(v):
    """the reference's Q8_K quantizer (buf_q8_k.rs:84-131) on exact values, in f64 -> (q [nsb, 256], class [nsb]: +1 where mx < 0
    (d > 0), -1 where mx > 0, 0 for an all-zero block)"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 256)
    j = np.argmax(np.abs(v), axis=1)  # the first element of maximal |v|
    mx = v[np.arange(v.shape[0]), j]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(mx[:, None] != 0, np.clip(_round_half_away(-128.0 / mx[:, None] * v), -128, 127), 0.0)
    return q, -np.sign(mx)


class QuantIntervalsK:
    """The reference's Q8_K quantizer on a row known to an interval [lo, hi] per element (ref = the exact value): see the module
    docstring.  Everything here comes from the reference alone; check() then looks at a device's blocks."""

    def __init__(self, lo, hi, ref):
        lo, hi, ref = (np.asarray(a, dtype=np.float64).reshape(-1, 256) for a in (lo, hi, ref))
        mag_hi = np.maximum(np.abs(lo), np.abs(hi))
        mag_lo = np.where((lo <= 0) & (hi >= 0), 0.0, np.minimum(np.abs(lo), np.abs(hi)))
        M = mag_lo.max(axis=1)
        adm = mag_hi >= M[:, None]  # the elements that can hold the maximum
        self.q_ref, self.cls_ref = q8k_reference(ref)
        self.cls = {}
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            for c, sel in ((1.0, adm & (lo < 0)), (-1.0, adm & (hi > 0))):  # c = sign of scale and of d: mx < 0 / mx > 0
                top = np.where(sel, mag_hi, 0.0).max(axis=1)
                s_lo, s_hi = 128.0 / top * (1 - U), np.where(M > 0, 128.0 / np.where(M > 0, M, 1.0) * (1 + U), np.inf)  # |scale|
                d_lo, d_hi = 1.0 / s_hi * (1 - U), 1.0 / s_lo * (1 + U)                                                   # |d|
                a, z = c * s_lo[:, None], c * s_hi[:, None]
                pr = np.stack([a * lo, a * hi, z * lo, z * hi])
                pr = np.where(np.isnan(pr), 0.0, pr)
                p_lo, p_hi = pr.min(axis=0), pr.max(axis=0)
                p_lo, p_hi = p_lo - np.abs(p_lo) * U, p_hi + np.abs(p_hi) * U  # the f32 product
                q_lo = np.clip(_round_half_away(np.clip(p_lo, -200, 200)), -128, 127)
                q_hi = np.clip(_round_half_away(np.clip(p_hi, -200, 200)), -128, 127)
                self.cls[c] = {"ok": sel.any(axis=1) & (top > 0), "d_lo": d_lo, "d_hi": d_hi, "q_lo": q_lo, "q_hi": q_hi}
        self.zero = mag_hi.max(axis=1) == 0  # an all-zero block: d = 0, q = 0
        # excused, from the reference alone: the quants whose interval holds a half-integer in the reference's own class; every quant
        # of a block whose maximum may sit on elements of either sign
        both = self.cls[1.0]["ok"] & self.cls[-1.0]["ok"]
        own = np.where((self.cls_ref > 0)[:, None], self.cls[1.0]["q_lo"] != self.cls[1.0]["q_hi"], self.cls[-1.0]["q_lo"] != self.cls[-1.0]["q_hi"])
        self.excused = (own | both[:, None]) & ~self.zero[:, None]
        self.share = float(np.mean(self.excused))

    def check(self, raw, qp, res, name, ctx):
        """raw: the device's blocks (292 bytes each), qp: its class-major plane (None: not tapped)"""
        res.excused[name] = self.share
        if self.share > EXCUSED_CAP:
            res.fails.append(f"{ctx} {res.launch}: {name}: excused share {self.share:.3f} > {EXCUSED_CAP} (from the reference alone)")
            return
        a = parse_act(raw, o.Q8_K)
        d, q = a["d"], a["q"].astype(np.float64)
        for i in range(d.size):
            where = f"{ctx} {res.launch}: {name} super-block {i}"
            if self.zero[i]:
                if d[i] != 0 or np.any(q[i] != 0):
                    res.fails.append(f"{where}: an all-zero block must have d = 0 and q = 0")
                continue
            k = self.cls.get(float(np.sign(d[i])))
            if k is None or not k["ok"][i]:
                res.fails.append(f"{where}: d = {d[i]:.8g} has the sign of no element that can hold the maximum")
                continue
            if not (k["d_lo"][i] <= abs(d[i]) <= k["d_hi"][i]):
                res.fails.append(f"{where}: |d| = {abs(d[i]):.9g} outside [{k['d_lo'][i]:.9g}, {k['d_hi'][i]:.9g}]")
            okq = (q[i] >= k["q_lo"][i]) & (q[i] <= k["q_hi"][i])
            if np.sign(d[i]) == self.cls_ref[i]:
                okq &= np.abs(q[i] - self.q_ref[i]) <= 1
            if not okq.all():
                e = int(np.flatnonzero(~okq)[0])
                res.fails.append(f"{where} element {e}: quant {int(q[i, e])} not in [{int(k['q_lo'][i, e])}, {int(k['q_hi'][i, e])}] "
                                 f"(reference {int(self.q_ref[i, e])}; {int((~okq).sum())} elements)")
        check_q8k_own(res, a, qp, name, ctx)


def check_q8k_own(res, a, qp, name, ctx):
    """bsums and the class-major plane are exact functions of the device's own q"""
    bs = a["q"].reshape(-1, 16, 16).sum(axis=2)
    if not np.array_equal(bs, a["bsums"]):
        i, g = np.argwhere(bs != a["bsums"])[0]
        res.fails.append(f"{ctx} {res.launch}: {name} super-block {int(i)}: bsums[{int(g)}] = {int(a['bsums'][i, g])}, its own quants add up to {int(bs[i, g])}")
    if qp is not None:
        got = np.ascontiguousarray(qp).view(np.int8).astype(np.int64).reshape(-1)
        want = class_major(a["q"].reshape(-1))
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            res.fails.append(f"{ctx} {res.launch}: {name}.qp byte {i} is not the class-major permutation of the q plane ({int((got != want).sum())} bytes)")


def check_quantizer_bytes(res, tap, name, f32_row, ctx):
    """planes whose f32 input is stored are the reference quantizer's bytes; a Q8_K set's qp the permutation of its q"""
    qt = tap["qtype"][name]
    exp = o.quantize(np.ascontiguousarray(f32_row, dtype=np.float32), qt)
    if not np.array_equal(exp, tap[name]):
        i = int(np.flatnonzero(exp != tap[name])[0])
        res.fails.append(f"{ctx} {res.launch}: {name.split('.', 1)[1]} differs from the reference quantizer of its f32 row at byte {i} "
                         f"(block {i // synth.BLOCK_BYTES[qt]})")
    if qt == o.Q8_K:
        check_q8k_own(res, parse_act(tap[name], qt), tap.get(name + ".qp"), name.split(".", 1)[1], ctx)


def check_f32(res, got, exact, bound, what, ctx):
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        res.fails.append(f"{ctx} {res.launch}: {what}: non-finite values")
        return
    res.ratio(np.abs(got - exact), bound, what, ctx)


def norm_interval(x, w, eps, n):
    """x / rms * w of the exact norm (norm_quant_block, nq_epilogue: sqrtf(sum / n + eps), (v / rms) * w) -> (lo, hi, ref)"""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    rms = math.sqrt(float(np.sum(x * x)) / n + float(np.float32(eps)))
    ref = x / rms * w
    r = (r_ss(n) / 2 + 1 + 2) * U
    return ref - np.abs(ref) * r, ref + np.abs(ref) * r, ref


def r_inv(n):
    """relative error factor (in U) of the argument of the deferred 1 / rms, from the chunk sums the launch read (module docstring)"""
    return math.ceil(n / 2048) + 8


def inv_rms_of_sums(rsums, eps, n):
    """1 / rms as RmsTail's consumers form it from the n / 32 chunk sums they read -- rsq(sum * inv_n + eps) with the f32 inv_n
    and eps of the kernel's expression -- in f64, and the relative error bound of the kernel's f32 value"""
    s = float(np.sum(np.asarray(rsums, dtype=np.float64)))
    inv_n = float(np.float32(1.0) / np.float32(n))
    return 1.0 / math.sqrt(s * inv_n + float(np.float32(eps))), (r_inv(n) / 2 + 2) * U


# ---- the launches ----
def _w(model, name):
    return model.tensors[name]


def _f32(model, name):
    return np.ascontiguousarray(model.tensors[name].data).view(np.float32)


def check_planes_in_front(tap, model, l, form, ctx):
    """what the q|k|v launch of layer 0 reads was made by the norm + quantize launch in front of it (k_norm_quant): exact-norm planes
    of the tapped x.  (For l > 0 the planes are the previous layer's ffn_down output: check_gemv_out of that layer.)"""
    res = Result("norm+quantize")
    s = model.shape
    lo, hi, ref = norm_interval(tap["qkv_in.x"], _f32(model, f"blk.{l}.attn_norm.weight"), s.rms_eps, s.dim)
    QuantIntervals(lo, hi, ref, tap["qtype"]["qkv_in.act_dim"]).check(tap["qkv_in.act_dim"], res, "act_dim", ctx)
    return res


def qkv_reference(tap, model, l, pos, form):
    """exact q (roped, scaled), k (roped), v rows of the layer and their bounds, from the planes the launch read"""
    s = model.shape
    hd, dim, kvd = s.head_dim, s.dim, s.kv_dim
    qwen2 = s.arch == "qwen2"
    act = tap_act(tap, "qkv_in.act_dim")
    out = {}
    deferred = form.defer and l > 0
    if deferred:
        inv, ri = inv_rms_of_sums(tap["qkv_in.rsums"], s.rms_eps, dim)
    rope_dim = s.rope_dim if s.rope_dim is not None else hd
    ia, ib, c, sn = rope_cs(pos, hd, rope_dim, qwen2)
    for nm, wname, rows in (("q", "attn_q", dim), ("k", "attn_k", kvd), ("v", "attn_v", kvd)):
        e, b = row_dots(_w(model, f"blk.{l}.{wname}.weight"), act)
        if deferred:  # s *= inv_rms (k_qkv<.., DEFER>): the bound scales, the factor's own error and one rounding are added
            b = b * inv * (1 + ri) + np.abs(e * inv) * (ri + U)
            e = e * inv
        if qwen2:  # the bias AFTER the deferred multiply (qkv_epilogue_neox), one f32 add
            e = e + _f32(model, f"blk.{l}.{wname}.bias").astype(np.float64)
            b = b + np.abs(e) * U
        if nm != "v":
            e, b = e.reshape(-1, hd).copy(), b.reshape(-1, hd).copy()
            a0, b0, ba, bb_ = e[:, ia].copy(), e[:, ib].copy(), b[:, ia].copy(), b[:, ib].copy()
            e[:, ia], e[:, ib] = a0 * c - b0 * sn, a0 * sn + b0 * c
            b[:, ia] = ba * np.abs(c) + bb_ * np.abs(sn) + 3 * U * (np.abs(a0 * c) + np.abs(b0 * sn))
            b[:, ib] = ba * np.abs(sn) + bb_ * np.abs(c) + 3 * U * (np.abs(a0 * sn) + np.abs(b0 * c))
            if nm == "q":
                scale = float(np.float32(1.0) / np.sqrt(np.float32(hd)))
                e = e * scale
                b = b * scale + np.abs(e) * U
        out[nm] = (e.reshape(-1), b.reshape(-1))
    return out


def cache_rows(kv_raw, form, n_kv, hd, pos):
    """the rows at `pos` of a K or V cache ([n_kv][seq_cap][hd], raw bytes): f16 bits or f32 values, [n_kv * hd]"""
    dt = np.uint16 if form.kv_f16 else np.float32
    return np.ascontiguousarray(kv_raw).view(dt).reshape(n_kv, form.seq_cap, hd)[:, pos, :].reshape(-1)


def check_qkv(tap, kc_raw, vc_raw, model, l, pos, form, ctx):
    res = Result("q|k|v")
    s = model.shape
    ref = qkv_reference(tap, model, l, pos, form)
    e, b = ref["q"]
    check_f32(res, tap["qkv.qbuf"], e, b + 1e-30, "q", ctx)
    for nm, raw in (("k", kc_raw), ("v", vc_raw)):
        e, b = ref[nm]
        got = cache_rows(raw, form, s.n_kv_heads, s.head_dim, pos)
        if form.kv_f16:  # an f16 cache element passes if its code lies between the f16 codes of the interval's two ends
            ok = f16_code_between(got, e - b, e + b)
            if not ok.all():
                i = int(np.flatnonzero(~ok)[0])
                res.fails.append(f"{ctx} {res.launch}: {nm} cache row {i}: f16 {f16v(got[i:i + 1])[0]:.6g} outside f16([{e[i] - b[i]:.6g}, {e[i] + b[i]:.6g}]) "
                                 f"({int((~ok).sum())} of {ok.size})")
        else:
            check_f32(res, got, e, b + 1e-30, nm, ctx)
    return res


def oracle_attention(q, kc_raw, vc_raw, n_heads, n_kv, hd, seq_cap, pos, kv_f16):
    """the reference's attention ops (llama2.rs:571-590, as OracleLlamaRunner.forward_multi_query_attention) on a given q and cache"""
    odev = o.OracleDevice(thread_num=1)
    kvt = o.F16 if kv_f16 else o.F32
    kc = o.OracleTensor.from_bytes(np.ascontiguousarray(kc_raw).view(np.uint8), kvt, [n_kv, seq_cap, hd], odev).resize(1, pos + 1)
    vc = o.OracleTensor.from_bytes(np.ascontiguousarray(vc_raw).view(np.uint8), kvt, [n_kv, seq_cap, hd], odev).resize(1, pos + 1)
    qt = o.OracleTensor.new(np.ascontiguousarray(q, dtype=np.float32).copy(), [n_heads, 1, hd], odev)
    attn = qt.batch_matmul(kc.transpose([0, 2, 1]))
    attn = attn.softmax_inplace(2)
    return attn.batch_matmul(vc).export().reshape(-1)


def f64_attention(q, kc_raw, vc_raw, n_heads, n_kv, hd, seq_cap, pos):
    q16 = np.asarray(q, dtype=np.float32).astype(np.float16).astype(np.float64).reshape(n_heads, hd)
    kf = np.ascontiguousarray(kc_raw).view(np.float16).astype(np.float64).reshape(n_kv, seq_cap, hd)[:, :pos + 1]
    vf = np.ascontiguousarray(vc_raw).view(np.float16).astype(np.float64).reshape(n_kv, seq_cap, hd)[:, :pos + 1]
    grp = n_heads // n_kv
    out = np.zeros((n_heads, hd))
    for h in range(n_heads):
        sc = kf[h // grp] @ q16[h]
        p = np.exp(sc - sc.max())
        out[h] = (p / p.sum()) @ vf[h // grp]
    return out.reshape(-1)


def check_attention(tap, kc_raw, vc_raw, model, l, pos, form, ctx):
    res = Result("attention")
    s = model.shape
    q, got = tap["qkv.qbuf"], tap["attn.attn"]
    if form.flash_from and pos + 1 >= form.flash_from:  # k_attn_flash: float64 softmax(q K^T) V on the same f16 inputs
        ref = f64_attention(q, kc_raw, vc_raw, s.n_heads, s.n_kv_heads, s.head_dim, form.seq_cap, pos)
        check_f32(res, got, ref, np.full(ref.shape, FLASH_REL * np.max(np.abs(ref))), "attn (flash)", ctx)
    else:  # the reference's arithmetic, bit for bit
        ref = oracle_attention(q, kc_raw, vc_raw, s.n_heads, s.n_kv_heads, s.head_dim, form.seq_cap, pos, form.kv_f16)
        same = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32) == ref.view(np.uint32)
        if not same.all():
            i = int(np.flatnonzero(~same)[0])
            res.fails.append(f"{ctx} {res.launch}: attn row {i}: {got[i]!r} != the reference's {ref[i]!r} ({int((~same).sum())} of {same.size} differ)")
    # act_attn is the reference quantizer applied to a buffer we hold (a K-quant step whose wo quantizes in its prologue stores none)
    if "attn.act_attn" in tap:
        check_quantizer_bytes(res, tap, "attn.act_attn", got, ctx)
    return res


def check_gemv_out(tap, model, l, which, form, ctx):
    """wo (which = "wo": rhs act_attn, x_in = the x the q|k|v launch saw) or ffn_down ("down": rhs act_hid, x_in = wo's x):
    x_out = x_in + W . rhs, then the planes and chunk sums for the consuming launch"""
    res = Result(which if which == "wo" else "ffn_down")
    s = model.shape
    L = s.n_layers
    if which == "wo":
        wname, rhs, x_in = f"blk.{l}.attn_output.weight", "attn.act_attn", tap["qkv_in.x"]
        wn, eps, deferred = _f32(model, f"blk.{l}.ffn_norm.weight"), 1e-5, form.defer  # eps: the literal 1e-5 (llama2.rs:611)
    else:
        wname, rhs, x_in = f"blk.{l}.ffn_down.weight", "gateup.act_hid", tap["wo.x"]
        wn = _f32(model, f"blk.{l + 1}.attn_norm.weight" if l + 1 < L else "output_norm.weight")
        eps, deferred = s.rms_eps, form.defer and l + 1 < L
    e, b = row_dots(_w(model, wname), parse_act(tap[rhs], tap["qtype"][rhs]))
    e = np.asarray(x_in, dtype=np.float64) + e
    x_out = tap[which + ".x"]
    check_f32(res, x_out, e, b + np.abs(e) * U + 1e-30, "x", ctx)  # x = matmul_out + x: one more rounding
    planes = which + ".act_dim"
    if planes not in tap:
        return res
    if deferred:
        # chunk sums of squares of the stored x_out (nq_epilogue DEFER): 32 squares and 31 adds, all positive
        x64 = np.asarray(x_out, dtype=np.float64).reshape(-1, 32)
        cs = (x64 * x64).sum(axis=1)
        check_f32(res, tap[which + ".rsums"], cs, cs * 33 * U + 1e-37, "rsums", ctx)
        # the kernel quantizes f32(x * w_norm) of the value it also stores (quant_lane32(hv * wn)): the reference quantizer's bytes
        exp = o.quantize(np.asarray(x_out, dtype=np.float32) * wn, o.Q8_0)
        if not np.array_equal(exp, tap[planes]):
            i = int(np.flatnonzero(exp != tap[planes])[0])
            res.fails.append(f"{ctx} {res.launch}: act_dim (hop-free) differs from the reference quantizer of f32(x * w_norm) at byte {i} (block {i // 34})")
    else:
        lo, hi, ref = norm_interval(x_out, wn, eps, s.dim)
        QuantIntervals(lo, hi, ref, tap["qtype"][planes]).check(tap[planes], res, "act_dim", ctx)
    return res


_EXP_TABLE = []


def exp_table():
    """the reference's f16 -> f16 exp table (cpu_device.rs:108-115), as values"""
    if not _EXP_TABLE:
        import ctypes

        t = np.empty(65536, dtype=np.uint16)
        o.lib().co_init_exp_cache(ctypes.c_void_p(t.ctypes.data))
        _EXP_TABLE.append(f16v(t))
    return _EXP_TABLE[0]


def silu_mul_interval(g, bg, u, bu, hull=True):
    """h = (g / (1 + table[f16(-g)])) * u (silu.rs:6-13, arithmetic.rs:57-66) for g in [g - bg, g + bg], u in [u - bu, u + bu]:
    the hull over every f16 code reachable from the interval of g -> (lo, hi, ref)"""
    tab = exp_table()

    def code(v):
        with np.errstate(over="ignore"):
            return np.asarray(v, dtype=np.float64).astype(np.float16)

    ref = g / (1.0 + tab[code(-g).view(np.uint16)]) * u
    g_lo, g_hi = g - bg, g + bg
    a, z = code(-g_hi), code(-g_lo)  # a <= z as f16 values
    if not hull:
        a = z = code(-g)
    # the table is monotone in its argument (expf is, and so is the rounding to f16): the hull over every code from a to z is spanned
    # by the two ends -- however many codes lie between (an interval of g that straddles 0 spans thousands of subnormal codes)
    e_lo, e_hi = tab[a.view(np.uint16)], tab[z.view(np.uint16)]
    assert np.all(e_lo <= e_hi)
    # s = g / (1 + e): corners (1 + e > 0), two roundings; then * u: corners, one rounding
    sc = np.stack([g_lo / (1 + e_lo), g_lo / (1 + e_hi), g_hi / (1 + e_lo), g_hi / (1 + e_hi)])
    s_lo, s_hi = sc.min(axis=0), sc.max(axis=0)
    s_lo, s_hi = s_lo - np.abs(s_lo) * 2 * U, s_hi + np.abs(s_hi) * 2 * U
    hc = np.stack([s_lo * (u - bu), s_lo * (u + bu), s_hi * (u - bu), s_hi * (u + bu)])
    h_lo, h_hi = hc.min(axis=0), hc.max(axis=0)
    return h_lo - np.abs(h_lo) * U, h_hi + np.abs(h_hi) * U, ref


def gateup_reference(tap, model, l, form, hull=True):
    s = model.shape
    act = parse_act(tap["wo.act_dim"], tap["qtype"]["wo.act_dim"])
    g, bg = row_dots(_w(model, f"blk.{l}.ffn_gate.weight"), act)
    u, bu = row_dots(_w(model, f"blk.{l}.ffn_up.weight"), act)
    if form.defer:
        inv, ri = inv_rms_of_sums(tap["wo.rsums"], 1e-5, s.dim)  # eps: the literal 1e-5 (llama2.rs:611)
        bg, bu = bg * inv * (1 + ri) + np.abs(g * inv) * (ri + U), bu * inv * (1 + ri) + np.abs(u * inv) * (ri + U)
        g, u = g * inv, u * inv
    return silu_mul_interval(g, bg, u, bu, hull)


def check_gateup(tap, model, l, form, ctx):
    res = Result("gate|up")
    lo, hi, ref = gateup_reference(tap, model, l, form)
    QuantIntervals(lo, hi, ref, tap["qtype"]["gateup.act_hid"]).check(tap["gateup.act_hid"], res, "act_hid", ctx)
    return res


def check_classifier(tap, model, ctx):
    res = Result("classifier")
    t = model.tensors["output.weight"] if "output.weight" in model.tensors else model.tensors["token_embd.weight"]
    e, b = row_dots(t, tap_act(tap, "cls.act"))
    check_f32(res, tap["logits"], e, b + 1e-30, "logits", ctx)
    return res


# ---- the launches of the K-quant step (enqueue_segment_k) ----
def _in_interval(res, got, lo, hi, what, ctx):
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    check_f32(res, got, mid, half + 1e-30, what, ctx)


def check_norm_launch(res, tap, model, x_name, xn_name, planes_name, wn, eps, ctx):
    """a stand-alone launch_norm_f32 + quantizer: xn inside the exact norm's interval of the tapped x, the planes the reference
    quantizer's bytes of the tapped xn"""
    lo, hi, _ = norm_interval(tap[x_name], wn, eps, model.shape.dim)
    _in_interval(res, tap[xn_name], lo, hi, xn_name, ctx)
    if planes_name in tap and tap["qtype"][planes_name] != o.F32:
        check_quantizer_bytes(res, tap, planes_name, tap[xn_name], ctx)


def _rhs(tap, planes_name, f32_name, qt):
    """the rhs of wo / ffn_down: the planes a launch stored, else (the consuming kernel quantizes its f32 row in the prologue) the
    reference quantizer of that row"""
    if planes_name in tap:
        return tap_act(tap, planes_name)
    return parse_act(o.quantize(np.ascontiguousarray(tap[f32_name], dtype=np.float32), qt), qt)


def check_gemv_out_k(tap, model, l, which, ctx):
    res = Result(which if which == "wo" else "ffn_down")
    s, plan = model.shape, tap["plan"]
    L = s.n_layers
    qt = o.rhs_dtype(model.wtype)
    if which == "wo":
        wname, rhs, x_in = f"blk.{l}.attn_output.weight", _rhs(tap, "attn.act_attn", "attn.attn", qt), tap["qkv_in.x"]
        wn, eps = _f32(model, f"blk.{l}.ffn_norm.weight"), 1e-5  # eps: the literal 1e-5 (llama2.rs:611)
    else:
        wname, rhs, x_in = f"blk.{l}.ffn_down.weight", _rhs(tap, "gateup.act_hid", "gateup.h", qt), tap["wo.x"]
        wn, eps = _f32(model, f"blk.{l + 1}.attn_norm.weight" if l + 1 < L else "output_norm.weight"), s.rms_eps
    e, b = row_dots(_w(model, wname), rhs)
    e = np.asarray(x_in, dtype=np.float64) + e
    x_out = tap[which + ".x"]
    check_f32(res, x_out, e, b + np.abs(e) * U + 1e-30, "x", ctx)  # x = matmul_out + x: one more rounding
    if which == "wo" and plan["wo_x_only"]:  # the chunk sums the NORMIN launch reads: split_wo per chunk, each over its own rows
        parts = plan["split_wo"]
        x64 = np.asarray(x_out, dtype=np.float64).reshape(-1, 32 // parts)
        cs = (x64 * x64).sum(axis=1)
        if "wo.rsums" not in tap or tap["wo.rsums"].size != cs.size:
            res.fails.append(f"{ctx} {res.launch}: {parts} chunk sums per 32 rows expected, the tap holds {tap['wo.rsums'].size if 'wo.rsums' in tap else 0}")
        else:
            check_f32(res, tap["wo.rsums"], cs, cs * 33 * U + 1e-37, "rsums", ctx)
    elif plan["norm_epi_k"]:
        lo, hi, ref = norm_interval(x_out, wn, eps, s.dim)
        QuantIntervalsK(lo, hi, ref).check(tap[which + ".act_dim"], tap.get(which + ".act_dim.qp"), res, "act_dim", ctx)
    elif which == "wo":
        check_norm_launch(res, tap, model, "wo.x", "wo.xn", "wo.act_dim", wn, eps, ctx)
    elif l + 1 == L:  # the final norm launch reads this x (layers in between: the next layer's tap holds its own x and xn)
        check_norm_launch(res, tap, model, "down.x", "cls.xn", "cls.act", wn, eps, ctx)
    return res


def check_gateup_k(tap, model, l, ctx, twin=None):
    """h = act(g) * u from the planes the launch read -- in the NORMIN form the planes a NO_K_NORM_IN twin's wo left (bit-equal x) --,
    then h's planes where a launch stored them"""
    res = Result("gate|up")
    src = tap
    if tap["plan"]["wo_x_only"]:
        if twin is None or "wo.act_dim" not in twin:
            res.fails.append(f"{ctx} {res.launch}: the NORMIN form needs the tap of a NO_K_NORM_IN twin")
            return res
        if not np.array_equal(np.ascontiguousarray(twin["wo.x"]).view(np.uint32), np.ascontiguousarray(tap["wo.x"]).view(np.uint32)):
            res.fails.append(f"{ctx} {res.launch}: wo.x of the NO_K_NORM_IN twin differs from this step's")
            return res
        src = twin
        lo, hi, ref = norm_interval(twin["wo.x"], _f32(model, f"blk.{l}.ffn_norm.weight"), 1e-5, model.shape.dim)
        QuantIntervalsK(lo, hi, ref).check(twin["wo.act_dim"], twin.get("wo.act_dim.qp"), res, "twin act_dim", ctx)
    act = tap_act(src, "wo.act_dim")
    g, bg = row_dots(_w(model, f"blk.{l}.ffn_gate.weight"), act)
    u, bu = row_dots(_w(model, f"blk.{l}.ffn_up.weight"), act)
    if model.shape.arch == "gemma":
        from tests import gemma_step_ref as G
        lo, hi, _ = G.gelu_mul_interval(g, bg, u, bu)
    else:
        lo, hi, _ = silu_mul_interval(g, bg, u, bu)
    _in_interval(res, tap["gateup.h"], lo, hi, "h", ctx)
    if "gateup.act_hid" in tap:
        check_quantizer_bytes(res, tap, "gateup.act_hid", tap["gateup.h"], ctx)
    return res


def check_layer_k(tap, kc_raw, vc_raw, model, l, pos, form, ctx, twin=None, token=None):
    """every launch of the tapped layer of a K-quant step, in the form the tapped plan words name"""
    s, plan, out = model.shape, tap["plan"], {}
    if "qkv_in.xn" in tap:
        res = out["norm+quantize"] = Result("norm+quantize")
        check_norm_launch(res, tap, model, "qkv_in.x", "qkv_in.xn", "qkv_in.act_dim", _f32(model, f"blk.{l}.attn_norm.weight"), s.rms_eps, ctx)
    if s.arch == "gemma":
        from tests import gemma_step_ref as G
        if l == 0 and token is not None:
            out["embed"] = G.check_embed(tap, model, token, ctx)
        out["q|k|v"] = G.check_qkv(tap, kc_raw, vc_raw, model, l, pos, form, ctx)
    else:
        out["q|k|v"] = check_qkv(tap, kc_raw, vc_raw, model, l, pos, form, ctx)
    out["attention"] = check_attention(tap, kc_raw, vc_raw, model, l, pos, form, ctx)
    if ("attn.act_attn" in tap) != (plan["aq8"] == 1 or plan["qin"] == 0):
        out["attention"].fails.append(f"{ctx} attention: act_attn planes {'stored' if 'attn.act_attn' in tap else 'missing'} against the plan {plan}")
    out["wo"] = check_gemv_out_k(tap, model, l, "wo", ctx)
    out["gate|up"] = check_gateup_k(tap, model, l, ctx, twin)
    out["ffn_down"] = check_gemv_out_k(tap, model, l, "down", ctx)
    out["classifier"] = check_classifier(tap, model, ctx)
    return out


def check_layer(tap, kc_raw, vc_raw, model, l, pos, form, ctx, twin=None, token=None):
    """every launch of the tapped layer (and the classifier) -> {launch: Result}; the step's body from the tapped plan words"""
    if tap.get("plan", {}).get("path") == 2:
        return check_layer_k(tap, kc_raw, vc_raw, model, l, pos, form, ctx, twin, token)
    out = {}
    if l == 0:
        out["norm+quantize"] = check_planes_in_front(tap, model, l, form, ctx)
    out["q|k|v"] = check_qkv(tap, kc_raw, vc_raw, model, l, pos, form, ctx)
    out["attention"] = check_attention(tap, kc_raw, vc_raw, model, l, pos, form, ctx)
    if "attn.act_attn" not in tap:  # (the five launches always store wo's rhs)
        out["attention"].fails.append(f"{ctx} attention: the tap holds no act_attn planes")
    out["wo"] = check_gemv_out(tap, model, l, "wo", form, ctx)
    out["gate|up"] = check_gateup(tap, model, l, form, ctx)
    out["ffn_down"] = check_gemv_out(tap, model, l, "down", form, ctx)
    out["classifier"] = check_classifier(tap, model, ctx)
    return out


def failures(results):
    return [f for r in results.values() for f in r.fails]
