"""The launches of the fast fused decode step of a GEMMA context (crabml_hip_llama_create_arch with CRABML_HIP_ARCH_GEMMA) restated in
float64, for the tap recorder -- tests/fused_step_ref.py's pieces (row_dots, QuantIntervals with its EXCUSED_CAP, f64_attention and
FLASH_REL, the wo / ffn_down / classifier / attention checks, which do not depend on the architecture) plus what forward_gemma
(llama2.rs:455-524) changes in a launch:

  embedding   x = f32(dequantized row) * sqrtf((float)dim): one f32 multiply per element, a rounding of its own after the
              dequantization (llama2.rs:468) -- restated exactly, compared bit for bit (layer 0's tap holds that x).
  q|k|v       NEOX pairs (i, i + hd / 2) like Qwen2's, and NO bias (k_qkv's QKV_GEMMA form).
  gate|up     h = f32(table[f16(g)]) * u with the reference's f16 GELU table (gelu.rs:10-22).  Given g this is the reference's own
              lookup; g is known to an interval, so h is known to the hull of the table over every f16 code reachable from it.  The
              GELU table is NOT monotone (it dips near -0.75), and an interval of g that straddles 0 spans thousands of subnormal
              codes: the hull is the min / max of the table over the whole code range (a range reduction over the table in value
              order), never its two ends."""
import ctypes

import numpy as np

from oracle import oracle as o
from tests import fused_step_ref as R
from tests.fused_step_ref import U, Result, _w, check_f32, f16_code_between, f16v

_TAB = {}


def gelu_table():
    """the reference's f16 -> f16 GELU table (cpu_device.rs:117-124), as f64 values indexed by the f16 code"""
    if "t" not in _TAB:
        t = np.empty(65536, dtype=np.uint16)
        o.lib().co_init_gelu_cache(ctypes.c_void_p(t.ctypes.data))
        _TAB["t"] = f16v(t)
    return _TAB["t"]


def value_order(codes):
    """f16 codes -> their rank in VALUE order: negative codes descend (-0 = 0x7fff), positive ones ascend (+0 = 0x8000); rounding to
    f16 is monotone, so the codes reachable from an interval of reals are the ranks between those of its two ends"""
    c = np.asarray(codes, dtype=np.uint16).astype(np.int64)
    return np.where(c < 0x8000, c + 0x8000, 0xFFFF - c)


def gelu_by_value():
    """the table in value order of its argument, one spare element behind (ranges are taken with reduceat: [lo, hi + 1))"""
    if "v" not in _TAB:
        t = gelu_table()
        by = np.empty(65537)
        by[value_order(np.arange(65536, dtype=np.uint16))] = t
        by[65536] = by[65535]
        _TAB["v"] = by
    return _TAB["v"]


def table_hull(g_lo, g_hi):
    """(min, max) of the GELU table over every f16 code reachable from [g_lo, g_hi], per element"""
    with np.errstate(over="ignore"):
        a = value_order(np.asarray(g_lo, dtype=np.float64).astype(np.float16).view(np.uint16))
        z = value_order(np.asarray(g_hi, dtype=np.float64).astype(np.float16).view(np.uint16))
    assert np.all(a <= z)
    by = gelu_by_value()
    idx = np.stack([a, z + 1], axis=1).reshape(-1)
    lo, hi = np.minimum.reduceat(by, idx)[::2], np.maximum.reduceat(by, idx)[::2]
    assert np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)), "an interval of g reaches a non-finite f16 code"
    return lo, hi


def gelu_mul_interval(g, bg, u, bu, hull=True):
    """h = f32(table[f16(g)]) * u (gelu.rs:11-17, arithmetic.rs:57-66) for g in [g - bg, g + bg], u in [u - bu, u + bu] -> (lo, hi, ref).
    The lookup is exact (an f16 value); the product is one f32 rounding."""
    g, u = np.asarray(g, dtype=np.float64), np.asarray(u, dtype=np.float64)
    tab = gelu_table()
    with np.errstate(over="ignore"):
        ref = tab[g.astype(np.float16).view(np.uint16)] * u
    t_lo, t_hi = table_hull(g - bg, g + bg) if hull else table_hull(g, g)
    hc = np.stack([t_lo * (u - bu), t_lo * (u + bu), t_hi * (u - bu), t_hi * (u + bu)])
    h_lo, h_hi = hc.min(axis=0), hc.max(axis=0)
    return h_lo - np.abs(h_lo) * U, h_hi + np.abs(h_hi) * U, ref


# ---- the launches ----
def embed_reference(model, token):
    """the scaled embedding row, exactly: f32(dequantize(row)) * f32(sqrt(dim)), each product rounded once to f32"""
    s = model.shape
    emb = model.tensors["token_embd.weight"]
    row = o.dequantize(emb.data, emb.typ, token * s.dim, s.dim).astype(np.float32)
    return row * np.sqrt(np.float32(s.dim))


def check_embed(tap, model, token, ctx):
    """layer 0's tap: the x the first q|k|v launch saw is the scaled embedding row, bit for bit"""
    res = Result("embed")
    want = embed_reference(model, token)
    got = np.ascontiguousarray(tap["qkv_in.x"], dtype=np.float32)
    same = got.view(np.uint32) == want.view(np.uint32)
    if not same.all():
        i = int(np.flatnonzero(~same)[0])
        res.fails.append(f"{ctx} {res.launch}: x[{i}] = {got[i]!r}, the scaled embedding is {want[i]!r} ({int((~same).sum())} of {same.size} differ)")
    return res


def qkv_reference(tap, model, l, pos, form):
    """exact q (NEOX-roped, scaled), k (roped), v rows of the layer and their bounds, from the planes the launch read: fused_step_ref's
    qkv_reference with NEOX pairs and without a bias"""
    s = model.shape
    hd, dim, kvd = s.head_dim, s.dim, s.kv_dim
    act = R.tap_act(tap, "qkv_in.act_dim")
    out = {}
    deferred = form.defer and l > 0
    if deferred:
        inv, ri = R.inv_rms_of_sums(tap["qkv_in.rsums"], s.rms_eps, dim)
    rope_dim = s.rope_dim if s.rope_dim is not None else hd
    ia, ib, c, sn = R.rope_cs(pos, hd, rope_dim, True)
    for nm, wname in (("q", "attn_q"), ("k", "attn_k"), ("v", "attn_v")):
        e, b = R.row_dots(_w(model, f"blk.{l}.{wname}.weight"), act)
        if deferred:
            b = b * inv * (1 + ri) + np.abs(e * inv) * (ri + U)
            e = e * inv
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


def check_qkv(tap, kc_raw, vc_raw, model, l, pos, form, ctx):
    res = Result("q|k|v")
    s = model.shape
    ref = qkv_reference(tap, model, l, pos, form)
    e, b = ref["q"]
    check_f32(res, tap["qkv.qbuf"], e, b + 1e-30, "q", ctx)
    for nm, raw in (("k", kc_raw), ("v", vc_raw)):
        e, b = ref[nm]
        got = R.cache_rows(raw, form, s.n_kv_heads, s.head_dim, pos)
        if form.kv_f16:
            ok = f16_code_between(got, e - b, e + b)
            if not ok.all():
                i = int(np.flatnonzero(~ok)[0])
                res.fails.append(f"{ctx} {res.launch}: {nm} cache row {i}: f16 {f16v(got[i:i + 1])[0]:.6g} outside f16([{e[i] - b[i]:.6g}, {e[i] + b[i]:.6g}]) "
                                 f"({int((~ok).sum())} of {ok.size})")
        else:
            check_f32(res, got, e, b + 1e-30, nm, ctx)
    return res


def gateup_reference(tap, model, l, form, hull=True):
    s = model.shape
    act = R.parse_act(tap["wo.act_dim"], tap["qtype"]["wo.act_dim"])
    g, bg = R.row_dots(_w(model, f"blk.{l}.ffn_gate.weight"), act)
    u, bu = R.row_dots(_w(model, f"blk.{l}.ffn_up.weight"), act)
    if form.defer:
        inv, ri = R.inv_rms_of_sums(tap["wo.rsums"], 1e-5, s.dim)  # eps: the literal 1e-5 (llama2.rs:611)
        bg, bu = bg * inv * (1 + ri) + np.abs(g * inv) * (ri + U), bu * inv * (1 + ri) + np.abs(u * inv) * (ri + U)
        g, u = g * inv, u * inv
    return gelu_mul_interval(g, bg, u, bu, hull)


def check_gateup(tap, model, l, form, ctx):
    res = Result("gate|up")
    lo, hi, ref = gateup_reference(tap, model, l, form)
    R.QuantIntervals(lo, hi, ref, tap["qtype"]["gateup.act_hid"]).check(tap["gateup.act_hid"], res, "act_hid", ctx)
    return res


def check_layer(tap, kc_raw, vc_raw, model, l, pos, form, ctx, token=None):
    """every launch of the tapped layer (and the classifier) of a Gemma step -> {launch: Result}; token: the step's token id (layer 0:
    the scaled embedding is checked too)"""
    assert model.shape.arch == "gemma"
    out = {}
    if l == 0:
        if token is not None:
            out["embed"] = check_embed(tap, model, token, ctx)
        out["norm+quantize"] = R.check_planes_in_front(tap, model, l, form, ctx)
    out["q|k|v"] = check_qkv(tap, kc_raw, vc_raw, model, l, pos, form, ctx)
    out["attention"] = R.check_attention(tap, kc_raw, vc_raw, model, l, pos, form, ctx)
    if "attn.act_attn" not in tap:  # (the five launches always store wo's rhs)
        out["attention"].fails.append(f"{ctx} attention: the tap holds no act_attn planes")
    out["wo"] = R.check_gemv_out(tap, model, l, "wo", form, ctx)
    out["gate|up"] = check_gateup(tap, model, l, form, ctx)
    out["ffn_down"] = R.check_gemv_out(tap, model, l, "down", form, ctx)
    out["classifier"] = R.check_classifier(tap, model, ctx)
    return out


failures = R.failures
