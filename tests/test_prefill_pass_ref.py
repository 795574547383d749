"""The checker of the fast prompt pass (tests/prefill_pass_ref.py) decides what tests/test_hip_prefill_launches.py can see, so it is
tested first, without a device.

A pass tap is built from the ORACLE: the token loop walked launch by launch, all rows of the pass through one layer before the next,
with the reference's own ops (its quantizer, its scalar vec_dot per row, its rope / attention / SiLU) -- and, in the f16-GEMM form, the
GEMM outputs taken as the f32 sum of the restated A' B' in one admissible order (numpy's f32 matrix product; a wo / ffn_down GEMM cut
into two k pieces, the second left to the norm launch).  The checker must ACCEPT every such tap with every excused share under the cap,
then REJECT every single mutation of MUTATIONS (a pass that is subtly wrong in exactly that way), on every model."""
import copy

import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests import prefill_pass_ref as P
from tests import q5k_step_ref as Q5
from tests.helpers import to_oracle
from tests.qwen2_ref import OracleQwen2Runner, to_oracle_qwen2
from tests.test_fused_step_ref import TOKS, exact_norm, mv, rope, silu_mul
from tests.test_hip_f16w_gemm import weight_operands

SEQ = 24
PASS_TOKS = [3, 77, 500, 31, 8, 19, 64, 128, 5, 900, 12]
FMT = {synth.Q4_0: "Q4_0", synth.Q8_0: "Q8_0", synth.Q4_1: "Q4_1"}


def f32w(model, n):
    return np.ascontiguousarray(model.tensors[n].data).view(np.float32)


def xh_of(planes_rows, qt):
    return P.b_prime([R.parse_act(p, qt) for p in planes_rows])[0].reshape(-1)


def kernel_for(t, f16w):
    """the kernel a matrix takes in a pass that allows the f16 GEMM or not: a Q5_K matrix has no matrix-core GEMM at all"""
    if t.typ == synth.Q5_K:
        return P.KERNEL_GEMV
    return P.KERNEL_F16W if f16w else P.KERNEL_INT8


def gemm_pieces(t, planes_rows, qt, f16w, pieces, kern=None):
    """W . rows as `pieces` k pieces of f32 [B, m] (their sum in piece order is the GEMM's output); kern: the kernel this matrix takes
    (default: kernel_for)"""
    m, k = t.shape
    if (kernel_for(t, f16w) if kern is None else kern) != P.KERNEL_F16W:
        return [np.stack([mv(t, p) for p in planes_rows])]
    ap = weight_operands(np.ascontiguousarray(t.data).view(np.uint8).reshape(-1), P.F16W_FMT[t.typ], list(range(m)), k)[0].astype(np.float32)
    bp = P.b_prime([R.parse_act(p, qt) for p in planes_rows])[1].astype(np.float32)
    half = (k // 512) * 256 if qt == o.Q8_K else (k // 64) * 32  # (whole blocks / super-blocks on either side of the cut)
    cut = [0, k] if pieces == 1 else [0, half, k]
    return [bp[:, a:b] @ ap[:, a:b].T for a, b in zip(cut[:-1], cut[1:])]


def oracle_pass(model, pos0, n, layer, kv_f16, f16w, h_done, fused=True, kernel_of=None, toks=None, seq=SEQ):
    """(tap, kv_before, kv_after, form, aux) of one pass of n rows at pos0 with `layer` tapped, from the oracle's ops.  fused: residual
    add + norm + quantize as one launch per row (the pending ffn_down output and the k pieces of a cut GEMM are left to it); not fused:
    the separate launches -- k_res_epi right behind wo and ffn_down, nothing pending, no pieces left over.  Q8_K rows (K-quant
    layers): the f32 norms, h and the class-major planes are stored as the device's tap stores them.  kernel_of(matrix name, tensor,
    layer) -> KERNEL_*: the kernel each matrix takes, one by one (default: kernel_for, the same answer for every matrix of a format).
    toks / seq: the pass's own tokens and cache length (default: PASS_TOKS[:n], SEQ).  aux["h_absmax"]: max |silu(g) * u| per layer"""
    s = model.shape
    odev = o.OracleDevice(thread_num=1)
    qwen2 = s.arch == "qwen2"
    conf, w = (to_oracle_qwen2 if qwen2 else to_oracle)(model, odev)
    runner = (OracleQwen2Runner if qwen2 else o.OracleLlamaRunner)(conf, w, odev, seq, kv_f16)
    for i in range(pos0):
        runner.forward_llama([TOKS[i]], i)
    kdt = np.uint16 if kv_f16 else np.float32
    kcs = [np.array(c.storage, dtype=kdt).reshape(s.n_kv_heads, seq, s.head_dim) for c in runner.key_cache]
    vcs = [np.array(c.storage, dtype=kdt).reshape(s.n_kv_heads, seq, s.head_dim) for c in runner.value_cache]
    qt = o.rhs_dtype(model.wtype)
    dim, hd, L = s.dim, s.head_dim, s.n_layers
    rope_dim = s.rope_dim if s.rope_dim is not None else hd
    toks = PASS_TOKS[:n] if toks is None else [int(t) for t in toks]
    assert len(toks) == n and pos0 + n <= seq
    emb = model.tensors["token_embd.weight"]
    x = np.stack([o.dequantize(emb.data, emb.typ, t * dim, dim) for t in toks])
    kq = qt == o.Q8_K
    assert fused or kq
    plan = {"n_cu": 256, "rows": n, "pos0": pos0, "f16w": int(f16w), "recomputed": 0,
            "norm_kernel": (4 if fused else 0) if kq else (2 if f16w else 1), "in_parts": 0,
            "qkv_one": 0, "gu_one": 0, "h_done": h_done, "wo_parts": 0, "down_parts": 0, "attn_kernel": P.ATTN_TILE}
    tap, aux = {"qtype": {}, "plan": plan}, {"odev": odev}
    form = P.Form(kv_f16=kv_f16, seq_cap=seq)

    def put(name, v, t=None):
        tap[name] = np.ascontiguousarray(v).reshape(-1)
        tap["qtype"][name] = o.F32 if t is None else t

    def put_planes(name, planes_rows):
        put(name, np.concatenate(planes_rows), qt)
        if kq:
            put(name + ".qp", np.concatenate([R.class_major(R.parse_act(p, qt)["q"].reshape(-1)).astype(np.int8).view(np.uint8) for p in planes_rows]), qt)

    def quant_rows(v):
        return [o.quantize(np.ascontiguousarray(r, dtype=np.float32), qt) for r in v]

    def norm_rows(v, wn, eps):
        xn = np.stack([exact_norm(r, wn, eps, odev) for r in v])
        return quant_rows(xn), xn

    pending = None  # [piece 0, piece 1, ...] of the previous layer's ffn_down
    for l in range(L):
        rec = l == layer
        if rec:
            put("in.x", x)
            if pending:
                put("in.tmp", pending[0])
                if len(pending) > 1:
                    put("in.parts", np.stack(pending[1:]))
                    plan["in_parts"] = len(pending) - 1
        x0 = x
        if pending:
            acc = pending[0]
            for p in pending[1:]:
                acc = acc + p
            x = acc + x
        wn1 = f32w(model, f"blk.{l}.attn_norm.weight")
        planes, xn1 = norm_rows(x, wn1, s.rms_eps)
        W = {nm: model.tensors[f"blk.{l}.{nm}.weight"] for nm in P.KERNEL_WORD}
        kern = {nm: (kernel_of(nm, t, l) if kernel_of else kernel_for(t, f16w)) for nm, t in W.items()}
        f16 = {nm: k_ == P.KERNEL_F16W for nm, k_ in kern.items()}
        lin = {}
        for nm, wn_ in (("q", "attn_q"), ("k", "attn_k"), ("v", "attn_v")):
            lin[nm] = gemm_pieces(model.tensors[f"blk.{l}.{wn_}.weight"], planes, qt, f16w, 1, kern[wn_])[0]
        withb = {nm: (v + f32w(model, f"blk.{l}.attn_{nm}.bias")[None, :] if qwen2 else v) for nm, v in lin.items()}
        scale = np.float32(1.0) / np.sqrt(np.float32(hd))
        qr = np.stack([rope(withb["q"][r], s.n_heads, hd, pos0 + r, rope_dim, qwen2, odev) * scale for r in range(n)])
        kr = np.stack([rope(withb["k"][r], s.n_kv_heads, hd, pos0 + r, rope_dim, qwen2, odev) for r in range(n)])
        kv_before = (kcs[l].copy(), vcs[l].copy())
        for cache, rows_ in ((kcs[l], kr), (vcs[l], withb["v"])):
            for r in range(n):
                cache[:, pos0 + r, :] = (o.f32_to_f16_bits(rows_[r]) if kv_f16 else rows_[r]).reshape(s.n_kv_heads, hd)
        attn = np.stack([R.oracle_attention(qr[r], kcs[l], vcs[l], s.n_heads, s.n_kv_heads, hd, seq, pos0 + r, kv_f16) for r in range(n)])
        act_attn = quant_rows(attn)
        wo = gemm_pieces(model.tensors[f"blk.{l}.attn_output.weight"], act_attn, qt, f16w, 2 if fused else 1, kern["attn_output"])
        acc = wo[0]
        for p in wo[1:]:
            acc = acc + p
        x1 = acc + x
        planes1, xn2 = norm_rows(x1, f32w(model, f"blk.{l}.ffn_norm.weight"), 1e-5)
        g = gemm_pieces(model.tensors[f"blk.{l}.ffn_gate.weight"], planes1, qt, f16w, 1, kern["ffn_gate"])[0]
        u = gemm_pieces(model.tensors[f"blk.{l}.ffn_up.weight"], planes1, qt, f16w, 1, kern["ffn_up"])[0]
        h = np.stack([silu_mul(g[r], u[r], odev) for r in range(n)])
        aux.setdefault("h_absmax", []).append(float(np.max(np.abs(h))))
        act_hid = quant_rows(h)
        last = l + 1 == L
        deferred = fused and not last
        down = gemm_pieces(model.tensors[f"blk.{l}.ffn_down.weight"], act_hid, qt, f16w, 2 if deferred else 1, kern["ffn_down"])
        if rec:
            put("n1.x", x)
            put_planes("n1.act", planes)
            put("q", lin["q"]), put("k", lin["k"]), put("v", lin["v"])
            put("qr", qr)
            put("attn", attn)
            put_planes("attn.act", act_attn)
            put("wo.tmp", wo[0])
            if len(wo) > 1:
                put("wo.parts", np.stack(wo[1:]))
                plan["wo_parts"] = len(wo) - 1
            put("n2.x", x1)
            put_planes("n2.act", planes1)
            if h_done == 0:
                put("g", g), put("u", u)
            elif h_done == 1:
                put("g", h)
            if kq:
                put("n1.xn", xn1), put("n2.xn", xn2)
                if h_done == 0:
                    put("hid.h", h)
            put_planes("hid.act", act_hid)
            put("down.tmp", down[0])
            if len(down) > 1:
                put("down.parts", np.stack(down[1:]))
                plan["down_parts"] = len(down) - 1
            # B' as each f16 GEMM finds it; v's own where neither q nor k left one in v's order (a Q6_K attn_v behind a Q4_K / Q5_K attn_q;
            # behind a q the range check refused, k's GEMM makes it -- untapped -- and v finds it)
            if f16["attn_q"]:
                put("n1.xh", xh_of(planes, qt), o.F16)
            if f16["attn_v"] and not any(f16[nm] and W["attn_v"].typ == W[nm].typ for nm in ("attn_q", "attn_k")):
                put("n1.xh.v", xh_of(planes, qt), o.F16)
            if f16["attn_output"]:
                put("attn.xh", xh_of(act_attn, qt), o.F16)
            if f16["ffn_gate"]:
                put("n2.xh", xh_of(planes1, qt), o.F16)
            if f16["ffn_down"]:
                put("hid.xh", xh_of(act_hid, qt), o.F16)
            plan["qkv_one"] = int(all(f16[nm] and W[nm].typ == W["attn_q"].typ for nm in ("attn_q", "attn_k", "attn_v")))
            plan["gu_one"] = int(f16["ffn_gate"] and f16["ffn_up"] and W["ffn_up"].typ == W["ffn_gate"].typ)
            for nm, word in P.KERNEL_WORD.items():
                plan[word] = kern[nm]
            if not deferred:
                put("down.x", down[0] + x1)
            aux.update(x0=x0, pending=pending, lin=lin, withb=withb, g=g, u=u, h=h, x1=x1, wn1=wn1, kv_before=kv_before, kv_after=(kcs[l], vcs[l]),
                       planes=planes, xn1=xn1, xn2=xn2, x_n1=x)
        if not deferred:
            x = down[0] + x1
            pending = None
        else:
            x, pending = x1, down
    put("last.x", x[-1])
    cls_xn = exact_norm(x[-1], f32w(model, "output_norm.weight"), s.rms_eps, odev)
    cls = o.quantize(cls_xn, qt)
    if kq:
        put("cls.xn", cls_xn)
        put_planes("cls.act", [cls])
    else:
        put("cls.act", cls, qt)
    put("logits", mv(model.tensors["output.weight"], cls))
    aux["x_final"] = x
    return tap, aux["kv_before"], aux["kv_after"], form, aux


class Case:
    def __init__(self, model, layer, tap, kvb, kva, form, aux, small):
        self.model, self.layer, self.tap, self.kvb, self.kva, self.form, self.aux, self.small = model, layer, tap, kvb, kva, form, aux, small
        self.twin = None
        if tap["plan"]["h_done"] == 2:  # the SEPARATE_F16_ROWS twin stores h
            self.twin = dict(tap)
            self.twin["plan"] = dict(tap["plan"], h_done=1)
            self.twin["g"] = aux["h"].reshape(-1)
            self.twin["qtype"] = dict(tap["qtype"], g=o.F32)

    def fork(self):
        c = copy.copy(self)
        c.tap = dict(self.tap)
        c.kva = (self.kva[0].copy(), self.kva[1].copy())
        c.twin = dict(self.twin) if self.twin else None
        return c

    @property
    def n(self):
        return self.tap["plan"]["rows"]

    @property
    def pos0(self):
        return self.tap["plan"]["pos0"]


def _rope_row(c, nm, r, pos, bias=True):
    s = c.model.shape
    rope_dim = s.rope_dim if s.rope_dim is not None else s.head_dim
    src = (c.aux["withb"] if bias else c.aux["lin"])[nm][r]
    heads = s.n_heads if nm == "q" else s.n_kv_heads
    v = rope(src, heads, s.head_dim, pos, rope_dim, s.arch == "qwen2", c.aux["odev"])
    return v * (np.float32(1.0) / np.sqrt(np.float32(s.head_dim))) if nm == "q" else v


def _set_cache_row(c, which, pos, row):
    s = c.model.shape
    c.kva[which][:, pos, :] = (o.f32_to_f16_bits(row) if c.form.kv_f16 else row).reshape(s.n_kv_heads, s.head_dim)


# ---- the mutations: each changes its copy of the case and returns the launch that must now fail, or None where it does not apply ----
def m_rope_last_row_next_pos(c):
    q = P.rows_of(c.tap, "qr", c.model.shape.dim).copy()
    q[-1] = _rope_row(c, "q", c.n - 1, c.pos0 + c.n)
    c.tap["qr"] = q.reshape(-1)
    return "k_qkv_epi_rows"


def m_rope_ignores_pos0(c):
    if c.pos0 == 0:
        return None
    q = np.stack([_rope_row(c, "q", r, r) for r in range(c.n)])
    c.tap["qr"] = q.reshape(-1)
    return "k_qkv_epi_rows"


def m_k_rope_ignores_pos0(c):
    if c.pos0 == 0:
        return None
    for r in range(c.n):
        _set_cache_row(c, 0, c.pos0 + r, _rope_row(c, "k", r, r))
    return "k_qkv_epi_rows"


def _attn_row_at(c, r, pos):
    s = c.model.shape
    q = P.rows_of(c.tap, "qr", s.dim)
    a = P.rows_of(c.tap, "attn", s.dim).copy()
    a[r] = R.oracle_attention(q[r], c.kva[0], c.kva[1], s.n_heads, s.n_kv_heads, s.head_dim, SEQ, pos, c.form.kv_f16)
    if np.array_equal(a.view(np.uint32), P.rows_of(c.tap, "attn", s.dim).view(np.uint32)):
        return None  # (the moved position has softmax weight 0 in every head of this row: the same bits, nothing to see)
    qt = c.tap["qtype"]["attn.act"]
    c.tap["attn"] = a.reshape(-1)
    c.tap["attn.act"] = np.concatenate([o.quantize(np.ascontiguousarray(v), qt) for v in a])
    if "attn.xh" in c.tap:
        c.tap["attn.xh"] = xh_of([o.quantize(np.ascontiguousarray(v), qt) for v in a], qt)
    if "attn.act.qp" in c.tap:
        c.tap["attn.act.qp"] = np.concatenate([R.class_major(R.parse_act(o.quantize(np.ascontiguousarray(v), qt), qt)["q"].reshape(-1)).astype(np.int8).view(np.uint8)
                                               for v in a])
    return "attention"


def m_mask_one_wide(c):
    return _attn_row_at(c, c.n // 2, c.pos0 + c.n // 2 + 1)


def m_mask_one_narrow(c):
    return _attn_row_at(c, c.n // 2, c.pos0 + c.n // 2 - 1)


def m_k_rows_swapped(c):
    a, b = c.pos0 + 2, c.pos0 + 3
    c.kva[0][:, [a, b], :] = c.kva[0][:, [b, a], :]
    return "k_qkv_epi_rows"


def m_v_row_in_k_cache(c):
    c.kva[0][:, c.pos0 + 1, :] = c.kva[1][:, c.pos0 + 1, :]
    return "k_qkv_epi_rows"


def m_cache_row_outside(c):
    at = c.pos0 + c.n if c.pos0 + c.n < SEQ else c.pos0 - 1
    c.kva[1][0, at, 0] = c.kva[1][0, at, 0] + (1 if c.form.kv_f16 else np.float32(1.0))
    return "k_qkv_epi_rows"


def m_qwen2_bias_missing_on_k(c):
    if c.model.shape.arch != "qwen2":
        return None
    for r in range(c.n):
        _set_cache_row(c, 0, c.pos0 + r, _rope_row(c, "k", r, c.pos0 + r, bias=False))
    return "k_qkv_epi_rows"


def m_drop_block_q(c):
    e = P.gemm_reference(c.tap, c.model, f"blk.{c.layer}.attn_q.weight", "n1.act", drop_last_block=True)[0]
    c.tap["q"] = e.astype(np.float32).reshape(-1)
    return "q|k|v gemm"


def m_drop_block_down(c):
    e = P.gemm_reference(c.tap, c.model, f"blk.{c.layer}.ffn_down.weight", "hid.act", drop_last_block=True)[0]
    parts = np.asarray(c.tap["down.parts"], dtype=np.float64).reshape(-1, *e.shape).sum(axis=0) if "down.parts" in c.tap else 0.0
    c.tap["down.tmp"] = (e - parts).astype(np.float32).reshape(-1)
    return "ffn_down"


def m_drop_k_piece(c):
    if "wo.parts" not in c.tap:
        return None
    c.tap["wo.parts"] = np.zeros_like(c.tap["wo.parts"])
    return "wo"


def m_norm_skips_last_piece(c):  # the norm launch adds wo's piece 0 only
    if "wo.parts" not in c.tap:
        return None
    dim = c.model.shape.dim
    c.tap["n2.x"] = (P.rows_of(c.tap, "wo.tmp", dim) + P.rows_of(c.tap, "n1.x", dim)).reshape(-1)
    return "norm n2"


def m_gate_up_swapped(c):
    qt = c.tap["qtype"]["hid.act"]
    h = np.stack([silu_mul(c.aux["u"][r], c.aux["g"][r], c.aux["odev"]) for r in range(c.n)])
    planes = [o.quantize(np.ascontiguousarray(v), qt) for v in h]
    c.tap["hid.act"] = np.concatenate(planes)
    if "hid.xh" in c.tap:
        c.tap["hid.xh"] = xh_of(planes, qt)
    if c.tap["plan"]["h_done"] == 1:
        c.tap["g"] = h.reshape(-1)
    if c.twin:
        c.twin["g"] = h.reshape(-1)
    return "gate|up"


def m_residual_not_added_on_one_row(c):
    dim = c.model.shape.dim
    x = P.rows_of(c.tap, "n2.x", dim).copy()
    r = c.n - 2
    x[r] = x[r] - P.rows_of(c.tap, "n1.x", dim)[r]
    c.tap["n2.x"] = x.reshape(-1)
    return "norm n2"


def m_pending_down_added_twice(c):
    if "in.tmp" not in c.tap:
        return None
    dim = c.model.shape.dim
    c.tap["n1.x"] = (P.rows_of(c.tap, "n1.x", dim) + P.rows_of(c.tap, "in.tmp", dim)).reshape(-1)
    return "norm n1"


def m_final_norm_from_row_b_minus_2(c):
    s = c.model.shape
    if c.layer != s.n_layers - 1:
        return None
    qt = c.tap["qtype"]["cls.act"]
    x = c.aux["x_final"][-2]
    cls = o.quantize(exact_norm(x, f32w(c.model, "output_norm.weight"), s.rms_eps, c.aux["odev"]), qt)
    c.tap["last.x"], c.tap["cls.act"], c.tap["logits"] = x.copy(), cls, mv(c.model.tensors["output.weight"], cls)
    return "tail"


def _n1_intervals(c):
    s = c.model.shape
    lo, hi, ref = P.norm_intervals(P.rows_of(c.tap, "n1.x", s.dim), c.aux["wn1"], s.rms_eps, s.dim)
    return R.QuantIntervals(lo, hi, ref, c.tap["qtype"]["n1.act"])


def _n1_blocks(c):
    bb = synth.BLOCK_BYTES[c.tap["qtype"]["n1.act"]]
    return np.asarray(c.tap["n1.act"]).copy().reshape(-1, bb), bb - 32


def m_one_quant(c):
    iv = _n1_intervals(c)
    b, off = _n1_blocks(c)
    bi, ei = np.argwhere(~iv.excused)[-1]
    q = b[bi, off + ei].view(np.int8)
    b[bi, off + ei] = np.int8(q - 1 if q > 0 else q + 1).view(np.uint8)
    c.tap["n1.act"] = b.reshape(-1)
    return "norm n1"


def m_one_scale_code(c):
    iv = _n1_intervals(c)
    b, _ = _n1_blocks(c)
    bi = int(np.flatnonzero(iv.single_code)[-1])
    b[bi, 0:2] = (b[bi, 0:2].copy().view(np.uint16) + 1).view(np.uint8)
    c.tap["n1.act"] = b.reshape(-1)
    return "norm n1"


def m_one_s_code(c):
    if c.tap["qtype"]["n1.act"] != o.Q8_1:
        return None
    iv = _n1_intervals(c)
    b, _ = _n1_blocks(c)
    lo, hi = iv.s_interval(R.parse_act(c.tap["n1.act"], o.Q8_1))
    bi = int(np.flatnonzero(lo == hi)[-1])
    b[bi, 2:4] = (b[bi, 2:4].copy().view(np.uint16) + 1).view(np.uint8)
    c.tap["n1.act"] = b.reshape(-1)
    return "norm n1"


def m_one_b_half_word(c):
    if "n1.xh" not in c.tap:
        return None
    xh = np.asarray(c.tap["n1.xh"]).copy()
    xh[xh.size - 5] ^= 1
    c.tap["n1.xh"] = xh
    return "norm n1"


# The wrong eps (the other of 1e-5 / 1e-6 in the layer's first norm launch) moves 1 / rms by 0.5 * 9e-6 / (mean square + eps): on the plain
# synthetic models that is often inside what the interval check must admit.  Applied to every model and rejected, except where this
# test verifies that the mutated planes are ones the reference alone admits (every changed quant excused, every changed scale in a
# two-code block) -- the admission rule of tests/test_fused_step_ref.py.  On the shrunk twin the rejection is unconditional.
def m_wrong_eps(c):
    s = c.model.shape
    other = 1e-6 if abs(s.rms_eps - 1e-5) < 1e-9 else 1e-5
    qt = c.tap["qtype"]["n1.act"]
    iv = _n1_intervals(c)
    before, off = _n1_blocks(c)
    x = P.rows_of(c.tap, "n1.x", s.dim)
    planes = [o.quantize(exact_norm(x[r], c.aux["wn1"], other, c.aux["odev"]), qt) for r in range(c.n)]
    after = np.concatenate(planes).reshape(before.shape)
    dq = before[:, off:] != after[:, off:]
    dd = np.any(before[:, 0:2] != after[:, 0:2], axis=1)  # (a Q8_1 block's s follows its own quants and scale: the checker derives it from them)
    if not np.any(dq & ~iv.excused) and not np.any(dd & iv.single_code):
        assert not c.small
        return None
    c.tap["n1.act"] = after.reshape(-1)
    if "n1.xh" in c.tap:
        c.tap["n1.xh"] = xh_of(planes, qt)
    return "norm n1"


MUTATIONS = [m_rope_last_row_next_pos, m_rope_ignores_pos0, m_k_rope_ignores_pos0, m_mask_one_wide, m_mask_one_narrow, m_k_rows_swapped,
             m_v_row_in_k_cache, m_cache_row_outside, m_qwen2_bias_missing_on_k, m_drop_block_q, m_drop_block_down, m_drop_k_piece,
             m_norm_skips_last_piece, m_gate_up_swapped, m_residual_not_added_on_one_row, m_pending_down_added_twice,
             m_final_norm_from_row_b_minus_2, m_one_quant, m_one_scale_code, m_one_s_code, m_one_b_half_word, m_wrong_eps]

CHECK = {"norm n1": lambda c, ctx: P.check_norm(c.tap, c.model, c.layer, "n1", ctx),
         "q|k|v gemm": lambda c, ctx: P.check_qkv_gemm(c.tap, c.model, c.layer, ctx),
         "k_qkv_epi_rows": lambda c, ctx: P.check_epi(c.tap, c.kvb, c.kva, c.model, c.layer, c.form, ctx),
         "attention": lambda c, ctx: P.check_attention(c.tap, c.kva, c.model, c.layer, c.form, ctx),
         "wo": lambda c, ctx: P.check_wo(c.tap, c.model, c.layer, ctx),
         "norm n2": lambda c, ctx: P.check_norm(c.tap, c.model, c.layer, "n2", ctx),
         "gate|up": lambda c, ctx: P.check_gateup(c.tap, c.model, c.layer, ctx, None, c.twin),
         "ffn_down": lambda c, ctx: P.check_down(c.tap, c.model, c.layer, ctx),
         "tail": lambda c, ctx: P.check_tail(c.tap, c.model, c.layer, ctx)}


@pytest.mark.parametrize("pos0", [0, 5])
@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0", "Q4_1"])
@pytest.mark.parametrize("shape", ["15m", "tiny-gqa", "tiny-hd128", "tiny-qwen2"])
def test_checker_accepts_the_oracle_pass_and_rejects_every_mutation(oracle, shape, fmt, pos0):
    plain = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=21, n_layers=2)
    shrunk = R.shrink_residual(synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=21, n_layers=2))
    applied = set()
    n = len(PASS_TOKS)
    # (model, f16 GEMM form, h_done, shrunk): the int8 form leaves g and u; the f16 form stores h or, with the row quantizer, only planes
    forms = [(plain, False, 0, False), (plain, True, 1, False), (shrunk, True, 2, True)]
    for model, f16w, h_done, small in forms:
        for layer in (0, 1):
            kv_f16 = (pos0 + layer) % 2 == 0
            ctx = f"{shape}{' (shrunk residual)' if small else ''} {fmt} {'f16' if f16w else 'int8'} h_done={h_done} kv_f16={kv_f16} layer {layer} pos0 {pos0}"
            tap, kvb, kva, form, aux = oracle_pass(model, pos0, n, layer, kv_f16, f16w, h_done)
            base = Case(model, layer, tap, kvb, kva, form, aux, small)
            res = P.check_pass(tap, PASS_TOKS[:n], kvb, kva, model, layer, form, ctx, None, base.twin)
            assert not P.failures(res), P.failures(res)
            for r in res.values():
                for name, share in r.excused.items():
                    assert share <= R.EXCUSED_CAP, (ctx, r.launch, name, share)
            for m in MUTATIONS:
                c = base.fork()
                launch = m(c)
                if launch is None:
                    continue
                applied.add(m.__name__)
                got = CHECK[launch](c, ctx)
                assert got.fails, f"{ctx}: the checker let {m.__name__} through at {launch} (worst error / bound {got.worst:.3g}, excused {got.excused})"
    skipped = {m.__name__ for m in MUTATIONS} - applied
    allowed = set()
    if synth.SHAPES[shape].arch != "qwen2":
        allowed |= {"m_qwen2_bias_missing_on_k"}
    if fmt != "Q4_1":
        allowed |= {"m_one_s_code"}
    if pos0 == 0:
        allowed |= {"m_rope_ignores_pos0", "m_k_rope_ignores_pos0"}
    assert skipped <= allowed, skipped  # (the eps mutation is always applied at least on the shrunk twin)


def _flash_case(base):
    """the same pass as k_attn_flash_rows may leave it: the attention output is float64 causal attention on the stored f16 inputs,
    rounded once to f32 (one admissible output of that kernel), planes and B' of that output, the plan naming the kernel"""
    c = base.fork()
    s, n = c.model.shape, c.n
    q = P.rows_of(c.tap, "qr", s.dim)
    a = P.f64_causal_attention(q, c.kva[0], c.kva[1], s.n_heads, s.n_kv_heads, s.head_dim, SEQ, c.pos0, n).astype(np.float32).reshape(n, -1)
    c.tap["plan"] = dict(c.tap["plan"], attn_kernel=P.ATTN_FLASH_ROWS)
    _put_attn(c, a)
    return c


def _put_attn(c, a):
    qt = c.tap["qtype"]["attn.act"]
    planes = [o.quantize(np.ascontiguousarray(v), qt) for v in a]
    c.tap["attn"], c.tap["attn.act"] = a.reshape(-1), np.concatenate(planes)
    if "attn.xh" in c.tap:
        c.tap["attn.xh"] = xh_of(planes, qt)


def _flash_row_at(c, r, pos):
    """row r attends positions 0 .. pos instead of 0 .. pos0 + r (float64, as _flash_case)"""
    s = c.model.shape
    q = P.rows_of(c.tap, "qr", s.dim)
    a = P.rows_of(c.tap, "attn", s.dim).copy()
    a[r] = R.f64_attention(q[r], c.kva[0], c.kva[1], s.n_heads, s.n_kv_heads, s.head_dim, SEQ, pos).astype(np.float32)
    _put_attn(c, a)


@pytest.mark.parametrize("pos0", [0, 5])
@pytest.mark.parametrize("fmt", ["Q4_0", "Q4_1"])
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128", "tiny-qwen2"])
def test_checker_on_a_flash_rows_tap(oracle, shape, fmt, pos0):
    """plan["attn_kernel"] == ATTN_FLASH_ROWS, the default from 96 cached positions on: the checker's float64 branch accepts an oracle-made
    pass whose attention output is the float64 one, and rejects the causal mask one position wide or narrow on one row (the row the
    slip moves most), under the FLASH_ROWS_REL * max|out| bound (how far that bound sees at the GPU file's lengths: test_flash_rows_bound_sees_a_mask_slip_at_the_long_lengths)"""
    model = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=21, n_layers=2)
    n = len(PASS_TOKS)
    for layer in (0, 1):
        ctx = f"{shape} {fmt} flash rows layer {layer} pos0 {pos0}"
        tap, kvb, kva, form, aux = oracle_pass(model, pos0, n, layer, True, True, 1)
        c = _flash_case(Case(model, layer, tap, kvb, kva, form, aux, False))
        got = P.check_attention(c.tap, c.kva, model, layer, form, ctx)
        assert not got.fails and got.worst < 1e-3, (got.fails, got.worst)  # (its own f32 rounding only)
        s = model.shape
        q, a = P.rows_of(c.tap, "qr", s.dim), P.rows_of(c.tap, "attn", s.dim).astype(np.float64)
        bound = P.FLASH_ROWS_REL * np.max(np.abs(a))
        for shift in (1, -1):
            # the row on which the slip moves the float64 output most (a position the softmax gives no weight moves nothing, and no
            # check of the output can see it): chosen from the reference alone; these models must give one that moves by more than the bound (1 % over: the f32 rounding
            # of the mutated row is 6e-8 of it)
            rows = [r for r in range(n) if 0 <= pos0 + r + shift < pos0 + n]
            moved = [np.max(np.abs(R.f64_attention(q[r], c.kva[0], c.kva[1], s.n_heads, s.n_kv_heads, s.head_dim, SEQ, pos0 + r + shift) - a[r])) for r in rows]
            r = rows[int(np.argmax(moved))]
            assert max(moved) > 1.01 * bound, (ctx, shift, max(moved), bound)
            m = c.fork()
            _flash_row_at(m, r, pos0 + r + shift)
            got = P.check_attention(m.tap, m.kva, model, layer, form, ctx)
            assert got.fails, f"{ctx}: the flash-rows check let a mask {shift:+d} position on row {r} through (worst error / bound {got.worst:.3g})"


def _attention_only(rng, n_pos, seq_cap, pos0, rows, kernel):
    """a tap holding only what check_attention reads, on random f16 K / V rows and f32 q rows of the tiny-gqa geometry"""
    s = synth.SHAPES["tiny-gqa"]
    kc = (rng.standard_normal((s.n_kv_heads, seq_cap, s.head_dim)) * 0.7).astype(np.float16).view(np.uint16)
    vc = (rng.standard_normal((s.n_kv_heads, seq_cap, s.head_dim)) * 0.7).astype(np.float16).view(np.uint16)
    q = (rng.standard_normal((rows, s.dim)) * 0.3).astype(np.float32)
    tap = {"plan": {"rows": rows, "pos0": pos0, "attn_kernel": kernel}, "qr": q.reshape(-1), "qtype": {"attn.act": o.Q8_0}}
    return s, tap, (kc, vc), P.Form(kv_f16=True, seq_cap=seq_cap)


def _with_attn(tap, a):
    t = dict(tap)
    t["attn"] = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    t["attn.act"] = np.concatenate([o.quantize(np.ascontiguousarray(v, dtype=np.float32), o.Q8_0) for v in a])
    return t


def test_flash_rows_bound_sees_a_mask_slip_at_the_long_lengths(oracle):
    """How far the bound the project states for k_attn_flash_rows (FLASH_ROWS_REL of max|out| over the pass) sees ONE row's mask being one
    position wide at the GPU file's lengths: a slip at position n moves the row's output by about p_n |v_n - out| ~ 1 / n of a V row
    while the bound is a constant of the pass.  On random rows it is seen on an early row and on the LAST row of a 130-row and of a
    384-row pass."""
    import types
    rng = np.random.default_rng(17)
    seen = {}
    for rows in (130, 384):
        s, tap, kv, form = _attention_only(rng, rows, rows + 1, 0, rows, P.ATTN_FLASH_ROWS)
        q = P.rows_of(tap, "qr", s.dim)
        a = P.f64_causal_attention(q, kv[0], kv[1], s.n_heads, s.n_kv_heads, s.head_dim, form.seq_cap, 0, rows).astype(np.float32).reshape(rows, -1)
        model = types.SimpleNamespace(shape=s)
        assert not P.check_attention(_with_attn(tap, a), kv, model, 0, form, "flash").fails
        for r in (32, rows - 1):
            m = a.copy()
            m[r] = R.f64_attention(q[r], kv[0], kv[1], s.n_heads, s.n_kv_heads, s.head_dim, form.seq_cap, r + 1).astype(np.float32)
            seen[(rows, r)] = bool(P.check_attention(_with_attn(tap, m), kv, model, 0, form, "flash").fails)
    assert all(seen.values()), seen


def test_long_row_hull_is_the_reference_chain_and_holds_the_mask(oracle):
    """the exact long-row kernels past 1024 cached positions (plan["attn_kernel"] == ATTN_LONG_ROWS): with no slack on the row sum the
    restated f16 chain IS the reference's attention, bit for bit; with the slack of a re-associated row sum the reference lies inside
    the hull, the hull is a few f16 steps wide, and a row whose mask is one position wide or narrow lies outside it.  Rows of the same
    pass at up to 1024 positions stay bit for bit."""
    import types
    rng = np.random.default_rng(3)
    pos0, rows, cap = 1020, 8, 1040
    s, tap, kv, form = _attention_only(rng, pos0 + rows, cap, pos0, rows, P.ATTN_LONG_ROWS)
    q = P.rows_of(tap, "qr", s.dim)
    att = lambda r, pos: R.oracle_attention(q[r], kv[0], kv[1], s.n_heads, s.n_kv_heads, s.head_dim, cap, pos, True)
    a = np.stack([att(r, pos0 + r) for r in range(rows)])
    lo, hi = P.long_row_hull(q[7], kv[0], kv[1], s.n_heads, s.n_kv_heads, s.head_dim, cap, pos0 + 7, rel=0.0)
    assert np.array_equal(lo, a[7].astype(np.float64)) and np.array_equal(hi, lo)
    lo, hi = P.long_row_hull(q[7], kv[0], kv[1], s.n_heads, s.n_kv_heads, s.head_dim, cap, pos0 + 7)
    assert np.all((lo <= a[7]) & (a[7] <= hi)) and np.max(hi - lo) <= 4e-3 * np.max(np.abs(a[7]))
    model = types.SimpleNamespace(shape=s)
    assert not P.check_attention(_with_attn(tap, a), kv, model, 0, form, "long rows").fails
    for r in (2, 6):  # (2: 1023 positions, the bit-for-bit side; 6: 1027, the hull)
        for shift in (1, -1):
            m = a.copy()
            m[r] = att(r, pos0 + r + shift)
            assert P.check_attention(_with_attn(tap, m), kv, model, 0, form, "long rows").fails, (r, shift)
    m = a.copy()
    m[2, 5] = np.nextafter(m[2, 5], np.float32(9))  # one f32 ulp on a row that must be exact
    assert P.check_attention(_with_attn(tap, m), kv, model, 0, form, "long rows").fails


def test_sample_holds_both_end_tiles_and_the_row_at_pos0():
    """Sample (the 8B row lengths of the GPU file): the first and the last 64-row tile of a matrix, and the first and the last column tile
    of the pass for every tile the launcher may choose (16 T rows, T = 2, 4, 8)"""
    sm = P.Sample()
    for m in (64, 100, 4096, 14336, 14337):
        w = set(sm.wrows(m).tolist())
        assert set(range(min(64, m))) <= w and set(range((m - 1) // 64 * 64, m)) <= w
    for b in (33, 40, 136, 200, 384):
        pr = set(sm.prows(b).tolist())
        assert 0 in pr
        for T in (2, 4, 8):
            tile = 16 * T
            assert set(range(min(tile, b))) <= pr and set(range((b - 1) // tile * tile, b)) <= pr, (b, T)


def test_row_dots_many_is_row_dots(oracle):
    """the weight-ROW SELECTION of the multi-row form the pass checks use: row_dots is a wrapper around row_dots_many, so this pins only
    that a selection returns the same rows as the whole matrix (the arithmetic itself: tests/test_fused_step_ref.py, on row_dots)"""
    rng = np.random.default_rng(9)
    for typ, qt in ((synth.Q4_0, o.Q8_0), (synth.Q8_0, o.Q8_0), (synth.Q4_1, o.Q8_1)):
        t = synth.RawTensor(synth.random_blocks(rng, 300 * 96, typ), [300, 96], typ)
        acts = [R.parse_act(o.quantize(rng.standard_normal(96).astype(np.float32), qt), qt) for _ in range(3)]
        sel = np.array([0, 5, 255, 256, 299])
        e, b = R.row_dots_many(t, acts, sel)
        for i, a in enumerate(acts):
            e1, b1 = R.row_dots(t, a)
            assert np.array_equal(e[i], e1[sel]) and np.array_equal(b[i], b1[sel])


# ---- Q8_K-row passes (K-quant layers): oracle-made taps of both norm arms, the f16 and the int8 forms, with k pieces ----
K_FMTS = {"Q4_K": (synth.Q4_K, False), "Q4_K_M": (synth.Q4_K, True), "Q6_K": (synth.Q6_K, False), "Q5_K": (synth.Q5_K, False),
          "Q5_K_M": (synth.Q5_K, True)}


def k_model(shape, fmt, shrunk=False):
    wtype, mix = K_FMTS[fmt]
    model = synth.build_model(synth.SHAPES[shape], wtype, seed=21, n_layers=2, k_m_mix=mix)
    if shrunk:
        model = (Q5.shrink_residual if wtype == synth.Q5_K else R.shrink_residual)(model, 7)
    return model


def _kq(c):
    return c.tap["qtype"]["n1.act"] == o.Q8_K


def _typ(c, nm):
    return c.model.tensors[f"blk.{c.layer}.{nm}.weight"].typ


def _mutated_gemm(c, nm, act_name, out_name, launch, model=None, wrong=None):
    """the GEMM output a kernel that is wrong in the given way leaves: the exact dot of the WRONG weights / pieces, rounded once"""
    e = P.gemm_reference(c.tap, model or c.model, f"blk.{c.layer}.{nm}.weight", act_name, wrong=wrong)[0]
    new = e.astype(np.float32).reshape(-1)
    assert not np.array_equal(new, np.asarray(c.tap[out_name])), (nm, wrong)
    c.tap[out_name] = new
    return launch


def _with_bytes(c, nm, edit):
    """the model with blk.layer.nm's blocks edited (a copy of that tensor only)"""
    name = f"blk.{c.layer}.{nm}.weight"
    t = c.model.tensors[name]
    blk = t.data.copy().reshape(-1, synth.BLOCK_BYTES[t.typ])
    edit(blk)
    m = copy.copy(c.model)
    m.tensors = dict(c.model.tensors)
    m.tensors[name] = synth.RawTensor(blk.reshape(-1), t.shape, t.typ)
    return m


def m_k_min_term_dropped(c):  # (Q4_K) the minimum of sub-block 2 of every super-block reads 0: its dmin m term is dropped
    if not _kq(c) or _typ(c, "attn_q") != synth.Q4_K:
        return None

    def edit(blk):
        blk[:, 4 + 4 + 2] &= 0xC0  # mn[2] = the low six bits of scales[6] (util.rs:19-27)
    return _mutated_gemm(c, "attn_q", "n1.act", "q", "q|k|v gemm", model=_with_bytes(c, "attn_q", edit))


def m_k_q6_neighbour_scale(c):  # (Q6_K) 16-group 5 of every super-block is scaled with group 6's scale
    if not _kq(c) or _typ(c, "attn_v") != synth.Q6_K:
        return None

    def edit(blk):
        blk[:, 192 + 5] = blk[:, 192 + 6]
    return _mutated_gemm(c, "attn_v", "n1.act", "v", "q|k|v gemm", model=_with_bytes(c, "attn_v", edit))


def _m_q5k(wrong):
    def m(c):
        if not _kq(c) or _typ(c, "ffn_gate") != synth.Q5_K:
            return None
        if c.tap["plan"]["h_done"] != 0:  # (g is not stored: through wo)
            return _mutated_gemm(c, "attn_output", "attn.act", "wo.tmp", "wo", wrong=wrong)
        return _mutated_gemm(c, "ffn_gate", "n2.act", "g", "gate|up", wrong=wrong)
    m.__name__ = "m_q5k_" + wrong
    return m


Q5K_MUTATIONS = [_m_q5k(w) for w in Q5.WRONG]


def q8k_pos(order, E):
    """f16w_pos_q8k (f16w_rows.hpp) for super-block 0: the position of element E in B' for k-slot order 1 (Q4_K weights) / 2 (Q6_K)"""
    if order == 1:
        l = E & 7
        g, hi, k, s, cc = E >> 6, (E >> 5) & 1, (E >> 3) & 3, l & 3, l >> 2
    else:
        r2 = E & 63
        hi, g, s, k, cc = (E >> 6) & 1, 2 * (r2 >> 5) + ((r2 >> 4) & 1), (r2 >> 2) & 3, r2 & 3, E >> 7
    return (4 * cc + g) * 32 + 8 * s + 4 * hi + ((k >> 1) | ((k & 1) << 1))


def m_k_v_reads_q4k_order(c):
    """a Q4_K_M layer whose v (Q6_K) does not re-make B': its GEMM finds B' in Q4_K's k-slot order, i.e. multiplies element E of A' with
    the element that order 1 put where order 2 has E.  B' itself is the right multiset: only v's GEMM output can show it"""
    if not _kq(c) or "n1.xh.v" not in c.tap or "n1.xh" not in c.tap:
        return None
    E = np.arange(256)
    p1, p2 = np.array([q8k_pos(1, e) for e in E]), np.array([q8k_pos(2, e) for e in E])
    assert sorted(p1) == sorted(p2) == list(range(256))
    inv1 = np.empty(256, dtype=np.int64)
    inv1[p1] = E
    found = inv1[p2]  # the element found where element E is expected
    assert np.any(found != E)
    t = c.model.tensors[f"blk.{c.layer}.attn_v.weight"]
    m, k = t.shape
    ap = weight_operands(np.ascontiguousarray(t.data).view(np.uint8).reshape(-1), "Q6_K", list(range(m)), k)[0]
    bp = P.b_prime(P.act_rows(c.tap, "n1.act"))[1].reshape(c.n, k // 256, 256)[:, :, found].reshape(c.n, k)
    c.tap["v"] = (bp @ ap.T).astype(np.float32).reshape(-1)
    return "q|k|v gemm"


def _xh_fields(c):
    return [(x, a, launch) for x, a, launch in (("n1.xh", "n1.act", "norm n1"), ("n1.xh.v", "n1.act", "norm n1"), ("attn.xh", "attn.act", "attention"),
                                                ("n2.xh", "n2.act", "norm n2"), ("hid.xh", "hid.act", "gate|up")) if x in c.tap]


def m_k_bprime_f16_scale(c):  # B' = f16(q) * f16(d): the scale rounded to f16 first
    if not _kq(c) or not _xh_fields(c):
        return None
    xh, act, launch = _xh_fields(c)[0]
    acts = P.act_rows(c.tap, act)
    with np.errstate(over="ignore"):
        v = np.stack([(a["q"].astype(np.float16) * a["d"].astype(np.float16)[:, None]).reshape(-1) for a in acts]).astype(np.float16)
    assert not np.array_equal(v.view(np.uint16).reshape(-1), np.asarray(c.tap[xh]))
    c.tap[xh] = v.view(np.uint16).reshape(-1)
    return launch


def single_rounding(acts):
    """f16 of the float64 product q d: ONE rounding, where the kernels and the checker round to f32 first"""
    with np.errstate(over="ignore"):
        return np.stack([(a["q"] * a["d"][:, None]).reshape(-1) for a in acts]).astype(np.float16).view(np.uint16)


def m_k_bprime_single_rounding(c):
    """differs from f16(f32(q d)) only where the f32 rounding lands on an f16 tie: the pass's own planes are searched for such an element,
    field by field; a pass that has none in any field leaves every bit as it was -- proven here by comparing the bits -- and the standalone
    search of test_b_prime_is_two_roundings covers the case"""
    if not _kq(c):
        return None
    for xh, act, launch in _xh_fields(c):
        one = single_rounding(P.act_rows(c.tap, act)).reshape(-1)
        if not np.array_equal(one, np.asarray(c.tap[xh])):
            c.tap[xh] = one
            return launch
    return None


def m_k_bsum_off_by_one(c):
    if not _kq(c):
        return None
    b = np.asarray(c.tap["attn.act"]).copy().reshape(-1, 292)
    s16 = b[-1, 260:292].copy().view(np.int16)
    s16[7] += 1
    b[-1, 260:292] = s16.view(np.uint8)
    c.tap["attn.act"] = b.reshape(-1)
    return "attention"


def m_k_class_major_swapped(c):
    if not _kq(c):
        return None
    qp = np.asarray(c.tap["hid.act.qp"]).copy()
    i = int(np.flatnonzero(qp[:-1] != qp[1:])[-1])
    qp[i], qp[i + 1] = qp[i + 1], qp[i]
    c.tap["hid.act.qp"] = qp
    return "gate|up"


def m_k_one_quant(c):
    if not _kq(c):
        return None
    b = np.asarray(c.tap["n2.act"]).copy().reshape(-1, 292)
    q = int(b[3, 4 + 100].view(np.int8))
    b[3, 4 + 100] = np.int8(q - 1 if q > 0 else q + 1).view(np.uint8)
    # (its own sum and class-major byte follow the quant: the byte comparison with the reference quantizer must see it)
    a = R.parse_act(b[3], o.Q8_K)
    b[3, 260:292] = a["q"].reshape(16, 16).sum(axis=1).astype(np.int16).view(np.uint8)
    c.tap["n2.act"] = b.reshape(-1)
    c.tap["n2.act.qp"] = np.concatenate([R.class_major(R.parse_act(r, o.Q8_K)["q"].reshape(-1)).astype(np.int8).view(np.uint8)
                                         for r in b.reshape(c.n, -1)])
    return "norm n2"


def _put_norm(c, which, xn):
    planes = [o.quantize(np.ascontiguousarray(v, dtype=np.float32), o.Q8_K) for v in xn]
    c.tap[which + ".xn"] = np.ascontiguousarray(xn, dtype=np.float32).reshape(-1)
    c.tap[which + ".act"] = np.concatenate(planes)
    c.tap[which + ".act.qp"] = np.concatenate([R.class_major(R.parse_act(p, o.Q8_K)["q"].reshape(-1)).astype(np.int8).view(np.uint8) for p in planes])
    for xh in (which + ".xh", which + ".xh.v"):
        if xh in c.tap:
            c.tap[xh] = xh_of(planes, o.Q8_K)


def m_k_norm_reads_x_before_the_add_on_one_row(c):
    """the FFN norm of ONE row reads x as it was before wo's output was added (x itself is stored right): that row's xn, planes and B'
    are those of the old x, consistent among themselves"""
    if not _kq(c):
        return None
    s, r = c.model.shape, c.n - 4
    xn = P.rows_of(c.tap, "n2.xn", s.dim).copy()
    xn[r] = exact_norm(P.rows_of(c.tap, "n1.x", s.dim)[r], f32w(c.model, f"blk.{c.layer}.ffn_norm.weight"), 1e-5, c.aux["odev"])
    _put_norm(c, "n2", xn)
    return "norm n2"


def m_k_norm_n1_skips_last_piece(c):  # k_norm_quant_rows_k adds the pending ffn_down piece 0 only; everything downstream of that x is consistent
    if not _kq(c) or "in.parts" not in c.tap:
        return None
    s = c.model.shape
    x = P.rows_of(c.tap, "in.tmp", s.dim) + P.rows_of(c.tap, "in.x", s.dim)
    c.tap["n1.x"] = x.reshape(-1)
    _put_norm(c, "n1", np.stack([exact_norm(v, c.aux["wn1"], s.rms_eps, c.aux["odev"]) for v in x]))
    return "norm n1"


def m_k_wrong_eps(c):
    """the other of 1e-5 / 1e-6 in the layer's first norm: rejected, except where every element of the mutated xn still lies inside the
    interval the reference alone gives (verified here; never on the shrunk model)"""
    if not _kq(c):
        return None
    s = c.model.shape
    other = 1e-6 if abs(s.rms_eps - 1e-5) < 1e-9 else 1e-5
    x = P.rows_of(c.tap, "n1.x", s.dim)
    xn = np.stack([exact_norm(v, c.aux["wn1"], other, c.aux["odev"]) for v in x])
    lo, hi, _ = P.norm_intervals(x, c.aux["wn1"], s.rms_eps, s.dim)
    if np.all((xn >= lo) & (xn <= hi)):
        assert not c.small
        return None
    _put_norm(c, "n1", xn)
    return "norm n1"


def m_k_h_done_2(c):
    if not _kq(c):
        return None
    c.tap["plan"] = dict(c.tap["plan"], h_done=2)
    return "gate|up"


K_MUTATIONS = [m for m in MUTATIONS if m not in (m_one_quant, m_one_scale_code, m_one_s_code, m_wrong_eps)] + Q5K_MUTATIONS + [
    m_k_min_term_dropped, m_k_q6_neighbour_scale, m_k_v_reads_q4k_order, m_k_bprime_f16_scale, m_k_bprime_single_rounding, m_k_bsum_off_by_one,
    m_k_class_major_swapped, m_k_one_quant, m_k_norm_reads_x_before_the_add_on_one_row, m_k_norm_n1_skips_last_piece, m_k_wrong_eps, m_k_h_done_2]


@pytest.mark.parametrize("pos0", [0, 5])
@pytest.mark.parametrize("fmt", sorted(K_FMTS))
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128", "tiny-qwen2"])
def test_checker_accepts_the_oracle_k_pass_and_rejects_every_mutation(oracle, shape, fmt, pos0):
    """Q8_K-row passes.  Forms: the separate norm launches with the int8 kernels (g, u and h stored), k_norm_quant_rows_k with the f16
    GEMMs and k pieces (g, u and h stored), and the same on the shrunk model with h from the GEMM's epilogue.  No launch may need an
    interval excuse: every excused share is 0.  A mutation that does not apply to a (format, layer, form) returns None; what may stay
    unapplied over all forms of a case is listed at the end and nothing else may."""
    applied = set()
    n = len(PASS_TOKS)
    forms = [(False, False, 0, False), (False, True, 0, True), (True, True, 1, True)]  # (shrunk, f16 GEMMs, h_done, fused norm)
    for small, f16w, h_done, fused in forms:
        model = k_model(shape, fmt, small)
        for layer in (0, 1):
            kv_f16 = (pos0 + layer) % 2 == 0
            ctx = f"{shape}{' (shrunk residual)' if small else ''} {fmt} {'f16' if f16w else 'int8'} h_done={h_done} fused={fused} kv_f16={kv_f16} layer {layer} pos0 {pos0}"
            tap, kvb, kva, form, aux = oracle_pass(model, pos0, n, layer, kv_f16, f16w, h_done, fused)
            assert tap["plan"]["norm_kernel"] == (4 if fused else 0)
            base = Case(model, layer, tap, kvb, kva, form, aux, small)
            res = P.check_pass(tap, PASS_TOKS[:n], kvb, kva, model, layer, form, ctx, None, None)
            assert not P.failures(res), P.failures(res)
            assert not any(r.excused for r in res.values()), {k: r.excused for k, r in res.items()}
            for m in K_MUTATIONS:
                c = base.fork()
                launch = m(c)
                if launch is None:
                    continue
                applied.add(m.__name__)
                got = CHECK[launch](c, ctx)
                assert got.fails, f"{ctx}: the checker let {m.__name__} through at {launch} (worst error / bound {got.worst:.3g})"
    skipped = {m.__name__ for m in K_MUTATIONS} - applied
    wtype, mix = K_FMTS[fmt]
    allowed = {"m_k_bprime_single_rounding"}  # (a pass without a double-rounding element: bit-equal, proven inside the mutation)
    if synth.SHAPES[shape].arch != "qwen2":
        allowed |= {"m_qwen2_bias_missing_on_k"}
    if pos0 == 0:
        allowed |= {"m_rope_ignores_pos0", "m_k_rope_ignores_pos0"}
    if wtype != synth.Q4_K:
        allowed |= {"m_k_min_term_dropped"}
    if wtype != synth.Q5_K:
        allowed |= {m.__name__ for m in Q5K_MUTATIONS}
    if not (mix or wtype == synth.Q6_K):
        allowed |= {"m_k_q6_neighbour_scale"}
    if not (mix and wtype == synth.Q4_K):
        allowed |= {"m_k_v_reads_q4k_order"}
    if wtype == synth.Q5_K and not mix:  # (no matrix of a pure Q5_K model takes the f16 GEMM: no B', no k pieces)
        allowed |= {"m_k_bprime_f16_scale", "m_drop_k_piece", "m_norm_skips_last_piece", "m_k_norm_n1_skips_last_piece", "m_one_b_half_word"}
    if wtype == synth.Q5_K and mix:  # (wo is Q5_K: the GEMV leaves no pieces; ffn_down of layer 0 is Q5_K too)
        allowed |= {"m_drop_k_piece", "m_norm_skips_last_piece", "m_k_norm_n1_skips_last_piece", "m_one_b_half_word"}
    assert skipped <= allowed, skipped


def _planes_tap(rows):
    planes = [o.quantize(np.ascontiguousarray(v, dtype=np.float32), o.Q8_K) for v in rows]
    qp = [R.class_major(R.parse_act(p, o.Q8_K)["q"].reshape(-1)).astype(np.int8).view(np.uint8) for p in planes]
    return {"x.act": np.concatenate(planes), "x.act.qp": np.concatenate(qp), "qtype": {"x.act": o.Q8_K}}


def test_q8k_byte_check_holds_ties_and_the_first_maximum(oracle):
    """check_planes_of -- what every Q8_K launch's planes go through -- on crafted rows.  A super-block whose maximum is -128 has the scale
    1, so 2.5 and -3.5 are ties: the reference rounds them AWAY from zero (3, -4), half-to-even would give 2, -4 / 2: one quant differs.
    A super-block whose maximum magnitude is held by +7 (element 9) and then by -7 (element 40): the FIRST holder decides the sign of d
    (negative) and every quant; taking the second flips all of them."""
    row = np.zeros(512, dtype=np.float32)
    row[:256] = np.linspace(-100, 100, 256)
    row[3], row[17], row[30] = -128.0, 2.5, -3.5
    row[256:] = np.linspace(-5, 5, 256)
    row[256 + 9], row[256 + 40] = 7.0, -7.0
    rows = row[None, :]
    tap = _planes_tap(rows)
    res = R.Result("planes")
    P.check_planes_of(res, tap, "x.act", rows, "crafted", "crafted")
    assert not res.fails, res.fails
    a = R.parse_act(tap["x.act"], o.Q8_K)
    assert a["q"][0, 17] == 3 and a["q"][0, 30] == -4 and a["d"][1] < 0 and a["q"][1, 9] == -128 and a["q"][1, 40] == 127

    def mutated(edit):
        t = dict(tap)
        b = tap["x.act"].copy().reshape(2, 292)
        edit(b)
        for i in range(2):  # (sums and the class-major plane follow the quants: only the byte comparison can see the quantizer's slip)
            b[i, 260:292] = b[i, 4:260].view(np.int8).astype(np.int64).reshape(16, 16).sum(axis=1).astype(np.int16).view(np.uint8)
        t["x.act"] = b.reshape(-1)
        t["x.act.qp"] = R.class_major(b[:, 4:260].view(np.int8).reshape(-1)).view(np.uint8)
        r = R.Result("planes")
        P.check_planes_of(r, t, "x.act", rows, "crafted", "crafted")
        return r.fails

    def half_even(b):
        b[0, 4 + 17] = np.int8(2).view(np.uint8)

    def second_holder(b):  # mx = -7: scale = 128 / 7 > 0, d > 0, every quant of the block negated (and clipped at 127)
        sc = np.float32(-128.0) / np.float32(-7.0)
        q = np.minimum(np.sign(row[256:] * sc) * np.floor(np.abs(row[256:] * sc) + np.float32(0.5)), 127)
        b[1, 4:260] = q.astype(np.int8).view(np.uint8)
        b[1, 0:4] = np.array([np.float32(1.0) / sc], dtype=np.float32).view(np.uint8)

    assert mutated(half_even) and mutated(second_holder)
    assert not mutated(lambda b: None)


def test_b_prime_is_two_roundings(oracle):
    """B' of Q8_K rows is f16(f32(q d)).  Rows are SEARCHED (fixed seed) for an element on which the single rounding f16(q d) differs --
    it need not exist in a given pass --; on that row check_xh accepts the two-rounding B' and rejects the single-rounding one, and the one
    made of f16(q) * f16(d)."""
    import types
    rng = np.random.default_rng(11)
    model = types.SimpleNamespace(tensors={"w": types.SimpleNamespace(typ=synth.Q4_K)})
    for _ in range(400):
        row = (rng.standard_normal(512) * rng.uniform(0.1, 30)).astype(np.float32)
        planes = o.quantize(row, o.Q8_K)
        acts = [R.parse_act(planes, o.Q8_K)]
        two, one = P.b_prime(acts)[0], single_rounding(acts)
        if not np.array_equal(two, one):
            break
    else:
        raise AssertionError("no double-rounding element in 400 rows")
    assert int((two != one).sum()) >= 1
    tap = {"plan": {"rows": 1}, "n1.act": planes, "qtype": {"n1.act": o.Q8_K}}
    with np.errstate(over="ignore"):
        scaled = (acts[0]["q"].astype(np.float16) * acts[0]["d"].astype(np.float16)[:, None]).reshape(-1).astype(np.float16).view(np.uint16)
    for bits, ok in ((two, True), (one, False), (scaled, False)):
        res = R.Result("norm n1")
        P.check_xh(res, dict(tap, **{"n1.xh": bits.reshape(-1)}), "n1.xh", "n1.act", "search", model, "w")
        assert bool(res.fails) != ok, (ok, res.fails)
