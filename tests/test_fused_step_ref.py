"""The checker of the fast fused launches (tests/fused_step_ref.py) decides what tests/test_hip_fused_launches.py can see, so it
is tested first, without a device.

A tap is built from the ORACLE: one token step walked launch by launch with the reference's own ops (its quantizer, its scalar
vec_dot per row, its rope / attention / SiLU), in the exact-norm form and -- by the kernels' stated expression (quantize
f32(x * w_norm), chunk sums of squares, row dots times 1 / rms) -- in the hop-free form.  The reference's scalar order is one
admissible order of the f32 sums, so the checker must ACCEPT both taps; then it must REJECT every single mutation of them listed in
MUTATIONS (a kernel that is subtly wrong in exactly that way), on every model."""
import copy

import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests.helpers import to_oracle
from tests.qwen2_ref import OracleQwen2Runner, to_oracle_qwen2

SEQ = 16
TOKS = [1, 365, 400, 282, 7, 9, 11, 13]


def _ot(v, odev):
    v = np.ascontiguousarray(v, dtype=np.float32)
    return o.OracleTensor.new(v, [v.size], odev)


def mv(t, planes):
    """W . planes, every row in the reference's scalar block order (vec_dot, f32)"""
    rows, k = t.shape
    raw = np.ascontiguousarray(t.data).reshape(rows, -1)
    return np.array([o.vec_dot(raw[r], t.typ, planes, k) for r in range(rows)], dtype=np.float32)


def exact_norm(x, w, eps, odev):
    return _ot(x, odev).rms_norm_inplace(eps).mul_inplace(_ot(w, odev)).export()


def rope(v, n_heads, hd, pos, rope_dim, neox, odev):
    t = o.OracleTensor.new(np.ascontiguousarray(v, dtype=np.float32), [1, n_heads, hd], odev)
    return t.rope_inplace(o.ROPE_NEOX if neox else o.ROPE_LLAMA, pos, rope_dim).export().reshape(-1)


def f32_inv_rms(rsums, n, eps):
    """1 / rms as the consuming launches form it (rms_finish): the chunk sums added (here: exactly, rounded once -- one admissible
    order), times 1 / n, plus eps, reciprocal square root"""
    s = np.float32(np.sum(rsums.astype(np.float64)))
    return np.float32(1.0 / np.sqrt(np.float64(s * np.float32(1.0 / n) + np.float32(eps))))


def silu_mul(g, u, odev):
    return _ot(g, odev).silu_inplace().mul_inplace(_ot(u, odev)).export()


def oracle_tap(model, pos, layer, kv_f16, hop_free):
    """(tap, kc_raw, vc_raw, form, aux) of one token step at `pos` with `layer` tapped, from the oracle's ops"""
    s = model.shape
    odev = o.OracleDevice(thread_num=1)
    qwen2 = s.arch == "qwen2"
    conf, w = (to_oracle_qwen2 if qwen2 else to_oracle)(model, odev)
    runner = (OracleQwen2Runner if qwen2 else o.OracleLlamaRunner)(conf, w, odev, SEQ, kv_f16)
    for i in range(pos):
        runner.forward_llama([TOKS[i]], i)
    kdt = np.uint16 if kv_f16 else np.float32
    kcs = [np.array(c.storage, dtype=kdt).reshape(s.n_kv_heads, SEQ, s.head_dim) for c in runner.key_cache]
    vcs = [np.array(c.storage, dtype=kdt).reshape(s.n_kv_heads, SEQ, s.head_dim) for c in runner.value_cache]
    wt = model.wtype
    qt = o.rhs_dtype(wt)
    dim, hd, L = s.dim, s.head_dim, s.n_layers
    rope_dim = s.rope_dim if s.rope_dim is not None else hd
    f32w = lambda n: np.ascontiguousarray(model.tensors[n].data).view(np.float32)
    emb = model.tensors["token_embd.weight"]
    x = o.dequantize(emb.data, emb.typ, TOKS[pos] * dim, dim)
    tap, aux = {"qtype": {}}, {}
    form = R.Form(defer=hop_free, kv_f16=kv_f16, seq_cap=SEQ)

    def put(name, v, t=None):
        tap[name] = v
        tap["qtype"][name] = o.F32 if t is None else t

    def out_planes(xv, wn, eps, deferred):
        """what a wo / ffn_down launch leaves for its consumer: (planes, rsums)"""
        if deferred:
            x64 = xv.astype(np.float64).reshape(-1, 32)
            return o.quantize(xv * wn, o.Q8_0), (x64 * x64).sum(axis=1).astype(np.float32)
        return o.quantize(exact_norm(xv, wn, eps, odev), qt), None

    planes, rsums = out_planes(x, f32w("blk.0.attn_norm.weight"), s.rms_eps, False)
    for l in range(L):
        deferred_in = hop_free and l > 0
        inv = f32_inv_rms(rsums, dim, s.rms_eps) if deferred_in else np.float32(1.0)
        rec = l == layer
        if rec:
            put("qkv_in.x", x.copy())
            put("qkv_in.act_dim", planes.copy(), qt)
            if rsums is not None:
                put("qkv_in.rsums", rsums.copy())
        lin = {}
        for nm, wn_ in (("q", "attn_q"), ("k", "attn_k"), ("v", "attn_v")):
            raw = mv(model.tensors[f"blk.{l}.{wn_}.weight"], planes)
            v = raw * inv if deferred_in else raw
            if qwen2:
                v = v + f32w(f"blk.{l}.{wn_}.bias")
            lin[nm], lin[nm + "_raw"] = v, raw
        q = rope(lin["q"], s.n_heads, hd, pos, rope_dim, qwen2, odev) * (np.float32(1.0) / np.sqrt(np.float32(hd)))
        k = rope(lin["k"], s.n_kv_heads, hd, pos, rope_dim, qwen2, odev)
        for cache, rows in ((kcs[l], k), (vcs[l], lin["v"])):
            cache[:, pos, :] = (o.f32_to_f16_bits(rows) if kv_f16 else rows).reshape(s.n_kv_heads, hd)
        attn = R.oracle_attention(q, kcs[l], vcs[l], s.n_heads, s.n_kv_heads, hd, SEQ, pos, kv_f16)
        act_attn = o.quantize(attn, qt)
        wo_dot = mv(model.tensors[f"blk.{l}.attn_output.weight"], act_attn)
        x1 = wo_dot + x
        planes1, rsums1 = out_planes(x1, f32w(f"blk.{l}.ffn_norm.weight"), 1e-5, hop_free)
        inv1 = f32_inv_rms(rsums1, dim, 1e-5) if hop_free else np.float32(1.0)
        g_raw, u_raw = mv(model.tensors[f"blk.{l}.ffn_gate.weight"], planes1), mv(model.tensors[f"blk.{l}.ffn_up.weight"], planes1)
        h = silu_mul(g_raw * inv1, u_raw * inv1, odev) if hop_free else silu_mul(g_raw, u_raw, odev)
        act_hid = o.quantize(h, qt)
        down_dot = mv(model.tensors[f"blk.{l}.ffn_down.weight"], act_hid)
        x2 = down_dot + x1
        wnext = f32w(f"blk.{l + 1}.attn_norm.weight" if l + 1 < L else "output_norm.weight")
        planes2, rsums2 = out_planes(x2, wnext, s.rms_eps, hop_free and l + 1 < L)
        if rec:
            put("qkv.qbuf", q.copy())
            put("attn.attn", attn.copy())
            put("attn.act_attn", act_attn, qt)
            put("wo.x", x1.copy())
            put("wo.act_dim", planes1, qt)
            if rsums1 is not None:
                put("wo.rsums", rsums1)
            put("gateup.act_hid", act_hid, qt)
            put("down.x", x2.copy())
            put("down.act_dim", planes2, qt)
            if rsums2 is not None:
                put("down.rsums", rsums2)
            aux.update(lin=lin, inv=inv, inv1=inv1, g_raw=g_raw, u_raw=u_raw, h=h, wo_dot=wo_dot, rsums_in=rsums, rsums1=rsums1, odev=odev,
                       kc=kcs[l], vc=vcs[l])
        x, planes, rsums = x2, planes2, rsums2
    put("cls.act", planes, qt)
    put("logits", mv(model.tensors["output.weight"], planes))
    return tap, aux["kc"], aux["vc"], form, aux


# ---- the mutations: each changes its copy of the case and returns the launch that must now fail, or None where it does not apply ----
def _hid_intervals(c):
    lo, hi, ref = R.gateup_reference(c.tap, c.model, c.layer, c.form)
    return R.QuantIntervals(lo, hi, ref, c.tap["qtype"]["gateup.act_hid"])


def _hid_blocks(c):
    qt = c.tap["qtype"]["gateup.act_hid"]
    bb = synth.BLOCK_BYTES[qt]
    return c.tap["gateup.act_hid"].copy().reshape(-1, bb), bb - 32


def m_hid_quant_moved(c):
    iv = _hid_intervals(c)
    b, off = _hid_blocks(c)
    bi, ei = np.argwhere(~iv.excused)[0]
    q = b[bi, off + ei].view(np.int8)
    b[bi, off + ei] = np.int8(q - 1 if q > 0 else q + 1).view(np.uint8)
    c.tap["gateup.act_hid"] = b.reshape(-1)
    return "gate|up"


def m_hid_scale_code(c):
    iv = _hid_intervals(c)
    b, _ = _hid_blocks(c)
    bi = int(np.flatnonzero(iv.single_code)[0])
    d = b[bi, 0:2].copy().view(np.uint16)
    b[bi, 0:2] = (d + 1).view(np.uint8)
    c.tap["gateup.act_hid"] = b.reshape(-1)
    return "gate|up"


def m_hid_s_code(c):  # Q8_1 planes: one block's s moved by one f16 code
    if c.tap["qtype"]["gateup.act_hid"] != o.Q8_1:
        return None
    iv = _hid_intervals(c)
    b, _ = _hid_blocks(c)
    lo, hi = iv.s_interval(R.parse_act(c.tap["gateup.act_hid"], o.Q8_1))
    bi = int(np.flatnonzero(lo == hi)[0])  # a block whose s the reference pins to one code
    sb = b[bi, 2:4].copy().view(np.uint16)
    b[bi, 2:4] = (sb + 1).view(np.uint8)
    c.tap["gateup.act_hid"] = b.reshape(-1)
    return "gate|up"


def m_hid_round_to_nearest(c):
    b, off = _hid_blocks(c)
    h = c.aux["h"].reshape(-1, 32)
    for bi in range(h.shape[0]):
        dd = np.float32(np.max(np.abs(h[bi]))) / np.float32(127.0)
        q = np.rint(h[bi] / dd).astype(np.int8)
        if not np.array_equal(q.view(np.uint8), b[bi, off:]):
            b[bi, off:] = q.view(np.uint8)
            break
    c.tap["gateup.act_hid"] = b.reshape(-1)
    return "gate|up"


def _act(c, name):
    return R.parse_act(c.tap[name], c.tap["qtype"][name])


def m_drop_block_v(c):
    s = c.model.shape
    e, _ = R.row_dots(c.model.tensors[f"blk.{c.layer}.attn_v.weight"], _act(c, "qkv_in.act_dim"), drop_last_block=True)
    v = e.astype(np.float32) * (c.aux["inv"] if c.form.defer and c.layer > 0 else np.float32(1.0))
    if s.arch == "qwen2":
        v = v + np.ascontiguousarray(c.model.tensors[f"blk.{c.layer}.attn_v.bias"].data).view(np.float32)
    c.vc = c.vc.copy()
    c.vc[:, c.pos, :] = (o.f32_to_f16_bits(v) if c.form.kv_f16 else v).reshape(s.n_kv_heads, s.head_dim)
    return "q|k|v"


def m_drop_block_wo(c):
    e, _ = R.row_dots(c.model.tensors[f"blk.{c.layer}.attn_output.weight"], _act(c, "attn.act_attn"), drop_last_block=True)
    c.tap["wo.x"] = e.astype(np.float32) + c.tap["qkv_in.x"]
    return "wo"


def m_drop_block_gateup(c):
    act = _act(c, "wo.act_dim")
    g, _ = R.row_dots(c.model.tensors[f"blk.{c.layer}.ffn_gate.weight"], act, drop_last_block=True)
    u, _ = R.row_dots(c.model.tensors[f"blk.{c.layer}.ffn_up.weight"], act, drop_last_block=True)
    inv1 = c.aux["inv1"]
    c.tap["gateup.act_hid"] = o.quantize(silu_mul(g.astype(np.float32) * inv1, u.astype(np.float32) * inv1, c.aux["odev"]), c.tap["qtype"]["gateup.act_hid"])
    return "gate|up"


def m_drop_block_down(c):
    e, _ = R.row_dots(c.model.tensors[f"blk.{c.layer}.ffn_down.weight"], _act(c, "gateup.act_hid"), drop_last_block=True)
    c.tap["down.x"] = e.astype(np.float32) + c.tap["wo.x"]
    return "ffn_down"


def m_drop_block_classifier(c):
    e, _ = R.row_dots(c.model.tensors["output.weight"], _act(c, "cls.act"), drop_last_block=True)
    c.tap["logits"] = e.astype(np.float32)
    return "classifier"


def _q_from(c, qlin, pos=None, neox=None):
    s = c.model.shape
    rope_dim = s.rope_dim if s.rope_dim is not None else s.head_dim
    neox = (s.arch == "qwen2") if neox is None else neox
    return rope(qlin, s.n_heads, s.head_dim, c.pos if pos is None else pos, rope_dim, neox, c.aux["odev"]) * (np.float32(1.0) / np.sqrt(np.float32(s.head_dim)))


def _gateup_with_inv(c, inv1):
    c.tap["gateup.act_hid"] = o.quantize(silu_mul(c.aux["g_raw"] * inv1, c.aux["u_raw"] * inv1, c.aux["odev"]), c.tap["qtype"]["gateup.act_hid"])


def _q_with_inv(c, inv):
    v = c.aux["lin"]["q_raw"] * inv
    if c.model.shape.arch == "qwen2":
        v = v + np.ascontiguousarray(c.model.tensors[f"blk.{c.layer}.attn_q.bias"].data).view(np.float32)
    c.tap["qkv.qbuf"] = _q_from(c, v)


def m_inv_rms_gateup_1e4(c):
    if not c.form.defer:
        return None
    _gateup_with_inv(c, c.aux["inv1"] * np.float32(1.0 + 1e-4))
    return "gate|up"


def m_inv_rms_qkv_1e4(c):
    if not (c.form.defer and c.layer > 0):
        return None
    _q_with_inv(c, c.aux["inv"] * np.float32(1.0 + 1e-4))
    return "q|k|v"


# The wrong eps moves 1 / rms by 0.5 * 9e-6 / (mean square of x + eps): 1.3e-5 at the smallest mean square of the plain synthetic
# models (0.35: layer 0 of 15m Q4_0), one f32 ulp near 40, nothing from ~75 on (most layer-1 rows).  Both mutations are applied to
# EVERY model and must be rejected, except where this test itself verifies that the mutated output is one the reference alone
# admits -- where no function of the launch's bytes could tell the wrong kernel from a right one that adds in another order:
#   * the two f32 values of 1 / rms are the same bits;
#   * gate | up (its output exists only as quantized rows, whose levels do not move with a common factor): every byte that changed
#     is a quant the interval check excuses from the reference alone, or the scale of a block whose interval holds two f16 codes;
#   * q | k | v: no row of q moved by more than twice its own re-association bound (the right value may lie anywhere inside the
#     bound, so a value within twice the bound of it cannot be excluded).
# The shrunk twin (R.shrink_residual) is the case where none of these can hold: there the rejection is unconditional.
def m_eps_gateup(c):  # RmsTail handed 1e-6 for the literal 1e-5
    if not c.form.defer:
        return None
    wrong = f32_inv_rms(c.aux["rsums1"], c.model.shape.dim, 1e-6)
    if wrong == c.aux["inv1"]:
        assert not c.small
        return None
    iv = _hid_intervals(c)
    before, _ = _hid_blocks(c)
    _gateup_with_inv(c, wrong)
    after, off = _hid_blocks(c)
    dq = before[:, off:] != after[:, off:]
    dd = np.any(before[:, :off] != after[:, :off], axis=1)
    if not np.any(dq & ~iv.excused) and not np.any(dd & iv.single_code):
        assert not c.small
        return None
    return "gate|up"


def m_eps_qkv(c):  # the other of (1e-5, 1e-6) for the model's rms_norm_eps
    if not (c.form.defer and c.layer > 0):
        return None
    other = 1e-6 if abs(c.model.shape.rms_eps - 1e-5) < 1e-9 else 1e-5
    wrong = f32_inv_rms(c.aux["rsums_in"], c.model.shape.dim, other)
    if wrong == c.aux["inv"]:
        assert not c.small
        return None
    right = c.tap["qkv.qbuf"]
    _, bound = R.qkv_reference(c.tap, c.model, c.layer, c.pos, c.form)["q"]
    _q_with_inv(c, wrong)
    if np.all(np.abs(c.tap["qkv.qbuf"].astype(np.float64) - right) <= 2 * bound):
        assert not c.small
        return None
    return "q|k|v"


def m_rope_next_pos(c):
    c.tap["qkv.qbuf"] = _q_from(c, c.aux["lin"]["q"], pos=c.pos + 1)
    return "q|k|v"


def m_rope_adjacent_pairs(c):
    if c.model.shape.arch != "qwen2" or c.pos == 0:  # (at position 0 every rotation is the identity)
        return None
    c.tap["qkv.qbuf"] = _q_from(c, c.aux["lin"]["q"], neox=False)
    return "q|k|v"


def m_bias_before_multiply(c):
    if not (c.model.shape.arch == "qwen2" and c.form.defer and c.layer > 0):
        return None
    b = np.ascontiguousarray(c.model.tensors[f"blk.{c.layer}.attn_q.bias"].data).view(np.float32)
    c.tap["qkv.qbuf"] = _q_from(c, (c.aux["lin"]["q_raw"] + b) * c.aux["inv"])
    return "q|k|v"


def m_no_residual(c):
    c.tap["wo.x"] = c.aux["wo_dot"].copy()
    return "wo"


def m_wrong_kv_head(c):
    s = c.model.shape
    if s.n_kv_heads in (1, s.n_heads):
        return None
    # head h reads kv head h % n_kv instead of h / group -- with an f32 cache the other way round: the reference's f32 batch_matmul
    # itself takes rhs batch h % n_kv (batch_matmul_naive_f32), which the fast step reproduces
    idx = np.arange(s.n_heads) % s.n_kv_heads if c.form.kv_f16 else np.arange(s.n_heads) // (s.n_heads // s.n_kv_heads)
    attn = R.oracle_attention(c.tap["qkv.qbuf"], c.kc[idx], c.vc[idx], s.n_heads, s.n_heads, s.head_dim, SEQ, c.pos, c.form.kv_f16)
    c.tap["attn.attn"] = attn
    c.tap["attn.act_attn"] = o.quantize(attn, c.tap["qtype"]["attn.act_attn"])
    return "attention"


def m_rsums_chunk(c):
    if not c.form.defer:
        return None
    r = c.tap["wo.rsums"].copy()
    r[3] = np.float32(r[3] * np.float32(1.0 + 1e-5))
    c.tap["wo.rsums"] = r
    return "wo"


MUTATIONS = [m_hid_quant_moved, m_hid_scale_code, m_hid_s_code, m_hid_round_to_nearest, m_drop_block_v, m_drop_block_wo, m_drop_block_gateup,
             m_drop_block_down, m_drop_block_classifier, m_inv_rms_gateup_1e4, m_inv_rms_qkv_1e4, m_eps_gateup, m_eps_qkv, m_rope_next_pos,
             m_rope_adjacent_pairs, m_bias_before_multiply, m_no_residual, m_wrong_kv_head, m_rsums_chunk]


class Case:
    def __init__(self, model, layer, pos, tap, kc, vc, form, aux, small):
        self.model, self.layer, self.pos, self.tap, self.kc, self.vc, self.form, self.aux = model, layer, pos, tap, kc, vc, form, aux
        self.small = small

    def fork(self):
        c = copy.copy(self)
        c.tap = dict(self.tap)
        return c


CHECK = {"q|k|v": lambda c, ctx: R.check_qkv(c.tap, c.kc, c.vc, c.model, c.layer, c.pos, c.form, ctx),
         "attention": lambda c, ctx: R.check_attention(c.tap, c.kc, c.vc, c.model, c.layer, c.pos, c.form, ctx),
         "wo": lambda c, ctx: R.check_gemv_out(c.tap, c.model, c.layer, "wo", c.form, ctx),
         "gate|up": lambda c, ctx: R.check_gateup(c.tap, c.model, c.layer, c.form, ctx),
         "ffn_down": lambda c, ctx: R.check_gemv_out(c.tap, c.model, c.layer, "down", c.form, ctx),
         "classifier": lambda c, ctx: R.check_classifier(c.tap, c.model, ctx)}


@pytest.mark.parametrize("pos", [0, 7])
@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0", "Q4_1"])
@pytest.mark.parametrize("shape", ["15m", "tiny-gqa", "tiny-hd128", "tiny-qwen2"])
def test_checker_accepts_the_oracle_step_and_rejects_every_mutation(oracle, shape, fmt, pos):
    plain = synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=21, n_layers=2)
    shrunk = R.shrink_residual(synth.build_model(synth.SHAPES[shape], synth.TYPE_BY_NAME[fmt], seed=21, n_layers=2))
    applied = set()
    forms = [(plain, False, False)] + ([(plain, True, False), (shrunk, True, True)] if fmt != "Q4_1" else [])  # Q4_1 has no hop-free form
    for model, hop_free, small in forms:
        for layer in (0, 1):
            kv_f16 = (pos + layer) % 2 == 0
            ctx = f"{shape}{' (shrunk residual)' if small else ''} {fmt} {'hop-free' if hop_free else 'exact-norm'} kv_f16={kv_f16} layer {layer} pos {pos}"
            tap, kc, vc, form, aux = oracle_tap(model, pos, layer, kv_f16, hop_free)
            res = R.check_layer(tap, kc, vc, model, layer, pos, form, ctx)
            assert not R.failures(res), R.failures(res)
            for r in res.values():
                for name, share in r.excused.items():
                    assert share <= R.EXCUSED_CAP, (ctx, r.launch, name, share)
            base = Case(model, layer, pos, tap, kc, vc, form, aux, small)
            for m in MUTATIONS:
                c = base.fork()
                launch = m(c)
                if launch is None:
                    continue
                applied.add(m.__name__)
                got = CHECK[launch](c, ctx)
                assert got.fails, f"{ctx}: the checker let {m.__name__} through at {launch} (worst error / bound {got.worst:.3g}, excused {got.excused})"
    # every mutation was exercised on this model, except those that need what the model does not have
    skipped = {m.__name__ for m in MUTATIONS} - applied
    allowed = set()
    if synth.SHAPES[shape].arch != "qwen2":
        allowed |= {"m_rope_adjacent_pairs", "m_bias_before_multiply"}
    if synth.SHAPES[shape].n_kv_heads == synth.SHAPES[shape].n_heads:
        allowed |= {"m_wrong_kv_head"}
    if fmt != "Q4_1":
        allowed |= {"m_hid_s_code"}
    if fmt == "Q4_1":
        allowed |= {"m_inv_rms_gateup_1e4", "m_inv_rms_qkv_1e4", "m_eps_gateup", "m_eps_qkv", "m_bias_before_multiply", "m_rsums_chunk"}
    if pos == 0:
        allowed |= {"m_rope_adjacent_pairs"}
    assert skipped <= allowed, skipped  # (the eps mutations are always applied at least on the shrunk twin)


def test_q6_k_rows_of_the_restatement_equal_the_reference_dequantizer(oracle):
    """weight_rows' Q6_K element order (the classifier of a Q4_0 body in llama.cpp's files) against the oracle's dequantize"""
    rng = np.random.default_rng(3)
    raw = synth.random_blocks(rng, 8 * 512, synth.Q6_K)
    w = R.weight_rows(synth.RawTensor(raw, [8, 512], synth.Q6_K), 0, 8)
    mine = (w["q"] * w["d"][:, :, None]).reshape(-1)
    assert np.array_equal(mine.astype(np.float32), o.dequantize(raw, o.Q6_K))


def test_exp_table_is_monotone(oracle):
    """silu_mul_interval spans the hull over a range of f16 codes by the table values at its two ends"""
    t = R.exp_table()
    v = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float64)
    fin = np.isfinite(v)
    tv = t[fin][np.argsort(v[fin], kind="stable")]
    assert np.all(np.diff(tv[np.isfinite(tv)]) >= 0)
