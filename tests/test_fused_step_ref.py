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


# ---- the K-quant step (enqueue_segment_k): the checker's K forms ----
K_FORMS = {  # the plan words of a tap: what fused.hip decides from the flags
    "default": dict(norm_epi_k=1, q8k_producers=1, k_norm_in=1, qin=1, qmode_wo=1, qmode_down=2, wo_x_only=1, aq8=0, split_wo=2, split_down=1),
    "no-k-norm-in": dict(norm_epi_k=1, q8k_producers=1, k_norm_in=0, qin=1, qmode_wo=1, qmode_down=2, wo_x_only=0, aq8=0, split_wo=1, split_down=1),
    "no-rhs-prologue": dict(norm_epi_k=1, q8k_producers=0, k_norm_in=0, qin=0, qmode_wo=0, qmode_down=0, wo_x_only=0, aq8=0, split_wo=1, split_down=1),
    "separate-norm": dict(norm_epi_k=0, q8k_producers=0, k_norm_in=0, qin=0, qmode_wo=0, qmode_down=0, wo_x_only=0, aq8=0, split_wo=0, split_down=0),
}


def oracle_tap_k(model, pos, layer, kv_f16, form_name):
    """(tap, kc_raw, vc_raw, form, aux) of one token step of a K-quant body at `pos` with `layer` tapped, from the oracle's ops alone:
    Q8_K / Q8_1 planes from o.quantize, row dots from the reference's scalar vec_dot; the fields a step of the named form stores"""
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
    qt = o.rhs_dtype(model.wtype)
    cls_t = model.tensors["output.weight"]
    cq = o.rhs_dtype(cls_t.typ)
    dim, hd, L = s.dim, s.head_dim, s.n_layers
    rope_dim = s.rope_dim if s.rope_dim is not None else hd
    f32w = lambda n: np.ascontiguousarray(model.tensors[n].data).view(np.float32)
    emb = model.tensors["token_embd.weight"]
    x = o.dequantize(emb.data, emb.typ, TOKS[pos] * dim, dim)
    words = dict(K_FORMS[form_name])
    nepi, qin, qout, x_only = words["norm_epi_k"] == 1, words["qin"] == 1, words["q8k_producers"] == 1, words["wo_x_only"] == 1
    tap, aux = {"qtype": {}, "plan": dict(words, path=2, n_cu=256, attn_variant=0)}, {}
    form = R.Form(defer=False, kv_f16=kv_f16, seq_cap=SEQ)

    def put(name, v, t=None):
        tap[name] = v
        tap["qtype"][name] = o.F32 if t is None else t
        if t == o.Q8_K:
            tap[name + ".qp"] = R.class_major(R.parse_act(v, t)["q"].reshape(-1)).astype(np.int8).view(np.uint8)

    xn = exact_norm(x, f32w("blk.0.attn_norm.weight"), s.rms_eps, odev)
    planes = o.quantize(xn, qt)
    for l in range(L):
        rec = l == layer
        if rec:
            put("qkv_in.x", x.copy())
            put("qkv_in.act_dim", planes.copy(), qt)
            if not nepi or l == 0:
                put("qkv_in.xn", xn.copy())
            tap["plan"]["v_q6k"] = int(model.tensors[f"blk.{l}.attn_v.weight"].typ == synth.Q6_K)
            tap["plan"]["down_q6k"] = int(model.tensors[f"blk.{l}.ffn_down.weight"].typ == synth.Q6_K)
        lin = {}
        for nm, wn_ in (("q", "attn_q"), ("k", "attn_k"), ("v", "attn_v")):
            v = mv(model.tensors[f"blk.{l}.{wn_}.weight"], planes)
            if qwen2:
                v = v + f32w(f"blk.{l}.{wn_}.bias")
            lin[nm] = v
        q = rope(lin["q"], s.n_heads, hd, pos, rope_dim, qwen2, odev) * (np.float32(1.0) / np.sqrt(np.float32(hd)))
        k = rope(lin["k"], s.n_kv_heads, hd, pos, rope_dim, qwen2, odev)
        for cache, rows in ((kcs[l], k), (vcs[l], lin["v"])):
            cache[:, pos, :] = (o.f32_to_f16_bits(rows) if kv_f16 else rows).reshape(s.n_kv_heads, hd)
        attn = R.oracle_attention(q, kcs[l], vcs[l], s.n_heads, s.n_kv_heads, hd, SEQ, pos, kv_f16)
        act_attn = o.quantize(attn, qt)
        wo_dot = mv(model.tensors[f"blk.{l}.attn_output.weight"], act_attn)
        x1 = wo_dot + x
        xn1 = exact_norm(x1, f32w(f"blk.{l}.ffn_norm.weight"), 1e-5, odev)
        planes1 = o.quantize(xn1, qt)
        g_raw, u_raw = mv(model.tensors[f"blk.{l}.ffn_gate.weight"], planes1), mv(model.tensors[f"blk.{l}.ffn_up.weight"], planes1)
        h = silu_mul(g_raw, u_raw, odev)
        act_hid = o.quantize(h, qt)
        x2 = mv(model.tensors[f"blk.{l}.ffn_down.weight"], act_hid) + x1
        last = l + 1 == L
        xn2 = exact_norm(x2, f32w("output_norm.weight" if last else f"blk.{l + 1}.attn_norm.weight"), s.rms_eps, odev)
        planes2 = o.quantize(xn2, cq if last else qt)
        if rec:
            put("qkv.qbuf", q.copy())
            put("attn.attn", attn.copy())
            if words["aq8"] or not qin:
                put("attn.act_attn", act_attn, qt)
            put("wo.x", x1.copy())
            if x_only:
                x64 = x1.astype(np.float64).reshape(-1, 32 // words["split_wo"])
                put("wo.rsums", (x64 * x64).sum(axis=1).astype(np.float32))
            else:
                put("wo.act_dim", planes1, qt)
            if not nepi:
                put("wo.xn", xn1.copy())
            put("gateup.h", h.copy())
            if qout or not qin:
                put("gateup.act_hid", act_hid, qt)
            put("down.x", x2.copy())
            if nepi:
                put("down.act_dim", planes2, qt)
            aux.update(lin=lin, h=h, wo_dot=wo_dot, odev=odev, kc=kcs[l], vc=vcs[l], planes1=planes1, x1=x1, xn2=xn2, g_raw=g_raw, u_raw=u_raw)
        x, xn, planes = x2, xn2, planes2
    put("cls.act", planes, cq)
    if not nepi:
        put("cls.xn", xn.copy())
    put("logits", mv(cls_t, planes))
    twin = None
    if x_only:  # the NO_K_NORM_IN twin: the same step, its wo leaves the planes
        twin = {"plan": dict(tap["plan"], wo_x_only=0), "qtype": {"wo.act_dim": qt}, "wo.x": tap["wo.x"].copy(), "wo.act_dim": aux["planes1"],
                "wo.act_dim.qp": R.class_major(R.parse_act(aux["planes1"], qt)["q"].reshape(-1)).astype(np.int8).view(np.uint8)}
    aux["twin"] = twin
    return tap, aux["kc"], aux["vc"], form, aux


# each K mutation changes its copy of the case and returns (the launch that must now fail, a piece of the failure's text), or None
def _planes_name(c, which):
    """the planes the named norm epilogue left, in whichever tap holds them"""
    return (c.twin, "wo.act_dim") if which == "wo" and c.tap["plan"]["wo_x_only"] else (c.tap, which + ".act_dim")


def _set_blocks(holder, name, blocks):
    holder[name] = blocks.reshape(-1)
    holder[name + ".qp"] = R.class_major(R.parse_act(holder[name], o.Q8_K)["q"].reshape(-1)).astype(np.int8).view(np.uint8)


def _fix_bsums(b):
    q = np.ascontiguousarray(b[:, 4:260]).view(np.int8).astype(np.int64)
    b[:, 260:292] = q.reshape(-1, 16, 16).sum(axis=2).astype(np.int16).view(np.uint8).reshape(-1, 32)


def _k_wrong_dot(c, tensor, act_name, f32_name, wrong):
    act = R._rhs(c.tap, act_name, f32_name, o.rhs_dtype(c.model.wtype)) if act_name != "cls.act" else R.tap_act(c.tap, "cls.act")
    return R.row_dots(c.model.tensors[tensor], act, drop_last_block=wrong is True, wrong=None if wrong is True else wrong)[0].astype(np.float32)


def km_drop_v(c):
    s = c.model.shape
    v = R.row_dots(c.model.tensors[f"blk.{c.layer}.attn_v.weight"], R.tap_act(c.tap, "qkv_in.act_dim"), drop_last_block=True)[0].astype(np.float32)
    if s.arch == "qwen2":
        v = v + np.ascontiguousarray(c.model.tensors[f"blk.{c.layer}.attn_v.bias"].data).view(np.float32)
    c.vc = c.vc.copy()
    c.vc[:, c.pos, :] = (o.f32_to_f16_bits(v) if c.form.kv_f16 else v).reshape(s.n_kv_heads, s.head_dim)
    return "q|k|v", "v cache" if c.form.kv_f16 else " v row"


def _km_wo(wrong):
    def m(c):
        if wrong is not True and c.model.tensors[f"blk.{c.layer}.attn_output.weight"].typ != synth.Q4_K:
            return None
        c.tap["wo.x"] = _k_wrong_dot(c, f"blk.{c.layer}.attn_output.weight", "attn.act_attn", "attn.attn", wrong) + c.tap["qkv_in.x"]
        return "wo", " x row"
    m.__name__ = f"km_wo_{wrong}"
    return m


def _km_down(wrong):
    def m(c):
        typ = c.model.tensors[f"blk.{c.layer}.ffn_down.weight"].typ
        if wrong is not True and (typ == synth.Q6_K) != (wrong == "q6_scale_shift") or typ == synth.Q4_1 and wrong is not True:
            return None
        c.tap["down.x"] = _k_wrong_dot(c, f"blk.{c.layer}.ffn_down.weight", "gateup.act_hid", "gateup.h", wrong) + c.tap["wo.x"]
        return "ffn_down", " x row"
    m.__name__ = f"km_down_{wrong}"
    return m


def km_drop_gateup(c):
    holder, name = (c.twin, "wo.act_dim") if c.tap["plan"]["wo_x_only"] else (c.tap, "wo.act_dim")
    act = R.tap_act(holder, name)
    g = R.row_dots(c.model.tensors[f"blk.{c.layer}.ffn_gate.weight"], act, drop_last_block=True)[0].astype(np.float32)
    u = R.row_dots(c.model.tensors[f"blk.{c.layer}.ffn_up.weight"], act, drop_last_block=True)[0].astype(np.float32)
    c.tap["gateup.h"] = silu_mul(g, u, c.aux["odev"])
    if "gateup.act_hid" in c.tap:  # (planes consistent with the wrong h: only the h clause may object)
        c.tap["gateup.act_hid"] = o.quantize(c.tap["gateup.h"], c.tap["qtype"]["gateup.act_hid"])
        if c.tap["qtype"]["gateup.act_hid"] == o.Q8_K:
            _set_blocks(c.tap, "gateup.act_hid", c.tap["gateup.act_hid"].reshape(-1, 292))
    return "gate|up", " h row"


def km_drop_classifier(c):
    c.tap["logits"] = _k_wrong_dot(c, "output.weight", "cls.act", None, True)
    return "classifier", "logits row"


def km_classifier_scale_group(c):
    if c.model.tensors["output.weight"].typ != synth.Q6_K:
        return None
    c.tap["logits"] = _k_wrong_dot(c, "output.weight", "cls.act", None, "q6_scale_shift")
    return "classifier", "logits row"


def km_no_residual(c):
    c.tap["wo.x"] = c.aux["wo_dot"].copy()
    return "wo", " x row"


def km_rope_next_pos(c):
    c.tap["qkv.qbuf"] = _q_from(c, c.aux["lin"]["q"], pos=c.pos + 1)
    return "q|k|v", " q row"


def km_wrong_kv_head(c):
    s = c.model.shape
    if s.n_kv_heads in (1, s.n_heads):
        return None
    idx = np.arange(s.n_heads) % s.n_kv_heads if c.form.kv_f16 else np.arange(s.n_heads) // (s.n_heads // s.n_kv_heads)  # (m_wrong_kv_head)
    attn = R.oracle_attention(c.tap["qkv.qbuf"], c.kc[idx], c.vc[idx], s.n_heads, s.n_heads, s.head_dim, SEQ, c.pos, c.form.kv_f16)
    c.tap["attn.attn"] = attn
    if "attn.act_attn" in c.tap:
        c.tap["attn.act_attn"] = o.quantize(attn, c.tap["qtype"]["attn.act_attn"])
        if c.tap["qtype"]["attn.act_attn"] == o.Q8_K:
            _set_blocks(c.tap, "attn.act_attn", c.tap["attn.act_attn"].reshape(-1, 292))
    return "attention", "attn row"


def km_stale_chunk_sum(c):
    if not c.tap["plan"]["wo_x_only"]:
        return None
    r = c.tap["wo.rsums"].copy()
    r[3] = np.float32(r[3] * np.float32(1.0 + 1e-5))
    c.tap["wo.rsums"] = r
    return "wo", "rsums"


def km_qp_in_element_order(c):
    name = "gateup.act_hid" if "gateup.act_hid" in c.tap and c.tap["qtype"]["gateup.act_hid"] == o.Q8_K else None
    if name is None:
        return None
    c.tap[name + ".qp"] = R.parse_act(c.tap[name], o.Q8_K)["q"].reshape(-1).astype(np.int8).view(np.uint8)
    return "gate|up", "class-major"


def km_hid_bsums(c):
    if "gateup.act_hid" not in c.tap or c.tap["qtype"]["gateup.act_hid"] != o.Q8_K:
        return None
    b = c.tap["gateup.act_hid"].copy().reshape(-1, 292)
    b[1, 262:264] = (np.ascontiguousarray(b[1, 262:264]).view(np.int16) + 1).view(np.uint8)
    c.tap["gateup.act_hid"] = b.reshape(-1)
    return "gate|up", "differs from the reference quantizer"


def _epi(c, which):
    """(holder, name, blocks copy, the interval object) of the planes wo's / ffn_down's norm epilogue left; None without the epilogue"""
    if not c.tap["plan"]["norm_epi_k"]:
        return None
    holder, name = _planes_name(c, which)
    L = c.model.shape.n_layers
    f32w = lambda n: np.ascontiguousarray(c.model.tensors[n].data).view(np.float32)
    if which == "wo":
        wn, eps, x = f32w(f"blk.{c.layer}.ffn_norm.weight"), 1e-5, holder["wo.x"]
    else:
        wn, eps, x = f32w("output_norm.weight" if c.layer + 1 == L else f"blk.{c.layer + 1}.attn_norm.weight"), c.model.shape.rms_eps, c.tap["down.x"]
    lo, hi, ref = R.norm_interval(x, wn, eps, c.model.shape.dim)
    return holder, name, holder[name].copy().reshape(-1, 292), R.QuantIntervalsK(lo, hi, ref)


def _km_epi(which, how):
    launch = "gate|up" if which == "wo" else "ffn_down"  # (wo's planes in the NORMIN form are the twin's, looked at by gate | up's check)

    def m(c):
        e = _epi(c, which)
        if e is None:
            return None
        holder, name, b, iv = e
        if holder is c.twin:
            c.twin = dict(c.twin)
            holder = c.twin
        k = iv.cls[float(iv.cls_ref[0])]
        if how == "quant":  # one quant moved by a step where no half-integer excuses it
            bi, ei = np.argwhere(~iv.excused)[0]
            qv = b[bi, 4 + ei].view(np.int8)
            b[bi, 4 + ei] = np.int8(qv - 1 if qv > 0 else qv + 1).view(np.uint8)
            _fix_bsums(b)
            needle = "quant"
        elif how == "d_ulp":  # d one f32 ulp past its interval
            edge = np.float32(k["d_hi"][0])
            if np.float64(edge) <= k["d_hi"][0]:
                edge = np.nextafter(edge, np.float32(np.inf))
            b[0, 0:4] = np.array([edge * np.float32(iv.cls_ref[0])], dtype=np.float32).view(np.uint8)
            needle = "|d| ="
        elif how == "bsums":
            b[0, 260:262] = (np.ascontiguousarray(b[0, 260:262]).view(np.int16) + 1).view(np.uint8)
            needle = "bsums"
        elif how == "sign":  # the maximum taken from a holder of the opposite sign: every quant and d negated
            qv = np.ascontiguousarray(b[0, 4:260]).view(np.int8).astype(np.int64)
            b[0, 4:260] = np.clip(-qv, -128, 127).astype(np.int8).view(np.uint8)
            b[0, 0:4] = (-np.ascontiguousarray(b[0, 0:4]).view(np.float32)).view(np.uint8)
            _fix_bsums(b)
            needle = "has the sign of no element"
        holder[name] = b.reshape(-1)
        if how == "qp":
            holder[name + ".qp"] = R.parse_act(holder[name], o.Q8_K)["q"].reshape(-1).astype(np.int8).view(np.uint8)
            needle = "class-major"
        else:
            holder[name + ".qp"] = R.class_major(R.parse_act(holder[name], o.Q8_K)["q"].reshape(-1)).astype(np.int8).view(np.uint8)
        return ("wo" if which == "wo" and holder is c.tap else launch), needle
    m.__name__ = f"km_epi_{which}_{how}"
    return m


def km_eps_ffn_norm(c):
    """1e-6 for the literal 1e-5 in the ffn norm: the planes gate | up reads, requantized from the wrong norm (the shrunk model only:
    elsewhere the two norms may agree to within the interval)"""
    if not c.small:
        return None
    f32w = np.ascontiguousarray(c.model.tensors[f"blk.{c.layer}.ffn_norm.weight"].data).view(np.float32)
    wrong = o.quantize(exact_norm(c.aux["x1"], f32w, 1e-6, c.aux["odev"]), c.tap["qtype"]["qkv_in.act_dim"])
    g, u = mv(c.model.tensors[f"blk.{c.layer}.ffn_gate.weight"], wrong), mv(c.model.tensors[f"blk.{c.layer}.ffn_up.weight"], wrong)
    c.tap["gateup.h"] = silu_mul(g, u, c.aux["odev"])
    if "gateup.act_hid" in c.tap:
        c.tap["gateup.act_hid"] = o.quantize(c.tap["gateup.h"], c.tap["qtype"]["gateup.act_hid"])
        if c.tap["qtype"]["gateup.act_hid"] == o.Q8_K:
            _set_blocks(c.tap, "gateup.act_hid", c.tap["gateup.act_hid"].reshape(-1, 292))
    return "gate|up", " h row"


K_MUTATIONS = [km_drop_v, _km_wo(True), _km_wo("dmin_plus"), _km_wo("scale_neighbour"), _km_wo("min_neighbour"), km_drop_gateup, _km_down(True),
               _km_down("dmin_plus"), _km_down("q6_scale_shift"), km_drop_classifier, km_classifier_scale_group, km_no_residual, km_rope_next_pos,
               km_wrong_kv_head, km_stale_chunk_sum, km_qp_in_element_order, km_hid_bsums, km_eps_ffn_norm] + \
              [_km_epi(w_, h_) for w_ in ("wo", "down") for h_ in ("quant", "d_ulp", "bsums", "sign", "qp")]


def _k_check(c, launch, ctx):
    return R.check_layer(c.tap, c.kc, c.vc, c.model, c.layer, c.pos, c.form, ctx, twin=c.twin)[launch]


def _k_model(shape, fmt, seed=22):
    s = synth.SHAPES[shape]
    if fmt == "Q4_K":
        return synth.build_model(s, synth.Q4_K, seed=seed, n_layers=2, output_type=synth.Q6_K)
    if fmt == "Q4_K_M":  # two layers: use_more_bits picks layer 1 only, so layer 0 is tapped with Q4_K attn_v / ffn_down and layer 1 with Q6_K
        return synth.build_model(s, synth.Q4_K, seed=seed, n_layers=2, k_m_mix=True)
    return synth.build_model(s, synth.Q4_1, seed=seed, n_layers=2, output_type=synth.Q6_K)


@pytest.mark.parametrize("pos", [0, 7])
@pytest.mark.parametrize("fmt", ["Q4_K", "Q4_K_M", "Q4_1"])
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128", "tiny-qwen2"])
def test_k_checker_accepts_the_oracle_step_and_rejects_every_mutation(oracle, shape, fmt, pos):
    """the K forms of the checker: an oracle-built tap of every form passes, each planted mutation fails in the clause that claims it
    (the failure's text names it), and the excused shares of the Q8_K interval check -- printed -- stay under EXCUSED_CAP"""
    applied, shares = set(), []
    forms = ["separate-norm"] if fmt == "Q4_1" else ["default", "no-k-norm-in", "no-rhs-prologue"] + (["separate-norm"] if fmt == "Q4_K" else [])
    for small in (False, True):
        model = _k_model(shape, fmt)
        if small:
            R.shrink_residual(model)
        for fi, form_name in enumerate(forms):
            for layer in (0, 1):
                kv_f16 = (pos + layer + fi) % 2 == 0
                ctx = f"{shape}{' (shrunk residual)' if small else ''} {fmt} {form_name} kv_f16={kv_f16} layer {layer} pos {pos}"
                tap, kc, vc, form, aux = oracle_tap_k(model, pos, layer, kv_f16, form_name)
                res = R.check_layer(tap, kc, vc, model, layer, pos, form, ctx, twin=aux["twin"])
                assert not R.failures(res), R.failures(res)
                for r in res.values():
                    for name, share in r.excused.items():
                        shares.append(share)
                        assert share <= R.EXCUSED_CAP, (ctx, r.launch, name, share)
                base = Case(model, layer, pos, tap, kc, vc, form, aux, small)
                base.twin, base.tap0 = aux["twin"], tap
                for m in K_MUTATIONS:
                    c = base.fork()
                    c.tap["plan"], c.tap["qtype"] = dict(tap["plan"]), dict(tap["qtype"])
                    hit = m(c)
                    if hit is None:
                        continue
                    launch, needle = hit
                    applied.add(m.__name__)
                    got = _k_check(c, launch, ctx)
                    assert any(needle in f for f in got.fails), \
                        f"{ctx}: the checker let {m.__name__} through at {launch} ({needle!r} not in {got.fails}; worst error / bound {got.worst:.3g})"
    print(f"{shape} {fmt} pos {pos}: excused shares of the Q8_K interval check: max {max(shares, default=0.0):.2e}, mean {np.mean(shares) if shares else 0.0:.2e} "
          f"over {len(shares)} plane sets")
    skipped = {m.__name__ for m in K_MUTATIONS} - applied
    allowed = set()
    if synth.SHAPES[shape].n_kv_heads == synth.SHAPES[shape].n_heads:
        allowed |= {"km_wrong_kv_head"}
    if fmt != "Q4_K_M":
        allowed |= {"km_down_q6_scale_shift"}
    if fmt == "Q4_1":
        allowed |= {m.__name__ for m in K_MUTATIONS if "epi" in m.__name__ or "wo_" in m.__name__ and m.__name__ != "km_wo_True"} | \
                   {"km_down_dmin_plus", "km_stale_chunk_sum", "km_qp_in_element_order", "km_hid_bsums"}
    assert skipped <= allowed, skipped


def test_q4_k_rows_of_the_restatement_equal_the_reference_dequantizer(oracle):
    """weight_rows' Q4_K fields (the 6-bit scale / min unpack, the nibble order) against the oracle's dequantize, in its own f32 steps"""
    rng = np.random.default_rng(4)
    raw = synth.random_blocks(rng, 8 * 512, synth.Q4_K)
    w = R.weight_rows(synth.RawTensor(raw, [8, 512], synth.Q4_K), 0, 8)
    f = np.float32
    d1 = (w["d"].astype(f)[:, :, None] * w["sc"].astype(f))[:, :, :, None]
    m1 = (w["dmin"].astype(f)[:, :, None] * w["mn"].astype(f))[:, :, :, None]
    mine = d1 * w["q"].reshape(8, 2, 8, 32).astype(f) - m1
    assert np.array_equal(mine.reshape(-1), o.dequantize(raw, o.Q4_K))
    assert np.allclose(R.k_values(w).reshape(-1), mine.reshape(-1).astype(np.float64), rtol=1e-6, atol=0)


@pytest.mark.parametrize("typ", [synth.Q4_K, synth.Q6_K])
def test_k_row_dot_bounds_lie_below_the_projects_bound(oracle, typ):
    """the derived bounds (n_terms + C_K) U sum A lie below 8 GEMV_REL sum |w_i x_i| on every row length of the tested shapes (dim 512,
    1792, 4096, 8192; hidden 1024, 14336) -- they are what the K launches are held to; the figures are printed.  The reference's scalar
    vec_dot -- one admissible order -- stays inside the derived bound on every row."""
    from tests.helpers import GEMV_REL
    rng = np.random.default_rng(6)
    for k in (512, 1024, 1792, 4096, 8192, 14336):
        rows = 64
        raw = synth.random_blocks(rng, rows * k, typ)
        t = synth.RawTensor(raw, [rows, k], typ)
        xq = o.quantize((rng.standard_normal(k) * rng.uniform(0.2, 3.0)).astype(np.float32), o.Q8_K)
        act = R.parse_act(xq, o.Q8_K)
        e, b = R.row_dots(t, act)
        w = R.weight_rows(t, 0, rows)
        proj = GEMV_REL * (np.abs(R.k_values(w)) @ np.abs(R.act_values(act)))
        assert np.all(b <= 8 * proj), (k, float(np.max(b / proj)))
        if typ == synth.Q6_K and k // 256 <= 41:  # (8 nsb + C_K <= 335 = GEMV_REL / U and A <= sum |w_i x_i|: below the bound itself)
            assert np.all(b <= proj), (k, float(np.max(b / proj)))
        got = np.array([o.vec_dot(raw.reshape(rows, -1)[r], typ, xq, k) for r in range(rows)], dtype=np.float64)
        assert np.all(np.abs(got - e) <= b), (k, float(np.max(np.abs(got - e) / b)))
        print(f"type {typ} k {k}: derived / project's bound: max {np.max(b / proj):.3f}; the reference's error / derived bound: max {np.max(np.abs(got - e) / b):.3f}")


def test_q8k_intervals_on_planted_ties(oracle):
    """the two clauses a random row never exercises, on planes whose f32 input is stored (the reference's bytes): a product scale * v
    exactly on a half-integer rounds AWAY from zero, and a maximum held by two elements of opposite sign goes to the FIRST one"""
    v = np.zeros(256, dtype=np.float32)
    v[0], v[1], v[2], v[3], v[200] = -2.0, 2.0 * 5 / 256, -2.0 * 7 / 256, 0.3, 2.0  # scale = 64: products 2.5 and -3.5; |v[200]| = |v[0]|
    ref = o.quantize(v, o.Q8_K)
    a = R.parse_act(ref, o.Q8_K)
    assert a["q"][0, 1] == 3 and a["q"][0, 2] == -4 and a["d"][0] > 0, a["q"][0, :4]
    tap = {"qtype": {"gateup.act_hid": o.Q8_K}, "gateup.act_hid": ref}
    res = R.Result("gate|up")
    R.check_quantizer_bytes(res, tap, "gateup.act_hid", v, "ties")
    assert res.ok(), res.fails
    even = ref.copy().reshape(-1, 292)  # round-half-even: 2 and -4
    even[0, 4 + 1] = np.int8(2).view(np.uint8)
    _fix_bsums(even)
    last = ref.copy().reshape(-1, 292)  # the last holder of the maximum: the opposite sign throughout
    last[0, 4:260] = np.clip(-a["q"][0], -128, 127).astype(np.int8).view(np.uint8)
    last[0, 0:4] = np.array([-a["d"][0]], dtype=np.float32).view(np.uint8)
    _fix_bsums(last)
    for wrong in (even, last):
        res = R.Result("gate|up")
        R.check_quantizer_bytes(res, dict(tap, **{"gateup.act_hid": wrong.reshape(-1)}), "gateup.act_hid", v, "ties")
        assert any("differs from the reference quantizer" in f for f in res.fails), res.fails
    # (the interval form cannot tell these: a product on a half-integer and a maximum of either sign are what it excuses)
    iv = R.QuantIntervalsK(v.astype(np.float64), v.astype(np.float64), v.astype(np.float64))
    assert iv.excused[0, 1] and iv.excused[0, 2] and iv.cls[1.0]["ok"][0] and iv.cls[-1.0]["ok"][0]
