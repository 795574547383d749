"""The checker of a Gemma context's fast fused launches (tests/gemma_step_ref.py) decides what tests/test_hip_gemma.py can see, so it
is tested first, without a device -- the way tests/test_fused_step_ref.py tests fused_step_ref.

A tap is built from the ORACLE: one token step of forward_gemma walked launch by launch with the reference's own ops (its quantizer,
its scalar vec_dot per row, NEOX rope, attention, the GELU lookup), in the exact-norm form and -- by the kernels' stated expression --
in the hop-free form.  The checker must ACCEPT both, leave at most EXCUSED_CAP of any plane's elements excused FROM THE REFERENCE ALONE,
and REJECT every mutation below: each is a Gemma kernel wrong in exactly one way."""
import copy

import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests import gemma_step_ref as G
from tests.gemma_ref import OracleGemmaRunner, to_oracle_gemma
from tests.test_fused_step_ref import _ot, exact_norm, f32_inv_rms, mv, rope, silu_mul

SEQ = 16
TOKS = [1, 365, 400, 282, 7, 9, 11, 13]
SEED = 21


def gelu_mul(g, u, odev):
    return _ot(g, odev).gelu_inplace().mul_inplace(_ot(u, odev)).export()


def oracle_tap(model, pos, layer, kv_f16, hop_free):
    """(tap, kc_raw, vc_raw, form, aux) of one forward_gemma token step at `pos` with `layer` tapped, from the oracle's ops"""
    s = model.shape
    odev = o.OracleDevice(thread_num=1)
    runner = OracleGemmaRunner(*to_oracle_gemma(model, odev), odev, SEQ, kv_f16)
    for i in range(pos):
        runner.forward_llama([TOKS[i]], i)
    kdt = np.uint16 if kv_f16 else np.float32
    kcs = [np.array(c.storage, dtype=kdt).reshape(s.n_kv_heads, SEQ, s.head_dim) for c in runner.key_cache]
    vcs = [np.array(c.storage, dtype=kdt).reshape(s.n_kv_heads, SEQ, s.head_dim) for c in runner.value_cache]
    qt = o.rhs_dtype(model.wtype)
    dim, hd, L = s.dim, s.head_dim, s.n_layers
    rope_dim = s.rope_dim if s.rope_dim is not None else hd
    f32w = lambda n: np.ascontiguousarray(model.tensors[n].data).view(np.float32)  # noqa: E731
    emb = model.tensors["token_embd.weight"]
    x = _ot(o.dequantize(emb.data, emb.typ, TOKS[pos] * dim, dim), odev).scale_inplace(np.sqrt(np.float32(dim))).export()
    tap, aux = {"qtype": {}}, {}
    form = R.Form(defer=hop_free, kv_f16=kv_f16, seq_cap=SEQ)

    def put(name, v, t=None):
        tap[name] = v
        tap["qtype"][name] = o.F32 if t is None else t

    def out_planes(xv, wn, eps, deferred):
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
            lin[nm], lin[nm + "_raw"] = (raw * inv if deferred_in else raw), raw
        q = rope(lin["q"], s.n_heads, hd, pos, rope_dim, True, odev) * (np.float32(1.0) / np.sqrt(np.float32(hd)))
        k = rope(lin["k"], s.n_kv_heads, hd, pos, rope_dim, True, odev)
        for cache, rows in ((kcs[l], k), (vcs[l], lin["v"])):
            cache[:, pos, :] = (o.f32_to_f16_bits(rows) if kv_f16 else rows).reshape(s.n_kv_heads, hd)
        attn = R.oracle_attention(q, kcs[l], vcs[l], s.n_heads, s.n_kv_heads, hd, SEQ, pos, kv_f16)
        act_attn = o.quantize(attn, qt)
        x1 = mv(model.tensors[f"blk.{l}.attn_output.weight"], act_attn) + x
        planes1, rsums1 = out_planes(x1, f32w(f"blk.{l}.ffn_norm.weight"), 1e-5, hop_free)
        inv1 = f32_inv_rms(rsums1, dim, 1e-5) if hop_free else np.float32(1.0)
        g_raw, u_raw = mv(model.tensors[f"blk.{l}.ffn_gate.weight"], planes1), mv(model.tensors[f"blk.{l}.ffn_up.weight"], planes1)
        h = gelu_mul(g_raw * inv1, u_raw * inv1, odev) if hop_free else gelu_mul(g_raw, u_raw, odev)
        act_hid = o.quantize(h, qt)
        x2 = mv(model.tensors[f"blk.{l}.ffn_down.weight"], act_hid) + x1
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
            aux.update(lin=lin, inv=inv, inv1=inv1, g_raw=g_raw, u_raw=u_raw, h=h, odev=odev, kc=kcs[l], vc=vcs[l])
        x, planes, rsums = x2, planes2, rsums2
    put("cls.act", planes, qt)
    put("logits", mv(model.tensors["token_embd.weight"], planes))  # tied (llama2.rs:203-207)
    return tap, aux["kc"], aux["vc"], form, aux


# ---- the mutations: each changes its copy of the case and returns the launch that must now fail, or None where it does not apply ----
def m_embed_not_scaled(c):
    if c.layer != 0:
        return None
    emb = c.model.tensors["token_embd.weight"]
    c.tap["qkv_in.x"] = o.dequantize(emb.data, emb.typ, TOKS[c.pos] * c.model.shape.dim, c.model.shape.dim)
    return "embed"


def m_embed_scale_in_f64(c):
    """the product formed in double and rounded once differs from the f32 product in some element: here the scale factor itself is
    sqrt(dim) in double (22.627416997969522 for 512) instead of the f32 sqrtf"""
    if c.layer != 0:
        return None
    s = c.model.shape
    emb = c.model.tensors["token_embd.weight"]
    row = o.dequantize(emb.data, emb.typ, TOKS[c.pos] * s.dim, s.dim).astype(np.float64)
    x = (row * np.sqrt(np.float64(s.dim))).astype(np.float32)
    if np.array_equal(x, G.embed_reference(c.model, TOKS[c.pos])):
        return None  # (dim a power of 4: the two factors agree)
    c.tap["qkv_in.x"] = x
    return "embed"


def _requant_hid(c, h):
    c.tap["gateup.act_hid"] = o.quantize(np.ascontiguousarray(h, dtype=np.float32), c.tap["qtype"]["gateup.act_hid"])
    return "gate|up"


def m_silu_for_gelu(c):
    return _requant_hid(c, silu_mul(c.aux["g_raw"] * c.aux["inv1"], c.aux["u_raw"] * c.aux["inv1"], c.aux["odev"]))


def m_gelu_of_f32_argument(c):
    """GELU evaluated on the f32 argument (tanh form, gelu.rs:19-22) instead of the f16 table lookup"""
    g = (c.aux["g_raw"] * c.aux["inv1"]).astype(np.float64)
    ge = 0.5 * g * (1.0 + np.tanh(0.7978845608028654 * g * (1.0 + 0.044715 * g * g)))
    return _requant_hid(c, (ge * (c.aux["u_raw"] * c.aux["inv1"]).astype(np.float64)).astype(np.float32))


def m_gelu_of_up(c):  # the activation applied to the wrong operand
    return _requant_hid(c, gelu_mul(c.aux["u_raw"] * c.aux["inv1"], c.aux["g_raw"] * c.aux["inv1"], c.aux["odev"]))


def m_hid_quant_moved(c):
    lo, hi, ref = G.gateup_reference(c.tap, c.model, c.layer, c.form)
    iv = R.QuantIntervals(lo, hi, ref, c.tap["qtype"]["gateup.act_hid"])
    bb = synth.BLOCK_BYTES[c.tap["qtype"]["gateup.act_hid"]]
    b = c.tap["gateup.act_hid"].copy().reshape(-1, bb)
    bi, ei = np.argwhere(~iv.excused)[0]
    q = b[bi, bb - 32 + ei].view(np.int8)
    b[bi, bb - 32 + ei] = np.int8(q - 1 if q > 0 else q + 1).view(np.uint8)
    c.tap["gateup.act_hid"] = b.reshape(-1)
    return "gate|up"


def m_drop_block_gateup(c):
    act = R.parse_act(c.tap["wo.act_dim"], c.tap["qtype"]["wo.act_dim"])
    g, _ = R.row_dots(c.model.tensors[f"blk.{c.layer}.ffn_gate.weight"], act, drop_last_block=True)
    u, _ = R.row_dots(c.model.tensors[f"blk.{c.layer}.ffn_up.weight"], act, drop_last_block=True)
    return _requant_hid(c, gelu_mul(g.astype(np.float32) * c.aux["inv1"], u.astype(np.float32) * c.aux["inv1"], c.aux["odev"]))


def _q_from(c, qlin, pos=None, neox=True):
    s = c.model.shape
    rope_dim = s.rope_dim if s.rope_dim is not None else s.head_dim
    return rope(qlin, s.n_heads, s.head_dim, c.pos if pos is None else pos, rope_dim, neox, c.aux["odev"]) * (np.float32(1.0) / np.sqrt(np.float32(s.head_dim)))


def m_rope_adjacent_pairs(c):
    if c.pos == 0:  # (at position 0 every rotation is the identity)
        return None
    c.tap["qkv.qbuf"] = _q_from(c, c.aux["lin"]["q"], neox=False)
    return "q|k|v"


def m_rope_next_pos(c):
    c.tap["qkv.qbuf"] = _q_from(c, c.aux["lin"]["q"], pos=c.pos + 1)
    return "q|k|v"


def m_a_bias_of_ones(c):  # a q|k|v form that adds something: a bias of 1e-3 on q
    c.tap["qkv.qbuf"] = _q_from(c, c.aux["lin"]["q"] + np.float32(1e-3))
    return "q|k|v"


def m_drop_block_v(c):
    s = c.model.shape
    e, _ = R.row_dots(c.model.tensors[f"blk.{c.layer}.attn_v.weight"], R.parse_act(c.tap["qkv_in.act_dim"], c.tap["qtype"]["qkv_in.act_dim"]),
                      drop_last_block=True)
    v = e.astype(np.float32) * (c.aux["inv"] if c.form.defer and c.layer > 0 else np.float32(1.0))
    c.vc = c.vc.copy()
    c.vc[:, c.pos, :] = (o.f32_to_f16_bits(v) if c.form.kv_f16 else v).reshape(s.n_kv_heads, s.head_dim)
    return "q|k|v"


def m_untied_classifier(c):  # the logits of another matrix (ffn rows) where the tied classifier is token_embd
    e, _ = R.row_dots(c.model.tensors["blk.0.ffn_gate.weight"], R.parse_act(c.tap["cls.act"], c.tap["qtype"]["cls.act"]))
    c.tap["logits"] = e.astype(np.float32)[:c.model.shape.vocab]
    return "classifier"


MUTATIONS = [m_embed_not_scaled, m_embed_scale_in_f64, m_silu_for_gelu, m_gelu_of_f32_argument, m_gelu_of_up, m_hid_quant_moved, m_drop_block_gateup,
             m_rope_adjacent_pairs, m_rope_next_pos, m_a_bias_of_ones, m_drop_block_v, m_untied_classifier]


class Case:
    def __init__(self, model, layer, pos, tap, kc, vc, form, aux):
        self.model, self.layer, self.pos, self.tap, self.kc, self.vc, self.form, self.aux = model, layer, pos, tap, kc, vc, form, aux

    def fork(self):
        c = copy.copy(self)
        c.tap = dict(self.tap)
        return c


CHECK = {"embed": lambda c, ctx: G.check_embed(c.tap, c.model, TOKS[c.pos], ctx),
         "q|k|v": lambda c, ctx: G.check_qkv(c.tap, c.kc, c.vc, c.model, c.layer, c.pos, c.form, ctx),
         "gate|up": lambda c, ctx: G.check_gateup(c.tap, c.model, c.layer, c.form, ctx),
         "classifier": lambda c, ctx: R.check_classifier(c.tap, c.model, ctx)}


@pytest.mark.parametrize("pos", [0, 7])
@pytest.mark.parametrize("fmt", ["Q4_0", "Q8_0"])
def test_checker_accepts_the_oracle_gemma_step_and_rejects_every_mutation(oracle, fmt, pos):
    model = synth.build_model(synth.SHAPES["tiny-gemma"], synth.TYPE_BY_NAME[fmt], seed=SEED)
    applied = set()
    for hop_free in (False, True):
        for layer in (0, 1):
            kv_f16 = (pos + layer) % 2 == 0
            ctx = f"tiny-gemma {fmt} {'hop-free' if hop_free else 'exact-norm'} kv_f16={kv_f16} layer {layer} pos {pos}"
            tap, kc, vc, form, aux = oracle_tap(model, pos, layer, kv_f16, hop_free)
            res = G.check_layer(tap, kc, vc, model, layer, pos, form, ctx, token=TOKS[pos])
            assert not G.failures(res), G.failures(res)
            assert ("embed" in res) == (layer == 0)
            for r in res.values():
                for name, share in r.excused.items():  # from the reference alone
                    print(f"{ctx} {r.launch} {name}: excused share {share:.4f}")
                    assert share <= R.EXCUSED_CAP, (ctx, r.launch, name, share)
            base = Case(model, layer, pos, tap, kc, vc, form, aux)
            for m in MUTATIONS:
                c = base.fork()
                launch = m(c)
                if launch is None:
                    continue
                applied.add(m.__name__)
                got = CHECK[launch](c, ctx)
                assert got.fails, f"{ctx}: the checker let {m.__name__} through at {launch} (worst error / bound {got.worst:.3g}, excused {got.excused})"
    skipped = {m.__name__ for m in MUTATIONS} - applied
    assert skipped <= ({"m_rope_adjacent_pairs"} if pos == 0 else set()), skipped


def test_gelu_table_is_not_monotone_and_the_hull_knows(oracle):
    """The GELU table dips (its minimum, about -0.17, sits near -0.75): an interval of g around the dip has a hull that neither of its
    ends spans, and an interval that straddles 0 covers every subnormal code.  table_hull is the min / max over the whole code range."""
    t = G.gelu_table()
    v = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float64)
    fin = np.isfinite(v)
    order = np.argsort(v[fin], kind="stable")
    assert np.any(np.diff(t[fin][order]) < 0)  # unlike the exp table (tests/test_fused_step_ref.py)
    gmin = v[fin][np.argmin(t[fin])]
    assert -0.8 < gmin < -0.7 and -0.18 < t[fin].min() < -0.16
    lo, hi = G.table_hull(np.array([-1.5, -1e-9, 0.25]), np.array([-0.25, 1e-9, 0.5]))
    ends = t[np.array([-1.5, -0.25], dtype=np.float16).view(np.uint16)]
    assert lo[0] == t[fin].min() and lo[0] < ends.min() and hi[0] == ends.max()
    assert lo[1] <= 0.0 <= hi[1] and hi[1] - lo[1] < 1e-8  # thousands of subnormal codes, all mapping to (+-) tiny values
    brute = t[fin][(v[fin] >= 0.25) & (v[fin] <= 0.5)]
    assert lo[2] == brute.min() and hi[2] == brute.max()
    # the interval product: u of either sign, the dip inside
    l2, h2, ref = G.gelu_mul_interval(np.array([-0.75, -0.75]), np.array([0.3, 0.3]), np.array([2.0, -2.0]), np.array([0.0, 0.0]))
    assert l2[0] <= ref[0] <= h2[0] and l2[1] <= ref[1] <= h2[1]
    assert np.isclose(l2[0], 2.0 * t[fin].min(), rtol=1e-6) and np.isclose(h2[1], -2.0 * t[fin].min(), rtol=1e-6)


def test_value_order_is_the_order_of_the_values():
    codes = np.arange(65536, dtype=np.uint16)
    v = codes.view(np.float16).astype(np.float64)
    fin = np.isfinite(v)
    rank = G.value_order(codes)
    assert sorted(rank.tolist()) == list(range(65536))
    srt = v[fin][np.argsort(rank[fin])]
    assert np.all(np.diff(srt) >= 0) and G.value_order(np.array([0x8000]))[0] + 1 == G.value_order(np.array([0]))[0]
