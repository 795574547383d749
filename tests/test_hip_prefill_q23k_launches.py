"""The fast prompt pass over Q2_K and Q3_K BODIES: passes of >= 32 rows run every Q2_K / Q3_K matrix on k_gemm_f16w (gemm_f16w.hip:
WF_Q2_K / WF_Q3_K, one B' k-slot order for both), the Q4_K / Q6_K tensors of the recipes on the GEMM they already had, and every Q5_K
matrix on the row-by-row GEMV.

Part 1, every launch of a tapped pass (modelled on tests/test_hip_prefill_k_launches.py, through the same run_case and
tests/prefill_pass_ref.check_pass, which reads the two formats inside q23k_f16w_ref.q23k_pass): plain Q3_K, the Q3_K_S and Q3_K_M
recipes, plain Q2_K, the Q2_K recipe and Q2_K_S, on tiny-gqa (GQA group 4: the Q2_K recipe's attn_v is Q4_K) and tiny-hd128 (group 2:
attn_v is Q3_K).  The launch plan must say k_gemm_f16w for every Q2_K / Q3_K / Q4_K / Q6_K matrix and the GEMV for a Q5_K one, one
launch for q | k | v and for gate | up where the formats agree, and B' re-made for attn_v only where its k-slot order differs from
attn_q's.  Every GEMM output is held to GEMV_REL sum |A' B'| with A' restated by tests/q23k_f16w_ref.py.  Observed error / bound
ratios: tests/golden/prefill_q23k_launch_pins_observed.json (evidence only).

Part 2, end to end against the oracle's token loop, in the form of tests/test_hip_prefill.test_fast_prompt_pass_f16_weight_gemm."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import prefill_pass_ref as P
from tests import q23k_f16w_ref as Q
from tests.helpers import FAST_TOL, record_observed, to_oracle
from tests.test_hip_prefill_k_launches import GEMV, F16W, MATS, NORM_ROWS_K, expect_norm
from tests.test_hip_prefill_launches import INT8_GEMM, POS0_CASES, expect_attn, run_case

pytestmark = pytest.mark.gpu

# body -> build_model's arguments
BODIES = {"Q3_K": (synth.Q3_K, {}), "Q3_K_S": (synth.Q3_K, {"q3_k_mix": "S"}), "Q3_K_M": (synth.Q3_K, {"q3_k_mix": "M"}),
          "Q2_K": (synth.Q2_K, {}), "Q2_K_MIX": (synth.Q2_K, {"q2_k_mix": "K"}), "Q2_K_S": (synth.Q2_K, {"q2_k_mix": "S"})}
ORDER = {synth.Q2_K: 3, synth.Q3_K: 3, synth.Q4_K: 1, synth.Q6_K: 2}  # gemm_f16w_order
WIDE = synth.ModelShape("tiny-wide", 512, 4096, 1, 4, 2, 512, 256, 1e-5, None)
_OBSERVED = {}


def record(key, results):
    _OBSERVED[key] = {"error_over_bound": {k: round(r.worst, 4) for k, r in results.items()},
                      "excused_share": {k: {n: round(v, 4) for n, v in r.excused.items()} for k, r in results.items() if r.excused}}
    record_observed(_OBSERVED, "prefill_q23k_launch_pins.json")


def body_model(shape, body, seed):
    wtype, kw = BODIES[body]
    return synth.build_model(synth.SHAPES[shape] if isinstance(shape, str) else shape, wtype, seed=seed, **kw)


TAP_Q2K_Q3K = 268435456  # CRABML_HIP_LLAMA_PREFILL_TAP_Q2K_Q3K: without it the tap refuses Q2_K / Q3_K bodies (test_tap_is_opt_in)


def case(ca, key, model, seq, n, layers, **kw):
    with Q.q23k_pass():
        return run_case(ca, key, model, seq, kw.pop("kv_f16", True), n, layers, rec=record, flags=kw.pop("flags", 0) | TAP_Q2K_Q3K, **kw)


def test_tap_is_opt_in(ca):
    """the flag only opens the tap: a context without it refuses a Q3_K body as before, and the two contexts' plain passes are equal
    bit for bit"""
    model = body_model("tiny-gqa", "Q3_K", 51)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    toks = [(7 * i + 3) % model.shape.vocab for i in range(40)]
    plain, flagged = ca.HipLlamaRunner(conf, w, dev, 64, True), ca.HipLlamaRunner(conf, w, dev, 64, True, extra_flags=TAP_Q2K_Q3K)
    with pytest.raises(ca.CrabmlError, match=r"ErrorKind\(9\)"):
        plain.debug_prefill_tap(toks, 0)
    assert plain.kv_cache_len() == 0
    assert np.array_equal(np.array(plain.prefill(toks)).view(np.uint32), np.array(flagged.prefill(toks)).view(np.uint32))


def types_of(model, layer):
    return {m: model.tensors[f"blk.{layer}.{nm}.weight"].typ for m, nm in MATS.items()}


def expect_layer(plan, model, layer, n):
    """the default pass from 32 rows over a Q2_K / Q3_K body"""
    assert plan["f16w"] == 1 and plan["recomputed"] == 0, plan
    typ = types_of(model, layer)
    for m, t in typ.items():
        assert t in ORDER or t == synth.Q5_K, (m, t)
        assert plan["kernel_" + m] == (GEMV if t == synth.Q5_K else F16W), (m, plan)
    expect_norm(plan, n)
    one = typ["q"] == typ["k"] == typ["v"]
    assert plan["qkv_one"] == (1 if one else 0) and "n1.xh" in plan["fields"], plan
    # B' for attn_v: made again only where its k-slot order is not the one attn_q and attn_k read
    remade = (not one) and typ["v"] != synth.Q5_K and ORDER[typ["v"]] != ORDER[typ["q"]]
    assert ("n1.xh.v" in plan["fields"]) == remade, (typ, plan)
    assert plan["gu_one"] == 1 and "n2.xh" in plan["fields"], plan
    assert ("attn.xh" in plan["fields"]) == (typ["wo"] != synth.Q5_K) and ("hid.xh" in plan["fields"]) == (typ["down"] != synth.Q5_K), plan


ROWS = {"tiny-gqa": (77, 200), "tiny-hd128": (130, 192)}  # one count below 192 (the separate norm launches) and one from 192 (k_norm_quant_rows_k)


@pytest.mark.parametrize("body", sorted(BODIES))
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hd128"])
def test_default_pass_every_launch(ca, shape, body):
    model = body_model(shape, body, 61)
    remade = 0
    for n in ROWS[shape]:
        plans = case(ca, f"default/{shape}/{body}", model, 256, n, [0, 1])
        for layer, plan in plans.items():
            expect_layer(plan, model, layer, n)
            assert plan["norm_kernel"] == (NORM_ROWS_K if n >= 192 else 0), plan
            assert plan["attn_kernel"] == expect_attn(model, n), plan
            remade += "n1.xh.v" in plan["fields"]
    # the Q2_K recipe on GQA group 4: attn_v is Q4_K, its B' its own; on group 2 it is Q3_K and shares attn_q's
    assert remade == (4 if (shape, body) == ("tiny-gqa", "Q2_K_MIX") else 0), remade
    if body == "Q2_K_MIX" and shape == "tiny-hd128":
        assert all(p["qkv_one"] == 0 for p in plans.values())  # (Q2_K | Q2_K | Q3_K: three launches, one B')


@pytest.mark.parametrize("body", ["Q3_K_M", "Q2_K_MIX"])
def test_pass_that_starts_inside_the_cache(ca, body):
    setup, seq, kv_f16, chunk, alf, n, attn = POS0_CASES["across-the-switch"]
    model = body_model("tiny-gqa", body, 70)
    plans = case(ca, f"pos0/across-the-switch/tiny-gqa/{body}", model, seq, n, [0, 1], kv_f16=kv_f16, setup=setup, chunk=chunk, attn_long_from=alf)
    for layer, plan in plans.items():
        assert plan["pos0"] > 0 and plan["attn_kernel"] == attn, plan
        expect_layer(plan, model, layer, n)


@pytest.mark.parametrize("body", ["Q3_K", "Q2_K"])
def test_k_pieces_left_to_the_norm_launch(ca, body):
    """two layers of the tiny-wide shape (hidden 4096): ffn_down's GEMM of layer 0 (Q3_K, Q2_K) is cut into k pieces whose sum is left
    to layer 1's k_norm_quant_rows_k"""
    model = body_model(synth.ModelShape("tiny-wide", 512, 4096, 2, 4, 2, 512, 256, 1e-5, None), body, 67)
    plans = case(ca, f"k-pieces/tiny-wide/{body}", model, 256, 200, [0, 1])
    assert plans[0]["down_parts"] > 0 and plans[0]["down_ksplit"] == plans[0]["down_parts"] + 1, plans[0]
    assert plans[1]["in_parts"] == plans[0]["down_parts"] and plans[1]["norm_kernel"] == NORM_ROWS_K, plans[1]
    for layer, plan in plans.items():
        expect_layer(plan, model, layer, 200)


@pytest.mark.parametrize("body", ["Q3_K_M", "Q2_K"])
def test_int8_gemm_flag_puts_the_matrices_back_on_the_gemv(ca, body):
    """CRABML_HIP_LLAMA_PREFILL_INT8_GEMM stays the A/B: no B' anywhere, Q2_K / Q3_K / Q5_K matrices row by row, the recipe's Q4_K
    tensors on their int8 matrix-core GEMM"""
    model = body_model("tiny-gqa", body, 65)
    plans = case(ca, f"int8-flag/tiny-gqa/{body}", model, 256, 77, [0, 1], flags=INT8_GEMM, sample=P.Sample(extra=8, col_tile=16))
    for layer, plan in plans.items():
        assert plan["f16w"] == 0 and plan["qkv_one"] == 0 and plan["gu_one"] == 0, plan
        assert not {"n1.xh", "n1.xh.v", "attn.xh", "n2.xh", "hid.xh"} & plan["fields"], plan
        for m, t in types_of(model, layer).items():
            assert plan["kernel_" + m] == (P.KERNEL_INT8 if t in (synth.Q4_K, synth.Q6_K) else GEMV), (m, plan)


@pytest.mark.parametrize("body", ["Q3_K", "Q2_K"])
def test_overflow_recomputation_puts_the_chunk_back_on_the_gemv(ca, body):
    """the massive-channel model of tests/test_hip_prefill_k_launches.test_overflow_recomputation_is_the_int8_pass (two elements of every
    ffn_norm weight x 2^16): B' overflows f16, the chunk is computed again without the f16 GEMM, and the tapped buffers are the
    recomputation's"""
    model = body_model("tiny-gqa", body, 5)
    s = model.shape
    for l in range(s.n_layers):
        t = model.tensors[f"blk.{l}.ffn_norm.weight"]
        w = t.data.view(np.float32).copy()
        w[[3, s.dim // 2 + 1]] *= np.float32(2.0 ** 16)
        t.data = w.view(np.uint8)
    plans = case(ca, f"overflow/tiny-gqa/{body}", model, 80, 64, [0, 1], sample=P.Sample(extra=8, col_tile=16))
    for layer, plan in plans.items():
        assert plan["recomputed"] == 1 and plan["f16w"] == 0 and plan["qkv_F"] == 0, plan
        assert all(plan["kernel_" + m] == GEMV for m in MATS), plan
        assert not {"n1.xh", "n1.xh.v", "attn.xh", "n2.xh", "hid.xh"} & plan["fields"], plan


# ---- end to end ----------------------------------------------------------------------------------------------------------------
PREFILL_INT8_GEMM = INT8_GEMM


@pytest.mark.parametrize("body,shape,n", [("Q3_K", "tiny-gqa", 200), ("Q3_K_M", "tiny-gqa", 200), ("Q2_K", "tiny-gqa", 200),
                                          ("Q2_K_MIX", "tiny-gqa", 200), ("Q3_K", "tiny-hd128", 384), ("Q3_K", "tiny-wide", 40),
                                          ("Q3_K", "tiny-wide", 200), ("Q2_K", "tiny-wide", 40), ("Q2_K", "tiny-wide", 200)])
def test_fast_prompt_pass_f16_weight_gemm(ca, body, shape, n):
    """Against the oracle's token loop the f16 pass sits inside the format's fast tolerance (FAST_TOL[fmt][1]), as the flagged pass
    (the GEMV row by row) does; the two agree inside it and are NOT equal (the flag must change the arithmetic); the greedy continuation
    starts with the same token; the pass is bit-identical run to run (tiny-wide: ffn_down's k pieces are added in a fixed order)."""
    model = body_model(WIDE if shape == "tiny-wide" else shape, body, 91 if shape != "tiny-wide" else 17)
    fmt = synth.TYPE_NAMES[BODIES[body][0]]
    prompt = [(11 * i + 5) % model.shape.vocab for i in range(n)]
    odev = o.OracleDevice(thread_num=8, use_avx2=False)
    oconf, ow = to_oracle(model, odev)
    orr = o.OracleLlamaRunner(oconf, ow, odev, n + 16, True)
    ref = None
    for i, t in enumerate(prompt):
        ref = orr.forward([t], i)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    a = ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=512)
    b = ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=512, extra_flags=PREFILL_INT8_GEMM)
    la, lb = np.array(a.prefill(prompt)), np.array(b.prefill(prompt))
    la2 = np.array(ca.HipLlamaRunner(conf, w, dev, n + 16, True, prefill_chunk=512).prefill(prompt))
    scale = float(np.max(np.abs(ref)))
    ea, eb, eab = (float(np.max(np.abs(x - y))) / scale for x, y in ((la, ref), (lb, ref), (la, lb)))
    tol = FAST_TOL[fmt][1]
    print(f"{shape}/{body}/{n}: f16 vs oracle {ea:.3g}, flagged vs oracle {eb:.3g}, f16 vs flagged {eab:.3g}, bound {tol:.3g}")
    record_observed({f"end-to-end/{shape}/{body}/{n}": {"f16_vs_oracle": ea, "flagged_vs_oracle": eb, "f16_vs_flagged": eab, "bound": tol}},
                    "prefill_q23k_launch_pins.json")
    assert eb <= tol, ("flagged pass vs oracle", eb)
    assert ea <= max(tol, 1.25 * eb), ("f16 pass vs oracle", ea)
    assert eab <= tol, ("f16 pass vs flagged pass", eab)
    assert not np.array_equal(la, lb)  # (equal logits would mean the matrices never left the GEMV)
    assert np.array_equal(la.view(np.uint32), la2.view(np.uint32))
    nxt = int(np.argmax(ref))
    assert list(a.decode_greedy(nxt, 4))[0] == list(b.decode_greedy(nxt, 4))[0]
    assert a.kv_cache_len() == b.kv_cache_len() == n + 4
