"""What the table of tests/weight_formats.py makes possible: ONE model whose layers hold Q2_K, Q3_K, Q4_K, Q5_K and Q6_K tensors side by
side -- no llama.cpp recipe, and no family of tests/weight_formats.FAMILY -- is read by fused_step_ref.check_layer_k as it stands, every
tensor by the row of its own format, and one subtly wrong kernel per format is rejected on that model's rows."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import fused_step_ref as R
from tests import weight_formats as WF
from tests.test_q5k_step_ref import _tap, oracle_tokens

Q2K, Q3K, Q4K, Q5K, Q6K = synth.Q2_K, synth.Q3_K, synth.Q4_K, synth.Q5_K, synth.Q6_K
# a Q2_K body (what a layer does not name stays Q2_K): every one of the five formats in either layer, and among the matrices of either
# kind -- those behind a norm (q, k, v, gate, up) and those that write the residual stream (attn_output, ffn_down)
LAYER_TYPES = {0: {"attn_q": Q3K, "attn_k": Q4K, "attn_v": Q5K, "attn_output": Q6K, "ffn_up": Q4K, "ffn_down": Q3K},
               1: {"attn_q": Q5K, "attn_k": Q6K, "attn_v": Q3K, "attn_output": Q4K, "ffn_gate": Q6K, "ffn_up": Q3K, "ffn_down": Q5K}}
SEED, SEQ, POSITIONS = 61, 64, [0, 5]
# one wrong kernel per format, on a matrix of the model that holds it
WRONG = [(Q2K, "blk.0.ffn_gate.weight", "min_added"), (Q3K, "blk.0.ffn_down.weight", "scale_without_32"), (Q4K, "blk.1.attn_output.weight", "dmin_plus"),
         (Q5K, "blk.1.ffn_down.weight", "fifth_bit_dropped"), (Q6K, "blk.0.attn_output.weight", "offset_dropped")]


@pytest.fixture(scope="module")
def model():
    m = synth.build_model(synth.SHAPES["tiny-gqa"], Q2K, seed=SEED, n_layers=2, layer_types=LAYER_TYPES, output_type=Q6K)
    held = {t.typ for n, t in m.tensors.items() if n.startswith("blk.") and t.typ in WF.FORMATS}
    assert held == {Q2K, Q3K, Q4K, Q5K, Q6K} and m.tensors["output.weight"].typ == Q6K, held
    return m


def test_mixed_k_quant_model_passes_the_k_checker_as_it_stands(oracle, model):
    """the reference's own step over the mixed model passes check_layer_k, and the Q8_K interval check excuses no more than EXCUSED_CAP"""
    shares = []
    with oracle_tokens(SEQ, max(POSITIONS) + 1):
        for pos in POSITIONS:
            for layer in (0, 1):
                tap, kc, vc, form, aux = _tap(model, pos, layer)
                ctx = f"mixed layer {layer} pos {pos}"
                res = R.check_layer_k(tap, kc, vc, model, layer, pos, form, ctx, twin=aux["twin"])
                assert not R.failures(res), R.failures(res)
                for r in res.values():
                    for name, share in r.excused.items():
                        shares.append(share)
                        assert share <= R.EXCUSED_CAP, (ctx, r.launch, name, share)
    assert shares
    print(f"mixed: excused shares of the Q8_K interval check: max {max(shares):.2e} over {len(shares)} plane sets")


@pytest.mark.parametrize("typ,wname,wrong", WRONG, ids=lambda v: v if isinstance(v, str) else synth.TYPE_NAMES[v])
def test_one_wrong_kernel_per_format_is_rejected_on_the_mixed_model(oracle, model, typ, wname, wrong):
    t = model.tensors[wname]
    assert t.typ == typ and wrong in WF.FORMATS[typ].wrong
    rng = np.random.default_rng(7)
    k = t.shape[1]
    act = R.parse_act(o.quantize((rng.standard_normal(k) * rng.uniform(0.2, 3.0)).astype(np.float32), o.Q8_K), o.Q8_K)
    exact, bound = R.row_dots(t, act)
    got, _ = R.row_dots(t, act, wrong=wrong)
    out = np.abs(got.astype(np.float32).astype(np.float64) - exact) > bound
    assert out.mean() > 0.9, (wrong, float(out.mean()))
