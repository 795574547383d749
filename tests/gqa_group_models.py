"""The four two-layer models of the GQA groups 3, 5, 6 and 7 (vocab 1024; every dim a whole number of 256-element super-blocks, so
K-quant bodies load), shared by tests/test_gqa_groups_ref.py (the checker on the oracle's own step, no device) and
tests/test_hip_gqa_groups.py (the device): the seeds the CPU test cleared are the seeds the device cases run."""
from crabml_amd import synth

SHAPES = {
    "tiny-g3": synth.ModelShape("tiny-g3", 768, 1024, 2, 6, 2, 1024, 64, 1e-5, None),
    "tiny-g5": synth.ModelShape("tiny-g5", 1280, 1024, 2, 10, 2, 1024, 64, 1e-5, None),
    "tiny-qwen2-g6": synth.ModelShape("tiny-qwen2-g6", 768, 1024, 2, 12, 2, 1024, 64, 1e-6, None, "qwen2"),
    "tiny-qwen2-g7": synth.SHAPES["tiny-qwen2-g7"],
}
GROUP = {"tiny-g3": 3, "tiny-g5": 5, "tiny-qwen2-g6": 6, "tiny-qwen2-g7": 7}
HEAD_DIM = {"tiny-g3": 128, "tiny-g5": 128, "tiny-qwen2-g6": 64, "tiny-qwen2-g7": 128}
SEED = 81

# (shape, format) of the device's hand-over cases
HANDOVER = [("tiny-g3", "Q4_0"), ("tiny-g5", "Q4_1"), ("tiny-qwen2-g6", "Q4_K"), ("tiny-qwen2-g7", "Q4_0"), ("tiny-qwen2-g7", "Q4_K")]


def build(shape, fmt, seed=SEED, **kw):
    """Q4_K: layers in Q4_K in front of a Q6_K classifier, as llama.cpp's files have it"""
    s = SHAPES[shape]
    assert (s.n_heads // s.n_kv_heads, s.head_dim) == (GROUP[shape], HEAD_DIM[shape])
    if fmt == "Q4_K":
        kw.setdefault("output_type", synth.Q6_K)
    return synth.build_model(s, synth.TYPE_BY_NAME[fmt], seed=seed, **kw)
