"""Which launches a decode context runs -- the table decide_step (crabml_amd/csrc/fused.hip) holds -- on the record-only test device
(CRABML_HIP_FLAG_DRY, armed by CRABML_HIP_TEST_HOOKS=1): shape x weight format x device mode x flag x cache type through
crabml_hip_debug_step_plan, against tests/golden/step_plan_cpu.json word for word.  The file is a RECORD of what the contexts ran
before the decisions were gathered into one function (tools/record_step_plan.py); no rule is restated here.  What needs a kernel's
LDS limit raised reads 0 on this device: tests/test_hip_step_plan.py covers those words on the GPU."""
import os

import pytest

os.environ["CRABML_HIP_TEST_HOOKS"] = "1"

import crabml_amd as ca  # noqa: E402
from tests import step_plan_cases as spc  # noqa: E402

REFUSALS = 2  # cases of the matrix that create refuses (recorded with the error's kind and text)


@pytest.fixture(scope="module")
def golden():
    return spc.load_golden("step_plan_cpu.json")


def test_every_case_runs_what_it_ran_before(golden):
    cases = spc.cpu_cases()
    assert sorted(c["id"] for c in cases) == sorted(golden), "the matrix and the record list different cases"
    ev = spc.Evaluator(ca, "dry")
    wrong = {}
    for c in cases:
        got = ev.plan(c)
        if got != golden[c["id"]]:
            want = golden[c["id"]]
            wrong[c["id"]] = {k: (want.get(k), got.get(k)) for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)}
    assert not wrong, "(recorded, now) per word: %r" % wrong


def test_the_record_exercises_the_table(golden):
    plans = [v for v in golden.values() if "error" not in v]
    assert len(golden) - len(plans) == REFUSALS
    for word in ("path", "ordered", "norm_epi", "norm_epi_k", "defer_norm", "q8k_producers", "k_norm_in"):
        assert len({p[word] for p in plans}) >= 2, word
    assert {p["path"] for p in plans} == {0, 1, 2}
    # the record-only device: 256 compute units, no graphs, no raised kernel
    assert {(p["n_cu"], p["use_graph"], p["graphs"], p["attn_flash"], p["attn_s_rows"], p["gu_rows"]) for p in plans} == {(256, 0, 0, 0, 0, 0)}


def test_create_still_refuses_the_record_only_device_the_read_out_serves():
    """crabml_hip_debug_step_plan accepts the record-only device; the create entry points still refuse it."""
    ev = spc.Evaluator(ca, "dry")
    c = spc.case("tiny-gqa", "Q4_0")
    assert ev.plan(c)["path"] == 1
    conf, w = ev.hip[("tiny-gqa", "Q4_0", 1, True, False)]
    with pytest.raises(ca.CrabmlError, match="record-only test device"):
        ca.HipLlamaRunner(conf, w, ev.devs[False], 64, True)
