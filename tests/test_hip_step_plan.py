"""The words of a context's step plan that only a real device can reach (tests/test_step_plan.py holds the rest on the record-only
device): the attention forms, which need kernels' LDS limits raised, the captured graphs, the ordered forms of the strict-order device
and gate | up's row count on a tensor-parallel rank -- through crabml_hip_debug_step_plan, against tests/golden/step_plan_mi355x.json
word for word (a RECORD of what the contexts ran on an MI355X before the decisions were gathered into decide_step; tools/
record_step_plan.py).  Contexts are created and destroyed only; no step runs."""
import os

import pytest

os.environ["CRABML_HIP_TEST_HOOKS"] = "1"

import crabml_amd as ca  # noqa: E402
from tests import step_plan_cases as spc  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = ["tiny-gqa/Q4_0", "tiny-gqa/Q4_1", "tiny-hd128/Q4_0", "tiny-hd128/Q4_1", "tiny-gqa/Q4_K", "tiny-gemma", "gu-rows"]


@pytest.fixture(scope="module")
def golden():
    return spc.load_golden("step_plan_mi355x.json")


@pytest.fixture(scope="module")
def evaluator():
    return spc.Evaluator(ca, "lazy")


def test_the_groups_cover_the_matrix(golden):
    ids = sorted(c["id"] for c in spc.gpu_cases())
    assert ids == sorted(golden), "the matrix and the record list different cases"
    assert all(sum(i.startswith(g + "/") for g in GROUPS) == 1 for i in ids)
    assert not [i for i, v in golden.items() if "error" in v]
    # the record reaches what the record-only device cannot
    plans = list(golden.values())
    for word in ("attn_long_ok", "exact_long_ok", "pv_split", "attn_flash", "flash_ticket", "attn_flash_rows", "attn_s_rows", "ordered", "path"):
        assert len({p[word] for p in plans}) >= 2, word
    assert {96, 224, 12} <= {p["attn_long_from"] for p in plans} and {1, 2, 3} <= {p["graphs"] for p in plans}
    assert {golden[i]["gu_rows"] for i in golden if i.startswith("gu-rows/")} == {0, 16}


@pytest.mark.parametrize("group", GROUPS)
def test_every_case_runs_what_it_ran_before(golden, evaluator, group):
    wrong = {}
    for c in spc.gpu_cases():
        if not c["id"].startswith(group + "/"):
            continue
        got, want = evaluator.plan(c), golden[c["id"]]
        if got != want:
            wrong[c["id"]] = {k: (want.get(k), got.get(k)) for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)}
    assert not wrong, "(recorded, now) per word: %r" % wrong
