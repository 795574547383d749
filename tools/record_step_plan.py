"""Records the step plan of every case of tests/step_plan_cases.py: `cpu` on the record-only device -> tests/golden/step_plan_cpu.json,
`gpu` on an MI355X -> tests/golden/step_plan_mi355x.json (or the path given).  The committed records were taken at the commit before
decide_step existed, with the read-out computing its words from the context's loose members; the tests hold every later commit to them."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["CRABML_HIP_TEST_HOOKS"] = "1"

import crabml_amd as ca  # noqa: E402
from tests import step_plan_cases as spc  # noqa: E402


def main():
    kind = sys.argv[1]
    cases, mode, name = (spc.cpu_cases(), "dry", "step_plan_cpu.json") if kind == "cpu" else (spc.gpu_cases(), "lazy", "step_plan_mi355x.json")
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(spc.GOLDEN, name)
    ev = spc.Evaluator(ca, mode)
    rec = {c["id"]: ev.plan(c) for c in cases}
    assert len(rec) == len(cases), "case ids are not unique"
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(rec[k], sort_keys=True)) for k in sorted(rec)) + "\n}\n")  # a case per line
    print("recorded %d cases (%d refusals) -> %s" % (len(rec), sum("error" in v for v in rec.values()), path))


if __name__ == "__main__":
    main()
