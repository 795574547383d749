"""bench.py's command line: a plain run times ONE region of exactly --steps steps and measures nothing else, `--full` adds every
other leg, `--dump-outputs DIR` writes what the timed path computed (the same arguments give the same inputs on every run).
CPU tests: the option defaults and the dump writer.  GPU tests: both kinds of run end to end on the tiny-gqa shape."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("fused_entry_point", "roofline", "c3_positions_0_127", "trait_path", "parity_check", "cpu_baseline", "gemv_points")


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_times_one_region_and_full_repeats_it(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.repeats, a.steps, a.warmup, a.dump_outputs) == (False, 1, 7, 2, None)
    a = parse(monkeypatch, "--full")
    assert (a.full, a.repeats) == (True, 5)
    a = parse(monkeypatch, "--full", "--repeats", "2", "--dump-outputs", "d")
    assert (a.full, a.repeats, a.dump_outputs) == (True, 2, "d")


def test_dump_outputs_writes_float_arrays_only(tmp_path):
    bench.dump_outputs(str(tmp_path / "o"), {"tokens": [float(t) for t in (3, 1, 2)], "logits": np.arange(4, dtype=np.float32)})
    assert sorted(os.listdir(tmp_path / "o")) == ["logits.npy", "tokens.npy"]
    t = np.load(tmp_path / "o" / "tokens.npy")
    assert t.dtype == np.float64 and t.tolist() == [3.0, 1.0, 2.0]
    assert np.load(tmp_path / "o" / "logits.npy").dtype == np.float32
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "o"), {"ids": np.arange(3)})


def run_bench(*extra, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "tiny-gqa", *extra],
                       capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_its_outputs_repeat(tmp_path):
    dumps = []
    for i in range(2):
        d = tmp_path / str(i)
        line = run_bench("--steps", "12", "--warmup", "3", "--dump-outputs", str(d))
        assert line["steps"] == 12 and line["warmup"] == 3 and line["timed_regions"]["repeats"] == 1
        assert line["value"] > 0 and line["ms_per_step"] == pytest.approx(1e3 / line["value"], rel=1e-2)
        for k in ("metric", "unit", "higher_is_better", "dtype"):
            assert k in line
        assert not [k for k in FULL_ONLY if k in line]
        tokens, logits = np.load(d / "tokens.npy"), np.load(d / "logits.npy")
        assert tokens.dtype == np.float64 and tokens.shape == (12,)
        assert logits.dtype == np.float32 and logits.shape == (1024,) and np.isfinite(logits).all()
        # the last step's logits are the ones its token was sampled from (greedy: the last maximum, as the runner's arg-max)
        assert tokens[-1] == len(logits) - 1 - int(np.argmax(logits[::-1]))
        dumps.append((tokens, logits))
    assert np.array_equal(dumps[0][0], dumps[1][0])
    assert np.array_equal(dumps[0][1].view(np.uint32), dumps[1][1].view(np.uint32))


@pytest.mark.gpu
def test_full_run_keeps_every_other_leg(tmp_path):
    line = run_bench("--steps", "8", "--warmup", "2", "--full", "--cpu-seconds", "2", "--dump-outputs", str(tmp_path), timeout=900)
    assert line["timed_regions"]["repeats"] == 5 and line["value"] > 0
    missing = [k for k in FULL_ONLY if k not in line]
    assert not missing, missing
    assert line["parity_check"]["strict_bit_identical"] == [True] * 4
    assert np.load(tmp_path / "tokens.npy").shape == (8,)
