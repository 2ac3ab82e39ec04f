"""bench.py's command line: a plain run measures the headline only, --dump-outputs writes what the last
timed step returned; the side measurements (--full) are not run here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "roofline_inflight", "h2d_ms_per_batch", "other_configs", "note_commitment_trees",
             "pghr13_sprout_proofs", "cpu_baseline")


def test_dump_outputs_files(tmp_path):
    """float32 arrays named after what the caller receives; a rank of a larger world tags its files"""
    import bench
    out = str(tmp_path / "d")
    bench.dump_outputs(out, (True, [0, 3, 1, 0]), 0, 1)
    bench.dump_outputs(out, (False, [4]), 1, 2)
    assert sorted(os.listdir(out)) == ["statuses.npy", "statuses_rank1.npy", "verdict.npy", "verdict_rank1.npy"]
    sts, ok = np.load(os.path.join(out, "statuses.npy")), np.load(os.path.join(out, "verdict.npy"))
    assert sts.dtype == np.float32 and sts.tolist() == [0.0, 3.0, 1.0, 0.0]
    assert ok.dtype == np.float32 and ok.tolist() == [1.0]
    assert np.load(os.path.join(out, "verdict_rank1.npy")).tolist() == [0.0]


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_is_the_headline_only(tmp_path):
    """bench.py without --full on an 8,192-proof batch: the result line holds the headline with the steps
    asked for and none of the side measurements, and the dumped statuses are the all-valid batch's"""
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--proofs", "8192",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", out],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["context_stats"]["batches"] == 4
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 - 8192) < 1e-3 * 8192
    sts, ok = np.load(os.path.join(out, "statuses.npy")), np.load(os.path.join(out, "verdict.npy"))
    assert sts.dtype == np.float32 and sts.shape == (8192,) and not sts.any()
    assert ok.dtype == np.float32 and ok.tolist() == [1.0]
