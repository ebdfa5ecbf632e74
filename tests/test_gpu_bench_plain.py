"""A plain bench.py run (no --full) on one GPU at reduced size: the line
carries the headline fields and none of the --full measurements, --steps sets
the number of timed steps, and --dump-outputs writes the last timed step's
release -- the same release from run to run (fixed inputs, nonce = fixed base
+ step index), so two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 200_000


def _run(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--records", "3000000",
           "--pids", "30000", "--partitions", str(P), "--steps", str(steps), "--warmup", "1",
           "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_and_reproducible_dump(built, tmp_path):
    d = _run(tmp_path / "a", 3)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "records/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(3_000_000 / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert 0 < d["roofline"]["device_ms"] <= d["ms_per_step"] * 1.01
    for moved in ("kernels", "cpu_baseline", "ms_per_step_pipelined", "kept_pairs"):
        assert moved not in d
    assert d["roofline"]["traffic"] is None
    ids = np.load(tmp_path / "a" / "partition_ids.npy")
    vals = np.load(tmp_path / "a" / "values.npy")
    assert sorted(os.listdir(tmp_path / "a")) == ["partition_ids.npy", "values.npy"]
    assert ids.dtype == np.float64 and vals.dtype == np.float64
    assert len(ids) == d["kept_partitions"] > 0 and vals.shape == (len(ids), 3)
    assert len(np.unique(ids)) == len(ids) and ids.min() >= 0 and ids.max() < P
    # the same arguments again: the last of 3 steps is the same release (kept
    # set exact; the noised columns to the 1e-9 relative of the float sums'
    # ordering, as in the parity suites)
    _run(tmp_path / "b", 3)
    assert np.array_equal(ids, np.load(tmp_path / "b" / "partition_ids.npy"))
    assert np.allclose(vals, np.load(tmp_path / "b" / "values.npy"), rtol=1e-9, atol=1e-9)
