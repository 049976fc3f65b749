"""bench.py --dump-outputs on the GPU: `--steps` timed steps are run, and what the last one computed is written the same
from run to run (seeded inputs), so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _bench(tmp_path, tag):
    out = tmp_path / tag
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c2", "--no-extras", "--steps", "2",
           "--warmup", "1", "--dump-outputs", str(out), "--detail", str(tmp_path / f"{tag}_detail.json")]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-4000:]
    return json.loads(run.stdout.strip().split("\n")[-1]), out


def test_dump_outputs_of_the_last_timed_step_repeat_from_run_to_run(tmp_path):
    line_a, a = _bench(tmp_path, "a")
    line_b, b = _bench(tmp_path, "b")
    for line in (line_a, line_b):
        assert line["steps"] == 2 and len(line["step_ms"]) == 2
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    # the one nn.Linear(4096, 4096) of BASELINE configs[1] comes back as a rank-r pair, and its config entry with it
    assert "layers.0.0.weight.npy" in names and "layers.0.1.weight.npy" in names and "config.layers.0.npy" in names
    assert sum(os.path.getsize(a / n) for n in names) <= 64 * 10**6
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), n
        assert np.array_equal(x, y), n
