"""bench.py on the GPU, plain and --full: a plain run times the headline alone and writes no detail file; --full adds
the side measurements after the timed steps and writes the detail file.  (One block and one step: the code paths, not
the figures.)"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _bench(tmp_path, *extra):
    detail = tmp_path / "detail.json"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--blocks", "1", "--steps", "1", "--warmup", "0",
           "--detail", str(detail)] + list(extra)
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-4000:]
    return json.loads(run.stdout.strip().split("\n")[-1]), detail


def test_plain_run_times_the_headline_alone(tmp_path):
    line, detail = _bench(tmp_path)
    assert line["steps"] == 1 and line["warmup"] == 0 and len(line["step_ms"]) == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["config"]["layers_per_step"] == 7
    for key in ("phases_ms", "roofline", "c2_layers_per_s", "cpu_baseline"):
        assert key not in line, key
    assert line["detail"] is None and not detail.exists()


def test_full_run_adds_the_side_measurements(tmp_path):
    line, detail = _bench(tmp_path, "--full", "--no-extras")
    assert line["steps"] == 1 and line["value"] > 0
    assert line["c2_layers_per_s"] > 0 and "phases_ms" not in line
    full = json.loads(detail.read_text())
    assert len(full["detail"]["step_ms"]) == 1 and "c2_single_layer" in full["detail"]
