"""bench.py on the GPU: a plain run prints the headline line and nothing that takes runs of its own (those come with --full)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_headline_only():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "tiny", "--steps", "2", "--warmup", "1"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    j = json.loads(line[0])
    assert j["value"] > 0 and j["ms_per_step"] > 0 and j["steps"] == 2 and j["warmup"] == 1
    assert "cpu_baseline" not in j and "also" not in j
    assert j["roofline"]["traffic"] is None and j["roofline"]["mfma_busy"] is None      # no rocprofv3 --pmc child passes
