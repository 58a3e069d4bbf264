"""bench.py without --full on the GPU: one JSON line with the headline figure and none of the measurements that --full
adds, and the outputs of the last timed step when --dump-outputs asks for them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("stages_ms_per_step", "fused_first_filter", "e2e", "api_e2e", "front_end", "multi_k", "bubbles", "cfg4",
             "cpu_baseline", "cpu_baseline_python", "cpu_baseline_ncore")


@pytest.mark.gpu
def test_plain_line_is_the_headline(tmp_path):
    steps, warmup = 2, 1
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                           "--warmup", str(warmup), "--dump-outputs", str(tmp_path)],
                          cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout[-3000:]
    out = json.loads(lines[0])
    assert out["metric"] == "gene-mers/s to corrected GeneMerGraph"
    assert out["unit"] == "gene-mers/s" and out["higher_is_better"] is True and out["dtype"] == "int32"
    assert (out["n_gpus"], out["steps"], out["warmup"]) == (1, steps, warmup)
    # value and ms_per_step are the same clock: gene-mers of one step (1 M reads x 56 windows) per step time
    assert out["value"] * out["ms_per_step"] * 1e-3 == pytest.approx(1_000_000 * 56, rel=1e-9)
    assert out["config"]["final_nodes"] > 0 and out["config"]["final_edges"] > 0
    assert out["roofline"] is None
    assert not [key for key in FULL_ONLY if key in out]
    sizes = np.load(tmp_path / "sizes.npy")
    assert sizes[2] == out["config"]["final_nodes"] and sizes[4] == 5
