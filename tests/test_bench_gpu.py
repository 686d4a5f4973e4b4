"""bench.py on the GPU: a plain run prints the headline line and nothing measured besides it, --dump-outputs writes the
same outputs for the same arguments, and --full still carries the per-kernel roofline and breakdown."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "kernel_breakdown_ms", "kernel_rates", "small_batch", "secondary", "cpu_baseline")


def run_bench(*argv):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", *argv], capture_output=True,
                         text=True, timeout=500)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.timeout(600)
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    lines = [run_bench("--workload", "c1", "--steps", "3", "--warmup", "1", "--deterministic",
                       "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "samples/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
        assert not set(FULL_ONLY) & set(line), sorted(line)
    names = sorted(os.listdir(tmp_path / "a"))
    assert "loss.npy" in names and sum(n.startswith("param.") for n in names) == 155  # DiT-S: 155 parameter tensors
    assert sum(n.startswith("grad.") for n in names) > 100
    assert names == sorted(os.listdir(tmp_path / "b"))
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all()
        assert np.array_equal(x, y), n  # deterministic mode: the same inputs give the same bits
        total += x.nbytes
    assert total <= 64 << 20
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == lines[0]["loss"]  # the loss of the last timed step


@pytest.mark.timeout(600)
def test_full_run_keeps_the_kernel_figures():
    line = run_bench("--workload", "c1", "--steps", "3", "--warmup", "2", "--full", "--no-cpu-baseline")
    assert line["steps"] == 3 and line["roofline"]["kernel"] in line["kernel_breakdown_ms"]
