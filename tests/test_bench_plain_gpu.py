"""A plain `bench.py` run: the headline line alone (none of the --full measurements), exactly --steps timed steps, and --dump-outputs
writing the last timed step's results - the same, up to rounding, on every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "64",
           "--dump-outputs", str(out_dir)]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def test_plain_run_and_dump(tmp_path):
    out = _run(tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "crops/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and abs(d["value"] - 64 * 1000 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert d["roofline"] is None and d["optimizer_ms"] is None and not d["kernels_ms_per_step"]
    assert not {"legs", "copy_probe", "cpu_baseline", "comm"} & set(d)
    files = os.listdir(tmp_path)
    assert "loss.npy" in files and any(f.startswith("mt_loss.") for f in files)
    assert any(f.startswith("param.convnet.") for f in files) and any(f.startswith("grad.convnet.") for f in files)
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in files) < 64 * 10**6
    assert float(np.load(os.path.join(tmp_path, "loss.npy"))) == pytest.approx(d["loss"], rel=1e-6)
    for f in files:
        a = np.load(os.path.join(tmp_path, f))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f


def test_dump_is_the_same_on_every_run(tmp_path):
    """Every step starts from the seeded initial weights (bench.py: WeightReset), so two runs differ only by the rounding of the
    weight-gradient reductions, which add in no fixed order: measured <= 8e-7 of a tensor's largest element at B = 512."""
    for name in ("a", "b"):
        out = _run(tmp_path / name)
        assert out.returncode == 0, out.stderr[-3000:]
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    for f in files:
        a, b = np.load(tmp_path / "a" / f).astype(np.float64), np.load(tmp_path / "b" / f).astype(np.float64)
        assert np.abs(a - b).max() <= 1e-5 * max(np.abs(a).max(), 1e-30), f
