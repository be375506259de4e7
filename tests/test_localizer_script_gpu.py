"""scripts/evaluate_stability.py closed-loop with --localizer, as a program, on a synthetic shard."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from landmark_shards import write_shard
from util import GOLDEN, PKG, build_net, gpu_section, load_golden

SCRIPT = os.path.join(PKG, "scripts", "evaluate_stability.py")
FRAMES, H, W = 12, 72, 96


def _script(*argv):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, SCRIPT, *argv], env=env, capture_output=True, text=True, timeout=300)


def _localizer_checkpoint(path):
    d = np.load(os.path.join(GOLDEN, "localizer.npz"))
    torch.save({k: torch.from_numpy(d["sd/" + k]) for k in json.loads(str(d["meta"]))["keys"]}, path)  # a plain state_dict file
    return path


@pytest.mark.gpu
def test_closed_loop_with_a_localizer_end_to_end(tmp_path):
    from trackertraincode.neuralnets.models import save_model

    src = write_shard(tmp_path, "video", "pose", FRAMES, H, W, seed=19)
    g, meta = load_golden("model_w050.npz")
    cal = {k[len("calib/"):]: g[k] for k in g.files if k.startswith("calib/")}
    ckpt, out = str(tmp_path / "net.ckpt"), str(tmp_path / "out.npz")
    save_model(build_net(meta, "cpu", cal), ckpt)
    loc = _localizer_checkpoint(str(tmp_path / "localizer.ckpt"))
    with gpu_section():
        res = _script("closed-loop", src, ckpt, "--output", out, "--localizer", loc, "--reacquire-after", "2", "--face-threshold", "0.05")
    assert res.returncode == 0, res.stderr[-3000:]
    assert "re-acquisitions per lane" in res.stdout and "lost frames per lane" in res.stdout
    saved = np.load(out)
    assert saved["g0/reacquired"].shape == (1, FRAMES, 2) and saved["g0/reacquired"].dtype == bool
    assert saved["g0/hasface"].shape == (1, FRAMES) and saved["g0/loc_roi"].shape == (1, FRAMES, 4)
    assert np.all((saved["g0/hasface"] > 0) & (saved["g0/hasface"] < 1)) and np.all(np.isfinite(saved["g0/loc_roi"]))
    assert saved["g0/lost"].shape == (1, FRAMES, 2)
    # a lane is re-acquired only after a run of lost frames
    lost, re = saved["g0/lost"][0], saved["g0/reacquired"][0]
    assert not np.any(re & ~lost)


@pytest.mark.parametrize("mode", ["open-loop", "noise-resist"])
def test_the_other_modes_refuse_the_flag(tmp_path, mode):
    res = _script(mode, str(tmp_path / "none.npz"), str(tmp_path / "none.ckpt"), "--localizer", str(tmp_path / "loc.ckpt"))
    assert res.returncode != 0 and "--localizer" in res.stderr and "closed-loop" in res.stderr
