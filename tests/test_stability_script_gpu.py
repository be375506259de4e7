"""scripts/evaluate_stability.py as a program: a synthetic 24-frame shard and two half-width checkpoints."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from landmark_shards import write_shard
from util import PKG, build_net, gpu_section, load_golden

pytestmark = pytest.mark.gpu

SCRIPT = os.path.join(PKG, "scripts", "evaluate_stability.py")
FRAMES, H, W = 24, 72, 96


def _script(*argv):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, SCRIPT, *argv], env=env, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """The shard (boxes + pose labels, frames in order), two half-width checkpoints, and the closed-loop runs: each checkpoint alone and
    both through a glob."""
    from trackertraincode.neuralnets.models import save_model

    d = tmp_path_factory.mktemp("stability")
    src = write_shard(d, "video", "pose", FRAMES, H, W, seed=19)
    g, meta = load_golden("model_w050.npz")
    cal = {k[len("calib/"):]: g[k] for k in g.files if k.startswith("calib/")}
    ckpts = []
    for seed in (0, 1):
        ckpts.append(str(d / f"net{seed}.ckpt"))
        save_model(build_net(dict(meta, state_seed=seed), "cpu", cal), ckpts[-1])
    runs = {}
    with gpu_section():
        runs["both"] = _script("closed-loop", src, str(d / "net*.ckpt"), "--output", str(d / "both.npz"), "--blinks", "8:12")
        for i, c in enumerate(ckpts):
            runs[i] = _script("closed-loop", src, c, "--output", str(d / f"single{i}.npz"), "--blinks", "8:12")
    return {"dir": d, "src": src, "ckpts": ckpts, "runs": runs}


def test_closed_loop_writes_mean_and_std_over_a_glob(setup):
    for k, res in setup["runs"].items():
        assert res.returncode == 0, res.stderr[-3000:]
    both = np.load(setup["dir"] / "both.npz")
    singles = [np.load(setup["dir"] / f"single{i}.npz") for i in (0, 1)]
    shapes = {"hpb": (FRAMES, 2, 3), "xy": (FRAMES, 2, 2), "sz": (FRAMES, 2)}
    for k, shape in shapes.items():
        assert both[f"g0/{k}"].shape == shape and both[f"g0/{k}_std"].shape == shape, k
        stack = [s[f"g0/{k}"] for s in singles]
        assert np.array_equal(both[f"g0/{k}"], np.average(stack, axis=0)) and np.array_equal(both[f"g0/{k}_std"], np.std(stack, axis=0)), k
        assert all(np.all(s[f"g0/{k}_std"] == 0) for s in singles)
    assert both["g0/lost"].shape == (2, FRAMES, 2) and both["g0/lost"].dtype == bool and np.array_equal(both["factors"], [1.0, 1.2])
    assert np.array_equal(both["g0/lost"], np.stack([s["g0/lost"][0] for s in singles]))
    out = setup["runs"]["both"].stdout
    assert "Found 2 checkpoints" in out and out.count("lost frames per lane") == 2
    # the blink report: one line per quantity, hpb with three numbers
    lines = {ln.split(":")[0].strip(): ln.split(":")[1] for ln in out.splitlines() if ln.startswith("\t ")}
    assert set(lines) == {"hpb", "sz", "xy"} and len(lines["hpb"].split(",")) == 3 and len(lines["xy"].split(",")) == 2


def test_blink_report_is_the_package_function(setup):
    from trackertraincode.eval import blink_stability

    s, res = np.load(setup["dir"] / "single0.npz"), setup["runs"][0]
    assert res.returncode == 0, res.stderr[-3000:]
    want = np.average([blink_stability(s["g0/sz"][:, lane], [(8, 12)]) for lane in (0, 1)], axis=0)
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("\t sz")][0]
    assert line.split(":")[1].strip() == f"{want[0]:0.2f}"


def test_blinks_near_the_ends_are_refused(setup):
    res = _script("closed-loop", setup["src"], setup["ckpts"][0], "--blinks", "2:12")  # (refused before anything touches the GPU)
    assert res.returncode != 0 and "within 5 frames" in res.stderr


def test_first_frame_of_closed_loop_is_the_open_loop_frame(setup):
    """Frame 0 is cropped around the stored box in both modes: bitwise the same crops.  The forwards differ in their batch (the lanes of
    one frame against a batch of frames with one factor), so in the tiling and summation order of the float32 GEMMs: compared to 1e-4 of
    the quantities' magnitudes - angles in radians, positions and sizes in pixels of a 96-pixel frame - not bitwise."""
    out = str(setup["dir"] / "open.npz")
    with gpu_section():
        res = _script("open-loop", setup["src"], setup["ckpts"][0], "--output", out)
    assert res.returncode == 0, res.stderr[-3000:]
    opened, closed = np.load(out), np.load(setup["dir"] / "single0.npz")
    assert opened["g0/hpb"].shape == (FRAMES, 2, 3) and not opened["g0/lost"].any()
    for k, scale in (("hpb", np.pi), ("xy", 96.0), ("sz", 96.0)):
        assert np.allclose(opened[f"g0/{k}"][0], closed[f"g0/{k}"][0], rtol=0, atol=1e-4 * scale), k


def test_noise_resist_level_zero_is_the_plain_error_and_seeds_repeat(setup):
    from trackertraincode import eval as E
    from trackertraincode.datasets.batch import Batch, Metadata
    from trackertraincode.datasets.shards import decode_pose_shard
    from trackertraincode.neuralnets.models import load_model

    out = str(setup["dir"] / "noise.npz")
    with gpu_section():
        a = _script("noise-resist", setup["src"], *setup["ckpts"], "--seed", "5", "--output", out)
        b = _script("noise-resist", setup["src"], *setup["ckpts"], "--seed", "5")
    assert a.returncode == 0, a.stderr[-3000:]
    assert b.returncode == 0 and a.stdout == b.stdout and "average" in a.stdout and "std" in a.stdout
    saved = np.load(out)
    assert saved["geodesic_deg"].shape == (2, 7) and np.array_equal(saved["noise_levels"], [0, 2, 8, 16, 32, 48, 64])
    shard = decode_pose_shard(setup["src"])
    with gpu_section(), torch.no_grad():
        for i, f in enumerate(setup["ckpts"]):
            p = E.Predictor(load_model(f))
            images = torch.from_numpy(shard["image"]).cuda()
            crop = p._crop(Batch(Metadata((W, H), FRAMES), image=images, roi=torch.from_numpy(shard["roi"]).cuda(), pose=torch.from_numpy(shard["pose"]).cuda()))
            err = E.GeodesicError()
            err.update(p.predict_cropped_normalized_batch(crop["image"]), crop)
            plain = float(err.compute().mean().item()) * 180.0 / np.pi
            assert saved["geodesic_deg"][i, 0] == plain, (saved["geodesic_deg"][i, 0], plain)  # level 0 adds 0 * noise: the same crops, the same batch
    assert np.all(np.isfinite(saved["geodesic_deg"]))


@pytest.mark.parametrize("mode", ["pitch-yaw", "variation-resist", "uncertainty-correlation"])
def test_modes_out_of_scope_are_refused_with_a_reason(setup, mode):
    res = _script(mode, setup["src"], setup["ckpts"][0])
    assert res.returncode != 0 and "not built" in res.stderr
