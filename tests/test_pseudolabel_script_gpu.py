"""scripts/add_pose_pseudolabels.py as a program: a synthetic 12-frame shard labelled by two checkpoints."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from landmark_shards import write_shard
from util import PKG, build_net, gpu_section, load_golden, script_args, train_script

pytestmark = pytest.mark.gpu

SCRIPT = os.path.join(PKG, "scripts", "add_pose_pseudolabels.py")
FRAMES = 12


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """The shard (rois + 2-D landmarks, no pose labels of its own), two half-width checkpoints, and the script's output for them."""
    from trackertraincode.neuralnets.models import save_model

    d = tmp_path_factory.mktemp("pseudolabels")
    src = write_shard(d, "faces", "landmarks_2d", FRAMES, 72, 96, seed=9)
    g, meta = load_golden("model_w050.npz")
    cal = {k[len("calib/"):]: g[k] for k in g.files if k.startswith("calib/")}
    ckpts = []
    for seed in (0, 1):
        ckpts.append(str(d / f"net{seed}.ckpt"))
        save_model(build_net(dict(meta, state_seed=seed), "cpu", cal), ckpts[-1])
    out = str(d / "faces_lp.npz")
    with gpu_section():
        first = _script(src, "-c", *ckpts, "--output", out, "-b", "5")  # 12 frames in batches of 5, 5, 2
    return {"dir": d, "src": src, "ckpts": ckpts, "out": out, "first": first, "meta": meta}


def _script(*argv):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, SCRIPT, *argv], env=env, capture_output=True, text=True, timeout=300)


def test_script_labels_equal_the_ensemble_predictor(setup):
    from trackertraincode import eval as E
    from trackertraincode.datasets.shards import decode_pose_shard
    from trackertraincode.neuralnets.models import load_model

    assert setup["first"].returncode == 0, setup["first"].stderr[-3000:]
    assert f"{FRAMES} frames labelled by 2 networks" in setup["first"].stdout and "0 dropped" in setup["first"].stdout
    src, got = decode_pose_shard(setup["src"]), decode_pose_shard(setup["out"])
    with gpu_section():
        ens = E.EnsemblePredictor([load_model(f) for f in setup["ckpts"]])
        images, rois = torch.from_numpy(src["image"]).cuda(), torch.from_numpy(src["roi"]).cuda()
        want = [ens.predict_batch(images[lo:lo + 5], rois[lo:lo + 5]) for lo in (0, 5, 10)]
        want = {k: torch.cat([w[k] for w in want]).cpu().numpy() for k in ("pose", "coord", "pt3d_68", "shapeparam", "rot_spread", "mean_quat_norm", "coord_spread")}
    assert np.array_equal(got["pose"], want["pose"]) and np.array_equal(got["shapeparam"], want["shapeparam"])
    # the writer stores x - 0.5 and the decoder adds 0.5 again, both in float32: exactly that, and z / the size as they are
    for k in ("coord", "pt3d_68"):
        there_and_back = want[k].copy()
        there_and_back[..., :2] = (want[k][..., :2] - np.float32(0.5)) + np.float32(0.5)
        assert got[k].dtype == np.float32 and np.array_equal(got[k], there_and_back), k
    raw = np.load(setup["out"])
    for k in ("rot_spread", "mean_quat_norm", "coord_spread"):
        assert np.array_equal(raw["pseudolabel_" + k], want[k]), k
    for k in ("image", "roi", "pt2d_68", "individual"):
        assert np.array_equal(got[k], src[k]), k


def test_second_run_without_overwrite_fails_and_leaves_the_file(setup):
    before = open(setup["out"], "rb").read()
    res = _script(setup["src"], "-c", *setup["ckpts"], "--output", setup["out"])  # (refused before anything touches the GPU)
    assert res.returncode != 0 and "exists" in res.stderr
    assert open(setup["out"], "rb").read() == before
    res = _script(setup["out"], "-c", *setup["ckpts"])  # default output = the input
    assert res.returncode != 0 and open(setup["out"], "rb").read() == before


def test_dryrun_labels_ten_frames(setup):
    out = str(setup["dir"] / "dry.npz")
    with gpu_section():
        res = _script(setup["src"], "-c", *setup["ckpts"], "--output", out, "--dryrun", "-b", "5")  # (the batches of the full run: same kernels per row)
    assert res.returncode == 0, res.stderr[-3000:]
    raw, full = np.load(out), np.load(setup["out"])
    assert all(len(raw[k]) == 10 for k in raw.files)
    assert np.array_equal(raw["quats"], full["quats"][:10]) and np.array_equal(raw["images"], full["images"][:10])
    res = _script(setup["src"], "-c", *setup["ckpts"], "--dryrun", "-f")
    assert res.returncode != 0 and "--output" in res.stderr and len(np.load(setup["src"])["images"]) == FRAMES


def test_max_rot_spread_zero_drops_every_frame_with_a_spread(setup):
    out = str(setup["dir"] / "strict.npz")
    with gpu_section():
        res = _script(setup["src"], "-c", *setup["ckpts"], "--output", out, "--max-rot-spread", "0")
    assert res.returncode == 0, res.stderr[-3000:]
    spread = np.load(setup["out"])["pseudolabel_rot_spread"]
    kept = np.load(out)
    assert (spread > 0).any() and len(kept["images"]) == int((spread == 0).sum()) and f"{int((spread > 0).sum())} dropped" in res.stdout
    assert all(len(kept[k]) == len(kept["images"]) for k in kept.files)


def test_labelled_shard_trains(setup):
    """The written shard as a POSE_WITH_LANDMARKS training set: resident frames -> crop -> one training step, finite loss."""
    import trackertraincode.train as train
    from trackertraincode.datasets.resident import ResidentLoader
    from trackertraincode.datasets.shards import load_resident_frames
    from trackertraincode.pipelines import Tag

    assert setup["first"].returncode == 0
    S = train_script()
    with gpu_section():
        frames = load_resident_frames(setup["out"], Tag.POSE_WITH_LANDMARKS)
        assert len(frames) == FRAMES and {"pose", "coord", "pt3d_68", "shapeparam", "roi"} <= set(frames.fields)
        net = build_net(setup["meta"], "cuda").train()
        crit, _ = S.setup_losses(script_args(setup["meta"]["flags"]), net)
        batches = next(iter(ResidentLoader([frames], [1.0], batchsize=8, steps_per_epoch=1)))
        out = train.training_step(net, batches, 0, crit)
        loss = float(out["loss"].detach())
    assert np.isfinite(loss)
