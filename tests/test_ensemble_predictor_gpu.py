"""eval.EnsemblePredictor: several networks on one crop, reduced by ttk_ensemble_reduce, against `Predictor` per network and
tests/ensemble_ref.py in float64.

Tolerances: the bounds of tests/ensemble_cases.py, evaluated on the networks' raw outputs (the kernel's inputs).  Where the comparison is
against `Predictor` - whose back-transformation is apply_affine2d in float32 torch: the same sums of products with the same operand
magnitudes, and atan2 / sin / cos of the same accuracy class - both sides lie within one bound of the exact value, so they are held to
TWICE the bound of each output."""
import types

import numpy as np
import pytest
import torch

import ensemble_ref as ER
from ensemble_cases import bounds, compare, within
from util import build_net, gpu_section, load_golden

pytestmark = pytest.mark.gpu

SIZES = [(96, 128), (96, 128), (120, 100), (96, 128), (120, 100)]  # five images of two sizes


@pytest.fixture(scope="module")
def nets():
    """Three half-width networks with the landmark head (state seeds 0, 1, 2) and a full-width one without it."""
    g, meta = load_golden("model_w050.npz")
    cal = {k[len("calib/"):]: g[k] for k in g.files if k.startswith("calib/")}
    small = [build_net(dict(meta, state_seed=s), "cuda", cal).eval() for s in (0, 1, 2)]
    g, meta = load_golden("model_posonly.npz")
    cal = {k[len("calib/"):]: g[k] for k in g.files if k.startswith("calib/")}
    return small, build_net(meta, "cuda", cal).eval()


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(77)
    images = [torch.from_numpy(rng.integers(0, 256, size=s, dtype=np.uint8)) for s in SIZES]
    rois = []
    for h, w in SIZES:
        cx, cy, half = 0.5 * w + rng.uniform(-8, 8), 0.5 * h + rng.uniform(-8, 8), rng.uniform(20, 30)
        rois.append([cx - half, cy - half, cx + half, cy + half])
    return images, torch.tensor(rois, dtype=torch.float32)


def _np(batch, keys):
    return {k: batch[k].detach().cpu().numpy().astype(np.float64) for k in keys if k in batch}


def _raw_inputs(ens, members, images, rois):
    """The kernel's inputs, formed the way predict_batch forms them: the raw outputs of every network on the predictor's crop + `back`."""
    from trackertraincode.datatransformation.tensors.affinetrafo import position_normalization
    from trackertraincode.neuralnets.affine2d import Affine2d

    with torch.no_grad():
        crop = ens.crop_batch(images, rois)
        preds = [n(crop["image"]) for n in members]
    N = ens.input_resolution
    back = (position_normalization(N, N).to("cuda") @ Affine2d(crop["image_transform"])).inv().tensor()
    stack = lambda k: np.stack([p[k].cpu().numpy() for p in preds]) if all(k in p for p in preds) else None
    return {"pose": stack("pose"), "coord": stack("coord"), "pts": stack("pt3d_68"), "shape": stack("shapeparam"), "back": back.cpu().numpy()}


def _got(out):
    g = _np(out, ("pose", "coord", "pt3d_68", "shapeparam"))
    return {"pose": g["pose"], "coord": g["coord"], "pts": g.get("pt3d_68"), "shape": g.get("shapeparam"),
            "stats": np.concatenate([_np(out, ("rot_spread",))["rot_spread"][:, None], _np(out, ("mean_quat_norm",))["mean_quat_norm"][:, None],
                                     _np(out, ("coord_spread",))["coord_spread"]], -1)}


def test_single_member_equals_predictor(nets, frames):
    from trackertraincode import eval as E

    small, _ = nets
    images, rois = frames
    with gpu_section():
        ens = E.EnsemblePredictor(small[:1], focus_roi_expansion_factor=1.2)
        out = ens.predict_batch(images, rois)
        ref = E.Predictor(small[0], focus_roi_expansion_factor=1.2).predict_batch(images, rois)
        inp = _raw_inputs(ens, small[:1], images, rois)
    got = _got(out)
    r = compare(got, inp, "E=1 against float64")
    bd = bounds(inp, r)
    p = _np(ref, ("pose", "coord", "pt3d_68", "shapeparam"))
    print("E=1 against Predictor")
    within("pose", got["pose"], p["pose"], 2 * bd["pose"], up_to_sign=True)  # (the pivot rule makes the largest component positive)
    within("coord", got["coord"], p["coord"], 2 * bd["coord"])
    within("pt3d_68", got["pts"], p["pt3d_68"], 2 * bd["pts"])
    assert np.array_equal(got["shape"], p["shapeparam"])  # one member, no geometry: 0 + s, divided by 1
    assert np.all(got["pose"][np.arange(len(SIZES)), r["pivot"]] > 0)
    assert out["rot_spread"].shape == (5,) and out["mean_quat_norm"].shape == (5,) and out["coord_spread"].shape == (5, 3)
    assert np.all(got["stats"][:, 2:] == 0) and np.all(np.abs(got["stats"][:, 1] - 1) < 1e-5)


def test_three_members_equal_the_averaged_predictors(nets, frames):
    from trackertraincode import eval as E

    small, _ = nets
    images, rois = frames
    with gpu_section():
        ens = E.EnsemblePredictor(small)
        out = ens.predict_batch(images, rois)
        singles = [E.Predictor(n, focus_roi_expansion_factor=1.2).predict_batch(images, rois) for n in small]
        inp = _raw_inputs(ens, small, images, rois)
    got = _got(out)
    r = compare(got, inp, "E=3 against float64 on the raw outputs")
    bd = bounds(inp, r)
    # the three Predictor results, already in image coordinates, averaged in float64
    st = lambda k: np.stack([s[k].cpu().numpy() for s in singles])
    ident = np.broadcast_to(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (len(SIZES), 2, 3))
    avg = ER.ensemble_reduce(st("pose"), st("coord"), st("pt3d_68"), st("shapeparam"), ident)
    print("E=3 against the averaged Predictor results")
    within("pose", got["pose"], avg["pose"], 2 * bd["pose"])
    within("coord", got["coord"], avg["coord"], 2 * bd["coord"])
    within("pt3d_68", got["pts"], avg["pts"], 2 * bd["pts"])
    within("shapeparam", got["shape"], avg["shape"], 2 * bd["shape"])
    within("mean norm", got["stats"][:, 1], avg["stats"][:, 1], 2 * bd["norm"])
    within("coord spread", got["stats"][:, 2:], avg["stats"][:, 2:], 2 * bd["std"])
    assert np.all(got["stats"][:, 0] > 0)  # different weights: the members do not agree exactly


def test_the_crop_runs_once_per_batch(nets, frames):
    from trackertraincode import eval as E

    small, _ = nets
    images, rois = frames
    ens = E.EnsemblePredictor(small)
    calls, crop = [], ens._crop

    def counted(batch):
        calls.append(int(batch.meta.batchsize))
        return crop(batch)

    ens._crop = counted
    with gpu_section():
        ens.predict_batch(images, rois)
    assert sorted(calls) == [2, 3]  # one warp per image size - not one per network
    calls.clear()
    with gpu_section():
        ens.predict_batch(torch.stack([images[0], images[1], images[3]])[:, None], rois[[0, 1, 3]])
    assert calls == [3]


def test_a_network_without_the_landmark_head_drops_the_landmarks(nets, frames):
    from trackertraincode import eval as E

    small, posonly = nets
    images, rois = frames
    with gpu_section():
        ens = E.EnsemblePredictor([small[0], posonly])
        out = ens.predict_batch(images, rois)
        inp = _raw_inputs(ens, [small[0], posonly], images, rois)
    assert "pt3d_68" not in out and "shapeparam" not in out and "pose" in out and "coord" in out
    assert inp["pts"] is None and inp["shape"] is None
    got = _np(out, ("pose", "coord"))
    got.update(pts=None, shape=None, stats=np.concatenate([out[k].cpu().numpy().astype(np.float64).reshape(5, -1)
                                                           for k in ("rot_spread", "mean_quat_norm", "coord_spread")], -1))
    compare(got, inp, "E=2, one member without the landmark head")


def test_mixed_input_resolutions_raise(nets):
    from trackertraincode import eval as E

    small, _ = nets
    with pytest.raises(ValueError, match="input resolutions"):
        E.EnsemblePredictor([small[0], types.SimpleNamespace(input_resolution=97)])
    with pytest.raises(ValueError, match="1 to 16"):
        E.EnsemblePredictor([])
