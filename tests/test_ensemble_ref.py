"""tests/ensemble_ref.py (the float64 restatement of ttk_ensemble_reduce) against what it restates: the reference's own quat_average /
np.average (tests/golden/ensemble.npz, tools/gen_golden_ensemble.py) and the repository's apply_affine2d."""
import os

import numpy as np
import pytest
import torch

import ensemble_ref as ER
from util import GOLDEN

IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ensemble.npz"))


@pytest.mark.parametrize("E", [1, 2, 3, 5, 16])
def test_reduction_matches_the_references_average(golden, E):
    g = {k: golden[f"E{E}/{k}"] for k in ("pose", "coord", "pt3d_68", "shapeparam", "avg_pose", "avg_coord", "avg_pt3d_68", "avg_shapeparam")}
    assert g["pose"].shape == (E, 64, 4) and g["pose"].dtype == np.float32
    back = np.broadcast_to(IDENTITY, (64, 2, 3))
    r = ER.ensemble_reduce(g["pose"], g["coord"], g["pt3d_68"].astype(np.float32), g["shapeparam"], back)
    # every row, sign included: the generator left no row whose pivot or member signs a rounding could change
    np.testing.assert_allclose(r["pose"], g["avg_pose"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["coord"], g["avg_coord"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r["pts"], g["avg_pt3d_68"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r["shape"], g["avg_shapeparam"], rtol=1e-12, atol=1e-12)
    assert r["stats"].shape == (64, 5) and np.all(r["stats"][:, 1] > 0.99) and np.all(r["stats"][:, 1] <= 1 + 1e-6)
    if E == 1:
        np.testing.assert_allclose(r["stats"][:, [0, 2, 3, 4]], 0.0, atol=1e-7)
    else:
        # members sit about sigma * sqrt(3) = 0.087 rad from their base rotation
        assert 0.02 < r["stats"][:, 0].mean() < 0.2
        np.testing.assert_allclose(r["stats"][:, 2:], g["coord"].astype(np.float64).std(0), rtol=1e-12)


def _transforms():
    ang, sc, sh = np.array([0.4, -2.6]), np.array([83.0, 0.7]), np.array([[212.5, 97.25], [40.0, -13.5]])
    rot = np.stack([np.stack([sc * np.cos(ang), -sc * np.sin(ang), sh[:, 0]], -1), np.stack([sc * np.sin(ang), sc * np.cos(ang), sh[:, 1]], -1)], 1)
    mirror = rot.copy()
    mirror[:, :, 0] *= -1.0  # x -> -x first: det < 0
    return {"rotated": rot, "mirrored": mirror}


@pytest.mark.parametrize("kind", ["rotated", "mirrored"])
def test_back_transformation_matches_apply_affine2d(kind):
    from trackertraincode.datatransformation.tensors.affinetrafo import FieldCategory, apply_affine2d
    from trackertraincode.neuralnets.affine2d import Affine2d

    back = _transforms()[kind].astype(np.float32)  # (Affine2d holds float32: both sides get the same float32 operands)
    assert np.all(np.sign(np.linalg.det(back[:, :, :2])) == (1 if kind == "rotated" else -1))
    rng = np.random.default_rng(7)
    E, B = 3, 2
    pose = rng.standard_normal((E, B, 4))
    pose = (pose / np.linalg.norm(pose, axis=-1, keepdims=True)).astype(np.float32)
    coord = rng.uniform(-1, 1, (E, B, 3)).astype(np.float32)
    pts = rng.uniform(-1, 1, (E, B, 68, 3)).astype(np.float32)
    # apply_affine2d computes in float32: a handful of roundings (<= 16) on terms of magnitude |a| + |b| + |t| (inputs lie in [-1, 1])
    tol = 16 * 2.0 ** -24 * np.abs(back).sum(-1).max(-1)  # per row of the batch
    pose_t, coord_t, pts_t = ER.back_transform(back, pose, coord, pts)
    tr = Affine2d(torch.from_numpy(back))
    for e in range(E):
        ref = {k: apply_affine2d(tr, k, torch.from_numpy(v[e]), c).numpy()
               for k, v, c in (("pose", pose, FieldCategory.quat), ("coord", coord, FieldCategory.xys), ("pt3d_68", pts, FieldCategory.points))}
        assert np.all(np.abs(pose_t[e] - ref["pose"]) <= 16 * 2.0 ** -24)
        assert np.all(np.abs(coord_t[e] - ref["coord"]) <= tol[:, None])
        assert np.all(np.abs(pts_t[e] - ref["pt3d_68"]) <= tol[:, None, None])
    if kind == "mirrored":  # the flip map moved landmarks: point 0 of the output is point 16 of the input
        b64, p64 = back.astype(np.float64), pts.astype(np.float64)
        x16 = b64[0, 0, 0] * p64[0, 0, 16, 0] + b64[0, 0, 1] * p64[0, 0, 16, 1] + b64[0, 0, 2]
        assert abs(pts_t[0, 0, 0, 0] - x16) < 1e-9 * np.abs(back[0]).sum()


def test_float32_form_runs_in_float32():
    rng = np.random.default_rng(3)
    pose = rng.standard_normal((2, 4, 4)).astype(np.float32)
    r = ER.ensemble_reduce(pose, rng.uniform(-1, 1, (2, 4, 3)), None, None, np.broadcast_to(IDENTITY, (4, 2, 3)), dtype=np.float32)
    assert all(r[k].dtype == np.float32 for k in ("pose", "coord", "stats")) and r["pts"] is None and r["shape"] is None
