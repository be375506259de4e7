"""Host side of the face-model fit without a GPU: the point weights in torch, the pixel <-> view mapping of FaceModelFitter.fit,
read_labels / write_face_fit (datasets/shards.py), the command line of scripts/fit_face_model.py, and the binding table."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import facefit_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
MINI = os.path.join(GOLDEN, "aflw2kmini.npz")
G = np.load(os.path.join(GOLDEN, "facefit.npz"))
U = 2.0 ** -24


def _fitter(**kw):
    from oracle.synth import synthetic_keypoint_buffers
    from trackertraincode.facemodel.fitting import FaceModelFitter

    return FaceModelFitter(*synthetic_keypoint_buffers(), device="cpu", **kw)


def _script():
    spec = importlib.util.spec_from_file_location("fit_face_model", os.path.join(REPO, "neuralnet-tracker-traincode_amd", "scripts", "fit_face_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_point_weights_in_torch_equal_the_restatement():
    """The torch function takes the heading from the rotation matrix, atan2(R02, R22), the restatement from scipy's as_euler: a few
    roundings of an angle of at most pi apart, divided by the 20 degree cutoff: 64 eps (weights are at most 1)."""
    from trackertraincode.facemodel.fitting import FACE_LEFT, FACE_RIGHT, facefit_point_weights, heading

    assert FACE_LEFT == R.FACE_LEFT and FACE_RIGHT == R.FACE_RIGHT
    pose = torch.from_numpy(G["wpose"])
    h = heading(pose).numpy()
    assert np.abs(h - np.array([R.heading(p) for p in G["wpose"]])).max() <= 8 * np.pi * 2.0 ** -53
    w = facefit_point_weights(pose, False)
    assert w.dtype == torch.float64 and tuple(w.shape) == (32, 68)
    assert np.abs(w.numpy() - G["w2d"]).max() <= 64 * 2.0 ** -53
    assert np.array_equal((w.numpy() == 0), (G["w2d"] == 0))
    assert np.array_equal(facefit_point_weights(pose, True).numpy(), G["w3d"])
    # float32 poses, as a shard stores them: the same function of the widened values
    w32 = facefit_point_weights(pose.float(), False).numpy()
    assert np.abs(w32 - np.stack([R.point_weights(p.astype(np.float64)) for p in G["wpose"].astype(np.float32)])).max() <= 64 * 2.0 ** -53


def test_view_roi_is_the_crops_and_labels_round_trip():
    """view_transform is GeneralFocusRoi.transform_for with scale 1.2 and no shift (whose integer view boxes tests/test_augment.py pins),
    and labels mapped into the view and back are the inputs.  Bound, float32 (u = 2^-24): in, x' = a x + t is 2 roundings on |a x| + |t|;
    back, x = a' x' + t' with the inverse's entries carrying 2 more; with |t / a| <= |x| + side (the view contains the face) that is
    <= 16 u (|x| + side) in pixels; the quaternion is multiplied by the unit z-rotation of angle atan2(-0, m11) = 0: 4 u.
    The size is scaled by Affine2d.scales = |R|_F / sqrt(2) each way, as the crop and Predictor.to_image_coordinates scale it.  The
    integer view rounds every corner on its own, so it can be a pixel off square: with r = height / width the two scales multiply to
    (r + 1 / r) / 2 instead of 1 - 1e-4 at 71 x 72 pixels.  That factor is the mapping's, stated here, and the round trip is held to
    it within 8 u."""
    from trackertraincode.datatransformation.batch.geometric import GeneralFocusRoi, RoiFocusRandomizationParameters
    from trackertraincode.datatransformation.tensors.affinetrafo import FieldCategory, apply_affine2d

    A = np.load(os.path.join(GOLDEN, "augment.npz"))
    roi = torch.from_numpy(A["roi"])
    B = len(roi)
    f = _fitter()
    view, to_norm = f.view_transform(roi)
    ref_view, _ = GeneralFocusRoi(None, 129).transform_for(roi, RoiFocusRandomizationParameters(torch.full((B,), 1.2), torch.zeros(B), torch.zeros(B, 2)))
    assert view.dtype == torch.int32 and torch.equal(view, ref_view)
    # (every corner is rounded on its own: the integer view is square up to a pixel)
    side = torch.maximum(view[:, 2] - view[:, 0], view[:, 3] - view[:, 1]).double().numpy()
    # the box's corners land on -1 / +1: the view size cancels
    corners = apply_affine2d(to_norm, "pt", view.float().reshape(B, 2, 2), FieldCategory.points).numpy()
    assert np.abs(corners - np.array([[-1.0, -1.0], [1.0, 1.0]])).max() <= 16 * U * (np.abs(view.numpy()).max() / side.min() * 2 + 1)
    rng = np.random.default_rng(3)
    centre = 0.5 * (roi[:, :2] + roi[:, 2:]).numpy()
    pts = (centre[:, None, :] + rng.uniform(-0.45, 0.45, (B, 68, 2)) * side[:, None, None]).astype(np.float32)
    coord = np.concatenate([centre, 0.3 * side[:, None]], -1).astype(np.float32)
    pose = rng.standard_normal((B, 4)).astype(np.float32)
    pose /= np.linalg.norm(pose, axis=-1, keepdims=True)
    back = to_norm.inv()
    rt = lambda k, v, c: apply_affine2d(back, k, apply_affine2d(to_norm, k, torch.from_numpy(v), c), c).numpy().astype(np.float64)
    bound_xy = 16 * U * (np.abs(pts).max(axis=(1, 2)) + side)
    assert np.all(np.abs(rt("pt2d_68", pts, FieldCategory.points) - pts).max(axis=(1, 2)) <= bound_xy)
    c2 = rt("coord", coord, FieldCategory.xys)
    r = (view[:, 3] - view[:, 1]).double().numpy() / (view[:, 2] - view[:, 0]).double().numpy()
    aniso = 0.5 * (r + 1.0 / r)
    assert np.all(np.abs(c2[:, :2] - coord[:, :2]).max(-1) <= bound_xy) and np.all(np.abs(c2[:, 2] - coord[:, 2] * aniso) <= 8 * U * coord[:, 2])
    assert aniso.max() < 1.0 + 5e-4
    assert np.abs(rt("pose", pose, FieldCategory.quat) - pose).max() <= 4 * U
    inside = apply_affine2d(to_norm, "pt2d_68", torch.from_numpy(pts), FieldCategory.points).numpy()
    assert np.abs(inside).max() <= 1.0  # landmarks within 0.45 sides of the centre (the corners round by half a pixel) are inside [-1, 1]


def test_fitter_construction_and_refusals(tmp_path):
    from oracle.synth import synthetic_keypoint_buffers
    from trackertraincode.facemodel.fitting import FaceModelFitter
    from trackertraincode.neuralnets.modelcomponents import DeformableHeadKeypoints

    kp, ev = synthetic_keypoint_buffers()
    f = _fitter()
    assert f.K == 10 and f.iters == (50, 100) and f.gtol == (1e-5, 5e-4) and not f.fit_3d_projections
    m = R.synthetic_model()  # the packaged mixture is the committed one, prepared the same way
    assert np.array_equal(f._ck.numpy(), m.ck) or np.abs(f._ck.numpy() - m.ck).max() <= 64 * 2.0 ** -53 * np.abs(m.ck).max()
    assert np.array_equal(f._mu.numpy(), m.mu)
    with pytest.raises(ValueError, match="all zero.*BFM blob"):
        FaceModelFitter(np.zeros((68, 3)), np.zeros((50, 68, 3)), device="cpu")
    head = DeformableHeadKeypoints()
    if not bool(head.keypts.any()):
        with pytest.raises(ValueError, match="BFM blob"):
            FaceModelFitter.from_module(head, device="cpu")
    head.set_basis(kp, ev)
    assert torch.equal(FaceModelFitter.from_module(head, device="cpu")._ev, torch.from_numpy(ev))
    with pytest.raises(ValueError, match=r"\[68,3\]"):
        FaceModelFitter(kp[:60], ev, device="cpu")
    with pytest.raises(ValueError, match="iters"):
        FaceModelFitter(kp, ev, device="cpu", gtol=(0.0, 1e-3))
    ck = tmp_path / "net.ckpt"
    torch.save({"state_dict": {"landmarks.deformablekeypoints.keypts": torch.from_numpy(kp), "landmarks.deformablekeypoints.keyeigvecs": torch.from_numpy(ev)},
                "class_name": "NetworkWithPointHead", "config": {}}, ck)
    assert torch.equal(FaceModelFitter.from_checkpoint(str(ck), device="cpu")._kp, torch.from_numpy(kp))
    torch.save({"state_dict": {"w": torch.zeros(1)}, "class_name": "x", "config": {}}, ck)
    with pytest.raises(ValueError, match="landmark head"):
        FaceModelFitter.from_checkpoint(str(ck), device="cpu")


def test_read_labels_is_decode_pose_shard_without_the_images():
    from trackertraincode.datasets.shards import decode_pose_shard, read_labels

    for off in (True, False):
        full, lab = decode_pose_shard(MINI, off), read_labels(MINI, off)
        assert set(lab) == set(full) - {"image", "image_size"} and "pose" in lab and "roi" in lab
        for k, v in lab.items():
            assert v.dtype == full[k].dtype and np.array_equal(v, full[k]), k


def _fit_labels(n, rng):
    return {"pose": rng.standard_normal((n, 4)).astype(np.float32), "coord": rng.uniform(10, 200, (n, 3)).astype(np.float32),
            "pt3d_68": rng.uniform(0, 300, (n, 68, 3)).astype(np.float32), "shapeparam": rng.standard_normal((n, 50)).astype(np.float32),
            "objective": rng.uniform(0, 1, n), "status": rng.integers(0, 4, n), "iterations": rng.integers(0, 100, (n, 2))}


def test_write_face_fit_round_trips_and_refuses(tmp_path):
    from trackertraincode.datasets.shards import decode_pose_shard, read_labels, write_face_fit

    n = len(np.load(MINI)["image_lengths"])
    lab = _fit_labels(n, np.random.default_rng(0))
    dst = str(tmp_path / "fit.npz")
    with pytest.raises(FileExistsError, match="already has"):  # the mini shard carries quats / coords / pt3d_68 / shapeparams of its own
        write_face_fit(MINI, dst, lab)
    assert not os.path.exists(dst)
    write_face_fit(MINI, dst, lab, overwrite=True)
    back, raw, src = decode_pose_shard(dst), np.load(dst), np.load(MINI)
    for k in ("pose", "coord", "pt3d_68", "shapeparam"):
        assert np.array_equal(back[k], lab[k]) or np.abs(back[k] - lab[k]).max() <= 2 * U * np.abs(lab[k]).max(), k  # (- 0.5 + 0.5 in float32)
    assert np.array_equal(raw["coords"][:, :2], lab["coord"][:, :2] - np.float32(0.5)) and np.array_equal(raw["coords"][:, 2], lab["coord"][:, 2])
    assert raw["facefit_status"].dtype == np.int32 and np.array_equal(raw["facefit_status"], lab["status"])
    assert raw["facefit_iterations"].dtype == np.int32 and np.array_equal(raw["facefit_iterations"], lab["iterations"])
    assert raw["facefit_objective"].dtype == np.float32 and np.array_equal(raw["facefit_objective"], lab["objective"].astype(np.float32))
    assert np.array_equal(raw["image_bytes"], src["image_bytes"]) and np.array_equal(raw["rois"], src["rois"])
    assert not [f for f in os.listdir(tmp_path) if f.startswith(".facefit-")]
    with pytest.raises(FileExistsError, match="exists"):
        write_face_fit(MINI, dst, lab)
    keep = np.arange(n) % 3 != 0
    write_face_fit(MINI, dst, lab, keep=keep, overwrite=True)
    kept = read_labels(dst)
    assert len(kept["pose"]) == int(keep.sum()) and np.array_equal(kept["shapeparam"], lab["shapeparam"][keep])
    assert len(decode_pose_shard(dst)["image"]) == int(keep.sum())
    with pytest.raises(ValueError, match="labels need 'pose', 'coord', 'pt3d_68', 'shapeparam'"):
        write_face_fit(MINI, dst, {k: lab[k] for k in ("pose", "coord")}, overwrite=True)
    with pytest.raises(ValueError, match="may hold"):
        write_face_fit(MINI, dst, dict(lab, rot_spread=np.zeros(n)), overwrite=True)
    with pytest.raises(ValueError, match="rows"):
        write_face_fit(MINI, dst, dict(lab, status=np.zeros(n - 1)), overwrite=True)
    with pytest.raises(ValueError, match="keep has shape"):
        write_face_fit(MINI, dst, lab, keep=keep[:-1], overwrite=True)


def test_write_pseudolabels_keeps_its_refusal_text(tmp_path):
    from trackertraincode.datasets.shards import write_pseudolabels

    with pytest.raises(ValueError, match="labels need 'pose' and 'coord' and may hold"):
        write_pseudolabels(MINI, str(tmp_path / "x.npz"), {"pose": np.zeros((16, 4))})
    with pytest.raises(ValueError, match="may hold"):
        write_pseudolabels(MINI, str(tmp_path / "x.npz"), {"pose": np.zeros((16, 4)), "coord": np.zeros((16, 3)), "status": np.zeros(16)})


def test_script_parser_and_refusals(tmp_path):
    S = _script()
    a = S.make_parser().parse_args(["in.npz", "--basis", "b.npz"])
    assert (a.batchsize, a.output, a.fit_3d_projections, a.max_objective, a.drop_unconverged, a.dryrun, a.overwrite, a.device) == \
        (4096, None, False, None, False, False, False, "cuda")
    a = S.make_parser().parse_args(["in.npz", "--output", "o.npz", "--basis-from-checkpoint", "c.ckpt", "--fit-3d-projections", "-b", "7",
                                    "--max-objective", "0.5", "--drop-unconverged", "--dryrun", "-f", "--device", "cpu"])
    assert (a.batchsize, a.output, a.basis_from_checkpoint, a.fit_3d_projections, a.max_objective, a.drop_unconverged, a.dryrun, a.overwrite) == \
        (7, "o.npz", "c.ckpt", True, 0.5, True, True, True)
    out = str(tmp_path / "o.npz")
    with pytest.raises(SystemExit, match="exists"):  # the default output is the input
        S.main([MINI, "--basis", "b.npz"])
    with pytest.raises(SystemExit, match="--dryrun"):
        S.main([MINI, "--basis", "b.npz", "--dryrun", "-f"])
    with pytest.raises(SystemExit, match="exactly one"):
        S.main([MINI, "--output", out])
    with pytest.raises(SystemExit, match="exactly one"):
        S.main([MINI, "--output", out, "--basis", "b.npz", "--basis-from-checkpoint", "c.ckpt"])
    with pytest.raises(SystemExit, match="batchsize"):
        S.main([MINI, "--output", out, "--basis", "b.npz", "-b", "0"])
    with pytest.raises(SystemExit, match=r"lacks \['pt2d_68'\]"):  # the mini shard has 3-D landmarks only
        S.main([MINI, "--output", out, "--basis", "b.npz"])
    stripped = str(tmp_path / "stripped.npz")
    np.savez(stripped, **{k: v for k, v in np.load(MINI).items() if k not in ("quats", "coords")})
    with pytest.raises(SystemExit, match=r"lacks \['quats', 'coords'\]"):
        S.main([stripped, "--output", out, "--basis", "b.npz", "--fit-3d-projections"])
    bad_basis = str(tmp_path / "basis.npz")
    np.savez(bad_basis, keypts=np.zeros((68, 3), np.float32))
    with pytest.raises(SystemExit, match="keyeigvecs"):
        S.main([MINI, "--output", out, "--basis", bad_basis, "--fit-3d-projections", "--device", "cpu"])
    assert not os.path.exists(out)


def test_binding_table_and_header_list_both_entry_points():
    import trackertraincode._hip as H

    hdr = open(os.path.join(REPO, "include", "ttk.h")).read()
    assert H.ABI_VERSION == 38 and re.search(r"#define TTK_ABI_VERSION 38\b", hdr)
    for name, nargs in (("ttk_facefit_objective", 13), ("ttk_facefit", 19)):
        assert len(H._SIGNATURES[name]) == nargs
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr).group(1)
        assert decl.count(",") + 1 == nargs + 1  # + the stream
    assert H._SIGNATURES["ttk_facefit"][11] is H._D and H._SIGNATURES["ttk_facefit"][13] is H._D
