"""2-D landmarks (`pt2d_68`, [B, 68, 2]) through the label kernel (ttk_affine_labels2d, csrc/warp.hip) and the crop (GpuFocusRoiAugment).

Tolerances are the ones tests/test_augment.py applies to `pt3d_68`: the kernel against the reference's values in the crop's [-1, 1] coordinates
rtol 1e-4 / atol 2e-5 (test_hip_augment_matches_reference_golden), in pixel coordinates (N = 0) rtol 1e-5 / atol 1e-4 (its mirrored
transform), a float64 restatement against the reference's values rtol 1e-4 / atol 1e-5 (test_oracle_transforms_and_warp_match_reference).
Observed maxima on the MI355X: profiles/landmark_sets.txt."""
import math
import os

import numpy as np
import pytest
import torch

from util import GOLDEN

N = 129
G2 = dict(np.load(os.path.join(GOLDEN, "augment_pt2d.npz")))


def keypoints2d_f64(m, pts):
    """Float64 restatement of the reference's 2-D point path: transform_points (tensors/affinetrafo.py:37-52: the 2 x 3 matrix applied to
    every point, `affinevecmul`) and transform_keypoints (:61-72, its 2-D branch :70-71: when the transform mirrors, det < 0, the outputs are
    re-ordered by the 68-point flip map, out[p] = transformed[flip_map[p]])."""
    from trackertraincode.facemodel.keypoints68 import flip_map

    m, pts = np.asarray(m, np.float64), np.asarray(pts, np.float64)
    out = pts @ m[:, :2].T + m[:, 2]
    if m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0] < 0.0:
        out = out[np.asarray(flip_map)]
    return out


def normalisation_f64(n):
    return np.array([[2.0 / n, 0.0, -1.0], [0.0, 2.0 / n, -1.0]])


def fliprot_f64(code, n):
    """The six exact point maps of the N x N crop, (rot_dir + 1) * 2 + do_flip: a mirror x -> N - x first, then a quarter turn about the centre."""
    rot_dir, do_flip = code // 2 - 1, code % 2
    F = np.array([[-1.0, 0.0, n], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) if do_flip else np.eye(3)
    if rot_dir:
        c = 0.5 * n  # (x, y) - c -> (-s (y - c), s (x - c)), s = rot_dir
        R = np.array([[0.0, -rot_dir, c + rot_dir * c], [rot_dir, 0.0, c - rot_dir * c], [0.0, 0.0, 1.0]], np.float64)
        F = R @ F
    return F


def test_restatement_matches_reference_fixture():
    """CPU: the float64 restatement, step by step as the reference's loaders apply it, against the reference's own outputs (all six draws)."""
    assert sorted(set(G2["code"].tolist())) == list(range(6))
    worst = 0.0
    for tr, code, pts, in_crop, out in zip(G2["tr"], G2["code"], G2["pt2d_68"], G2["crop_pt2d_68"], G2["out_pt2d_68"]):
        a = keypoints2d_f64(tr, pts)
        np.testing.assert_allclose(a, in_crop, rtol=1e-4, atol=1e-4)  # pixels (the tolerance of the mirrored pixel-space rows of test_augment.py)
        b = keypoints2d_f64(normalisation_f64(N), keypoints2d_f64(fliprot_f64(int(code), N)[:2], a))
        np.testing.assert_allclose(b, out, rtol=1e-4, atol=1e-5)
        worst = max(worst, float(np.abs(b - out).max()))
    print(f"restatement vs reference fixture: max abs error {worst:.3e}")


def _rot(angle_deg, scale, shift):
    a = math.radians(angle_deg)
    return [[scale * math.cos(a), -scale * math.sin(a), shift[0]], [scale * math.sin(a), scale * math.cos(a), shift[1]]]


def _composed(code, tr23):
    from trackertraincode.datatransformation import GpuFocusRoiAugment

    F = GpuFocusRoiAugment(N, flip_rot_p=0.01).fliprot_table()[code]
    return (F @ torch.cat((torch.tensor(tr23, dtype=torch.float32), torch.tensor([[0.0, 0.0, 1.0]])), 0))[:2].tolist()


def _transform_sets():
    base = _rot(30.0, 1.3, (-12.0, 7.0))
    return {
        "plain": [[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], base, _rot(-30.0, 0.8, (9.0, 21.0))],
        "mirrored": [[[-1.1, 0.0, 100.0], [0.0, 1.1, -3.0]], _composed(0, base), _composed(5, base)],  # det < 0, det > 0 (turn), det < 0 (turn + mirror)
    }


def _labels(seed, B=3):
    g = torch.Generator().manual_seed(seed)
    pts = torch.cat((torch.rand(B, 68, 2, generator=g) * 80 + 10, torch.rand(B, 68, 1, generator=g) * 40 - 20), -1)
    coord = torch.cat((torch.rand(B, 2, generator=g) * 30 + 30, torch.rand(B, 1, generator=g) * 15 + 15), -1)
    pose = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=-1)
    roi = torch.cat((torch.rand(B, 2, generator=g) * 20 + 10, torch.rand(B, 2, generator=g) * 30 + 60), -1)
    return {k: v.cuda().contiguous() for k, v in dict(coord=coord, pose=pose, roi=roi, pt3d_68=pts).items()}


def _launch(entry, tr, n, lab, pts2d):
    import trackertraincode._hip as H

    coord, pose, roi = lab["coord"].clone(), lab["pose"].clone(), lab["roi"].clone()
    out3 = torch.full_like(lab["pt3d_68"], float("nan"))
    args = [H.ptr(tr), tr.shape[0], n, H.ptr(coord), H.ptr(pose), H.ptr(roi), H.ptr(lab["pt3d_68"]), H.ptr(out3)]
    out2 = None
    if entry == "ttk_affine_labels2d":
        out2 = torch.full_like(pts2d, float("nan")) if pts2d is not None else None
        args += [H.ptr(pts2d), H.ptr(out2)]
    H.lib().call(entry, *args)
    torch.cuda.synchronize()
    return dict(coord=coord, pose=pose, roi=roi, pt3d_68=out3, pt2d_68=out2)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N, 0])
@pytest.mark.parametrize("which", ["plain", "mirrored"])
def test_label_kernel_2d_field(which, n):
    trs = _transform_sets()[which]
    tr = torch.tensor(trs, dtype=torch.float32).cuda().contiguous()
    lab = _labels(7 if which == "plain" else 8)
    pts2d = lab["pt3d_68"][..., :2].contiguous()
    with2d = _launch("ttk_affine_labels2d", tr, n, lab, pts2d)
    null2d = _launch("ttk_affine_labels2d", tr, n, lab, None)
    old = _launch("ttk_affine_labels", tr, n, lab, None)
    # x, y of the 2-D field are BITWISE those of the 3-D field of the same launch
    assert torch.equal(with2d["pt2d_68"], with2d["pt3d_68"][..., :2])
    # the other fields do not notice the 2-D field: null pointers, and the entry point without them, give the same bits
    for k in ("coord", "pose", "roi", "pt3d_68"):
        assert torch.equal(with2d[k], null2d[k]) and torch.equal(null2d[k], old[k]), k
    # against the float64 restatement of the reference
    got = with2d["pt2d_68"].cpu().numpy()
    tol = dict(rtol=1e-4, atol=2e-5) if n else dict(rtol=1e-5, atol=1e-4)
    worst = 0.0
    for b in range(tr.shape[0]):
        m = tr[b].cpu().numpy()
        ref = keypoints2d_f64(m, pts2d[b].cpu().numpy())
        if n:
            ref = keypoints2d_f64(normalisation_f64(n), ref)
        np.testing.assert_allclose(got[b], ref, err_msg=f"{which} sample {b}", **tol)
        worst = max(worst, float(np.abs(got[b] - ref).max()))
    print(f"ttk_affine_labels2d vs float64 restatement, {which}, N={n}: max abs error {worst:.3e}")


@pytest.mark.gpu
def test_label_kernel_2d_field_against_reference_fixture():
    """The kernel on the reference's cases: the crop transform composed with the drawn mirror / quarter turn (as GpuFocusRoiAugment composes
    them), 2-D landmarks only - every other pointer null."""
    import trackertraincode._hip as H

    tr = torch.tensor([_composed(int(c), t.tolist()) for t, c in zip(G2["tr"], G2["code"])], dtype=torch.float32).cuda().contiguous()
    pts = torch.from_numpy(G2["pt2d_68"]).cuda().contiguous()
    out = torch.full_like(pts, float("nan"))
    H.lib().call("ttk_affine_labels2d", H.ptr(tr), tr.shape[0], N, None, None, None, None, None, H.ptr(pts), H.ptr(out))
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), G2["out_pt2d_68"], rtol=1e-4, atol=2e-5)
    print(f"ttk_affine_labels2d vs reference fixture: max abs error {float(np.abs(out.cpu().numpy() - G2['out_pt2d_68']).max()):.3e}")
    # the aliasing rule of the 3-D field holds for the 2-D one: one buffer for both is refused before any launch
    with pytest.raises(RuntimeError, match="pts2d_in/pts2d_out"):
        H.lib().call("ttk_affine_labels2d", H.ptr(tr), tr.shape[0], N, None, None, None, None, None, H.ptr(pts), H.ptr(pts))


@pytest.mark.gpu
def test_crop_transforms_pt2d_68_and_leaves_the_rest_alone():
    from trackertraincode.datasets.batch import Batch, Metadata
    from trackertraincode.datatransformation import GpuFocusRoiAugment

    B, S = 12, 96
    g = torch.Generator().manual_seed(3)
    image = torch.randint(0, 256, (B, 1, S, S), dtype=torch.uint8, generator=g).cuda()
    lab = _labels(9, B)
    lab["roi"] = (torch.tensor([[24.0, 24.0, 72.0, 70.0]]) + torch.randn(B, 4, generator=g) * 2).cuda()
    codes = torch.arange(B) % 6  # every (rot_dir, do_flip) draw twice
    fields = dict(image=image, **lab, shapeparam=torch.randn(B, 50, generator=g).cuda())

    def crop(with2d, seed=21):
        data = dict(fields)
        if with2d:
            data["pt2d_68"] = lab["pt3d_68"][..., :2].contiguous()
        aug = GpuFocusRoiAugment(N, rotation_aug_angle=30.0, flip_rot_p=0.5)
        return aug(Batch(Metadata(S, B, tag="x"), data), generator=torch.Generator().manual_seed(seed), fliprot_codes=codes)

    a, b = crop(True), crop(False)
    assert a["pt2d_68"].shape == (B, 68, 2) and torch.equal(a["pt2d_68"], a["pt3d_68"][..., :2])
    assert not torch.equal(a["pt2d_68"], lab["pt3d_68"][..., :2])  # (it left source pixels)
    assert float(a["pt2d_68"].abs().max()) < 4.0                    # crop coordinates, not pixels
    assert set(a.keys()) == set(b.keys()) | {"pt2d_68"}
    for k in b.keys():  # a batch without the field: the same bits as one with it, in every other field (unknown ones pass through)
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a.transform, b.transform) and torch.equal(a["shapeparam"], fields["shapeparam"])
    with pytest.raises(ValueError, match="pt2d_68"):
        GpuFocusRoiAugment(N)(Batch(Metadata(S, B, tag="x"), dict(fields, pt2d_68=lab["pt3d_68"].contiguous())))
