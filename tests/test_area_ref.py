"""The float64 restatement of the area-filtered crop (tests/area_ref.py) against independent formulations of the same average, and the
host surface of the `resample=` switch.  CPU only; the kernel against the restatement: tests/test_area_crop_gpu.py."""
import numpy as np
import pytest

import area_ref as AR
from oracle import augment as A


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.float64)


def _integral_average(roi, N):
    """Exact area average of a piecewise-constant image over N x N equal cells, through its integral: the cumulative sum is the integral
    at the integer positions and is linear between them (no coverage weights involved)."""
    def along(a):  # first axis
        R = a.shape[0]
        C = np.concatenate([np.zeros((1,) + a.shape[1:]), np.cumsum(a, 0)])
        edges = np.arange(N + 1) * (R / N)
        lo = np.minimum(np.floor(edges).astype(int), R - 1)
        at = C[lo] + (edges - lo)[:, None] * a[lo]
        return np.diff(at, axis=0) / (R / N)
    return along(along(roi).T).T


def _padded_roi(img, view):
    x0, y0, x1, y1 = view
    H, W = img.shape
    canvas = np.zeros((y1 - y0, x1 - x0))
    ys, xs = slice(max(y0, 0), min(y1, H)), slice(max(x0, 0), min(x1, W))
    canvas[ys.start - y0:ys.stop - y0, xs.start - x0:xs.stop - x0] = img[ys, xs]
    return canvas


def test_integer_ratio_is_the_block_mean():
    img = _noise(12, 12, 0)
    out = AR.area_crop(img, AR.roi_transform((0, 0, 12, 12), 4), 4)
    np.testing.assert_allclose(out, img.reshape(4, 3, 4, 3).mean((1, 3)), atol=1e-4)


@pytest.mark.parametrize("view", [(40, 60, 310, 330), (-35, 200, 226, 461), (301, -20, 541, 220)])
def test_aligned_roi_is_the_exact_average_of_the_zero_padded_roi(view):
    """Equal width and height (240 - 270 pixels for a 129-pixel crop, ratio 1.9 - 2.1), inside the image and beyond two of its sides."""
    img, N = _noise(450, 450, 1), 129
    out = AR.area_crop(img, AR.roi_transform(view, N), N)
    assert np.abs(out - _integral_average(_padded_roi(img, view), N)).max() <= 5e-3  # the float32 rounding of tr


def test_unequal_extents_and_each_axis_on_its_own():
    img, N, view = _noise(60, 70, 2), 8, (3, 5, 32, 33)  # 29 wide, 28 high
    I = AR.intermediate(img, AR.roi_transform(view, N), N)
    assert I.shape == (28, 29)
    np.testing.assert_allclose(AR.area_crop(img, AR.roi_transform(view, N), N), _integral_average(_padded_roi(img, view), N), atol=1e-3)


@pytest.mark.parametrize("N,R", [(4, 12), (8, 29), (8, 76), (129, 129), (129, 247), (129, 612)])
def test_every_weight_row_sums_to_one(N, R):
    w = AR.weights(N, R)
    assert w.shape == (N, R) and (w >= 0).all()
    np.testing.assert_allclose(w.sum(1), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(w.sum(0), N / R, rtol=0, atol=1e-12)  # every intermediate cell is used exactly once


def test_mirror_composed_into_tr_is_the_flipped_crop():
    img, N = _noise(450, 450, 3), 129
    for angle in (0.0, 0.4):
        tr = AR.roi_transform((70, 90, 331, 351), N, angle)
        mirror = np.array([[-1.0, 0.0, N], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
        trm = (mirror @ np.vstack([tr.astype(np.float64), [0, 0, 1]]))[:2].astype(np.float32)
        assert np.abs(AR.area_crop(img, trm, N) - AR.area_crop(img, tr, N)[:, ::-1]).max() <= 5e-3


def test_magnification_is_the_bilinear_crop():
    img, N = _noise(37, 41, 4), 8
    for view, angle in (((10, 12, 15, 17), 0.0), ((10, 12, 15, 17), -0.5), ((-2, 30, 4, 36), 0.0)):
        tr = AR.roi_transform(view, N, angle)
        assert AR.intermediate(img, tr, N).shape == (N, N)
        np.testing.assert_allclose(AR.area_crop(img, tr, N), A.warp_bilinear(img, tr, N), atol=1e-4)  # warp_bilinear returns float32


# ---- the host surface of the switch ------------------------------------------------------------------------------------------------

def test_crop_refuses_an_unknown_resampler():
    from trackertraincode.datatransformation import GpuFocusRoiAugment

    assert GpuFocusRoiAugment(129).resample == "bilinear"
    assert GpuFocusRoiAugment(129, resample="area").resample == "area"
    with pytest.raises(ValueError, match="resample"):
        GpuFocusRoiAugment(129, resample="nearest")


def test_loaders_refuse_an_unknown_resampler_before_any_file_is_opened(tmp_path):
    from trackertraincode import pipelines as P
    from trackertraincode.datasets.resident import ResidentEvalLoader

    with pytest.raises(ValueError, match="resample"):  # (an empty directory: a shard lookup would raise FileNotFoundError instead)
        P.make_pose_estimation_loaders(129, 8, [P.Id.AFLW2k3d], device="cpu", datadir=str(tmp_path), resample="nearest")
    with pytest.raises(ValueError, match="resample"):
        P.make_pose_estimation_loaders(129, 8, "synthetic", device="cpu", resample="nearest")
    with pytest.raises(ValueError, match="resample"):
        ResidentEvalLoader([], 8, device="cpu", resample="nearest")


def test_scripts_accept_the_resample_flag():
    from util import train_script

    p = train_script().make_parser()
    assert p.parse_args([]).resample == "bilinear"
    assert p.parse_args(["--resample", "area"]).resample == "area"
    with pytest.raises(SystemExit):
        p.parse_args(["--resample", "nearest"])
