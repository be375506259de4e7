"""ttk_area_crop (csrc/area_crop.hip) and the `resample="area"` switch of the loaders against the float64 restatement of its definition
(tests/area_ref.py).  Criterion everywhere: max |kernel - restatement| <= 5e-2 grey levels (0..255), untrimmed - the project's bound for
the fp32 warp arithmetic (tests/test_augment.py); a float32 emulation of the definition stays within 8e-3.

Sources are seeded uniform-noise uint8 of 37 x 41, crops of N = 8 (ONE workgroup tile), B = 7, unless a case says otherwise.  The kernel
stages a tile's intermediate patch in LDS while it fits 8192 floats and loops directly beyond that: at N = 8 the patch is the whole
intermediate image, so views up to 90 pixels are staged and views from 91 pixels on take the direct loop - both sides are cases."""
import io
import os

import numpy as np
import pytest
import torch

import area_ref as AR
from util import GOLDEN

pytestmark = pytest.mark.gpu

TOL = 5e-2
N = 8
HS, WS = 37, 41


def _noise(B, seed, h=HS, w=WS):
    return np.random.default_rng(seed).integers(0, 256, (B, h, w), dtype=np.uint8)


def _launch(entry, src, trs, n, mul=1.0, add=0.0):
    """src [B, H, W] numpy uint8 / float32, trs [B, 2, 3] float32 -> [B, n, n] float32 (numpy)."""
    import trackertraincode._hip as H

    s, t = torch.from_numpy(np.ascontiguousarray(src)).cuda(), torch.from_numpy(np.ascontiguousarray(trs, np.float32)).cuda()
    B, hs, ws = s.shape
    out = torch.full((B, n, n), float("nan"), dtype=torch.float32, device="cuda")
    H.lib().call("ttk_area_crop" if entry == "area" else "ttk_affine_warp", H.ptr(s), int(s.dtype == torch.uint8), B, hs, ws, H.ptr(t),
                 H.ptr(out), n, mul, add)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _views_to_tr(views, n=N, angles=None):
    angles = [0.0] * len(views) if angles is None else angles
    return np.stack([AR.roi_transform(v, n, a) for v, a in zip(views, angles)])


def _check(src, trs, n=N):
    out = _launch("area", src, trs, n)
    ref = AR.area_crop_batch(src, trs, n)
    err = np.abs(out - ref).reshape(len(src), -1).max(1)
    print("max abs error per sample (grey levels):", np.array2string(err, precision=5))
    assert np.isfinite(out).all() and err.max() <= TOL, err
    return out


def _square(origins, size):
    return [(x, y, x + size, y + size) for x, y in origins]


INSIDE = [(0, 0), (3, 5), (17, 13), (11, 2), (1, 12), (16, 0), (8, 8)]  # 24- and 29-pixel views that stay inside 41 x 37 where they can


def test_integer_ratio():
    """(a) 24-pixel views: ratio 3, every output pixel averages whole source pixels."""
    _check(_noise(7, 10), _views_to_tr(_square(INSIDE, 24)))


def test_fractional_ratio():
    """(b) 29-pixel views: ratio 3.625, partial coverage on both edges of most windows."""
    _check(_noise(7, 11), _views_to_tr(_square([(x % 12, y % 8) for x, y in INSIDE], 29)))


def test_width_and_height_differ_by_one():
    """(c) Rx != Ry."""
    views = [(2, 3, 31, 31), (2, 3, 30, 32), (0, 0, 24, 25), (5, 1, 30, 25), (9, 7, 32, 29), (9, 7, 31, 30), (12, 8, 41, 36)]
    _check(_noise(7, 12), _views_to_tr(views))


def test_views_beyond_each_side_average_the_zeros_in():
    """(d) negative origin, beyond W, beyond H, corners, and a view with no source pixel at all."""
    views = [(-10, 5, 14, 29), (30, 5, 54, 29), (5, -9, 29, 15), (5, 25, 29, 49), (-7, -11, 22, 18), (25, 20, 54, 49), (60, 50, 84, 74)]
    src = _noise(7, 13)
    out = _check(src, _views_to_tr(views))
    assert (out[6] == 0).all()
    assert out[0][:, :3].max() == 0 and out[0][:, 4:].min() > 0  # columns 0-2 lie left of the image (10 of 24 pixels = 3.33 columns)


def test_ratio_nine_and_a_half_partly_outside():
    """(e) 76-pixel views around a 37 x 41 source: ratio 9.5."""
    views = [(-20, -18, 56, 58), (-40, -5, 36, 71), (0, 0, 76, 76), (-70, -70, 6, 6), (10, -30, 86, 46), (-17, -20, 59, 56), (-35, -39, 41, 37)]
    _check(_noise(7, 14), _views_to_tr(views))


def test_both_sides_of_the_lds_threshold_and_far_beyond():
    """The last staged size (90 x 90 = 8100 floats), the first direct one (91), and ratios 12.5, 15 and 50 through the direct loop; one of
    them rotated, one with unequal extents across the threshold (90 x 92 = 8280)."""
    views = [(-25, -27, 65, 63), (-25, -27, 66, 64), (-30, -30, 70, 70), (-40, -42, 80, 78), (-180, -181, 220, 219), (-25, -27, 65, 65), (-30, -30, 70, 70)]
    _check(_noise(7, 15), _views_to_tr(views, angles=[0, 0, 0, 0, 0, 0, 0.5]))


def test_magnification_is_the_bilinear_warp():
    """(f) 5-pixel views (and one of exactly N pixels): Rx = Ry = N, the window is one sample."""
    views = _square([(0, 0), (10, 12), (35, 30), (-2, 16), (20, -3), (38, 34)], 5) + [(4, 4, 12, 12)]
    src, trs = _noise(7, 16), _views_to_tr(views, angles=[0, 0.3, 0, 0, -0.5, 0, 0])
    out = _check(src, trs)
    warp = _launch("bilinear", src, trs, N)
    print("max |area - affine_warp|:", np.abs(out - warp).max())
    assert np.abs(out - warp).max() <= 1e-4


def test_rotated_views():
    """(g) +-30 degrees at ratios 2.4 (19-pixel views) and 3.6 (29-pixel views), inside and partly outside."""
    a = np.pi / 6
    views = _square([(9, 8), (9, 8), (14, 11), (-4, 20)], 19) + _square([(5, 4), (5, 4), (20, -6)], 29)
    _check(_noise(7, 17), _views_to_tr(views, angles=[a, -a, a, -a, a, -a, a]))


def _crop(resample, images, rois, n, codes=None, **kw):
    from trackertraincode.datasets.batch import Batch, Metadata
    from trackertraincode.datatransformation import GpuFocusRoiAugment
    from trackertraincode.datatransformation.batch.geometric import NoRoiRandomization

    B = len(images)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    batch = Batch(Metadata(images.shape[-2:][::-1], B, tag="x"), image=t(images[:, None]), roi=t(np.asarray(rois, np.float32)), **{k: t(v) for k, v in kw.items()})
    aug = GpuFocusRoiAugment(n, make_params=NoRoiRandomization(1.1 if n == 129 else 1.0), whiten=True, resample=resample,
                             flip_rot_p=None if codes is None else 0.01)
    out = aug(batch, fliprot_codes=None if codes is None else torch.tensor(codes))
    torch.cuda.synchronize()
    return out


def test_mirror_and_quarter_turn_codes():
    """(h) the six codes (rot_dir + 1) * 2 + do_flip composed into tr: each crop is the mirrored (code & 1) then turned (rot90 by
    1 - code // 2) crop of code 2 within 5e-3, and within the criterion of the restatement under the composed transform."""
    src = _noise(7, 18)
    rois = [(x, y, x + s, y + s) for (x, y), s in zip([(3, 5), (-6, 4), (20, 15), (0, 0), (12, 8), (15, -5), (6, 6)], [24, 29, 29, 24, 19, 29, 5])]
    crops = {}
    for code in range(6):
        out = _crop("area", src, rois, N, codes=[code] * 7)
        crops[code] = (out["image"].cpu().numpy()[:, 0] + 0.5) * 256.0
        ref = AR.area_crop_batch(src, out.transform.cpu().numpy(), N)
        assert np.abs(crops[code] - ref).max() <= TOL, code
    for code in range(6):
        base = torch.from_numpy(crops[2])
        want = torch.rot90(base.flip(2) if code & 1 else base, 1 - code // 2, (1, 2)).numpy()
        err = np.abs(crops[code] - want).max()
        print(f"code {code}: max |crop - permuted crop of code 2| = {err:.2e}")
        assert err <= 5e-3, code


def test_constant_source_and_source_types():
    """(i) a constant image under views inside it gives the constant (the weights sum to 1); uint8 and float32 sources: the same bits.
    The views keep one pixel from the border: a view that ENDS on it has its last sample at, say, v = 36.000004 in fp32 (the rounding of
    tr^-1, as in affine_warp_k), which gives the zero padding a weight of 4e-6 - 2e-4 grey levels here, far inside the criterion against
    the restatement, but not this case's subject."""
    views = _square([(1, 1), (3, 5), (16, 12), (11, 2)], 24) + _square([(1, 2), (7, 1), (11, 7)], 29)
    trs = _views_to_tr(views, angles=[0, 0, 0, 0, 0, 0, 0])
    const = _launch("area", np.full((7, HS, WS), 200, np.uint8), trs, N)
    print("constant 200: max deviation", np.abs(const - 200.0).max())
    assert np.abs(const - 200.0).max() <= 1e-4
    src = _noise(7, 19)
    mixed = _views_to_tr(views, angles=[0, 0.5, 0, -0.5, 0, 0.2, 0])
    assert np.array_equal(_launch("area", src, mixed, N), _launch("area", src.astype(np.float32), mixed, N))


def test_mixed_batch_is_bitwise_reproducible():
    """(j) integer ratio, ratio 9.5, magnification, rotation and the direct loop side by side in one launch, twice; mul / add applied."""
    a = np.pi / 6
    views = [(3, 5, 27, 29), (-20, -18, 56, 58), (10, 12, 15, 17), (9, 8, 28, 27), (5, 4, 34, 33), (-30, -30, 70, 70), (17, 13, 41, 37)]
    src, trs = _noise(7, 20), _views_to_tr(views, angles=[0, 0, 0, a, -a, 0, 0])
    _check(src, trs)
    one, two = _launch("area", src, trs, N, 1.0 / 256.0, -0.5), _launch("area", src, trs, N, 1.0 / 256.0, -0.5)
    assert np.array_equal(one, two)
    np.testing.assert_allclose((one + 0.5) * 256.0, AR.area_crop_batch(src, trs, N), rtol=0, atol=TOL)


def test_workload_geometry():
    """(k) N = 129 (5 x 17 tiles of 26 x 8 pixels) on two 450 x 450 frames, 263- and 248-pixel views, the second one rotated and leaving
    the frame."""
    src = _noise(2, 21, 450, 450)
    _check(src, _views_to_tr([(90, 110, 353, 373), (-30, 215, 218, 463)], 129, angles=[0.0, -np.pi / 6]), 129)


def _load_mini():
    from PIL import Image

    d = np.load(os.path.join(GOLDEN, "aflw2kmini.npz"))
    off, images = 0, []
    for n in d["image_lengths"]:
        img = np.array(Image.open(io.BytesIO(d["image_bytes"][off:off + int(n)].tobytes())))
        if img.ndim == 3:
            img = np.clip(np.rint((img.astype(np.float32) * np.array([0.299, 0.587, 0.114], np.float32)).sum(-1)), 0, 255).astype(np.uint8)
        images.append(img)
        off += int(n)
    return np.stack(images), d


def test_public_path_on_the_bundled_frames():
    """(l) GpuFocusRoiAugment(129, NoRoiRandomization(1.1), resample="area") on the 16 aflw2kmini frames: the crops are the restatement's,
    everything but the pixels is bitwise what "bilinear" gives, and the pixels do differ (> 0.3 grey levels rms on every frame; measured
    on the CPU for frames 0-3: >= 0.65)."""
    images, d = _load_mini()
    assert len(images) == 16
    lab = {"coord": d["coords"].astype(np.float32), "pose": d["quats"].astype(np.float32), "pt3d_68": d["pt3d_68"].astype(np.float32)}
    rois = d["rois"].astype(np.float32)
    area, bil = _crop("area", images, rois, 129, **lab), _crop("bilinear", images, rois, 129, **lab)
    assert torch.equal(area.view_roi, bil.view_roi) and torch.equal(area.transform, bil.transform)
    for k in ("coord", "pose", "roi", "pt3d_68"):
        assert torch.equal(area[k], bil[k]), k
    crops = (area["image"].cpu().numpy()[:, 0] + 0.5) * 256.0
    ref = AR.area_crop_batch(images, area.transform.cpu().numpy(), 129)
    err = np.abs(crops - ref).reshape(16, -1).max(1)
    print("max abs error per frame:", np.array2string(err, precision=5))
    assert err.max() <= TOL
    rms = np.sqrt((((bil["image"] - area["image"]).cpu().numpy()[:, 0] * 256.0) ** 2).reshape(16, -1).mean(1))
    print("rms |bilinear - area| per frame:", np.array2string(rms, precision=3))
    assert rms.min() > 0.3


def test_resident_loader_with_area_crops():
    """(m) two steps of the training loader (prefetch thread, side stream) with the area resampler."""
    from trackertraincode.datasets.resident import ResidentFrames, ResidentLoader
    from trackertraincode.datatransformation import GpuFocusRoiAugment
    from trackertraincode.pipelines import Tag

    g = torch.Generator().manual_seed(0)
    n = 60
    f = {"image": torch.randint(0, 256, (n, 1, 200, 180), generator=g, dtype=torch.uint8),
         "roi": torch.tensor([30.0, 40.0, 150.0, 160.0]) + torch.rand(n, 4, generator=g) * 8,
         "coord": torch.cat((90 + torch.randn(n, 2, generator=g), 50 + torch.rand(n, 1, generator=g)), -1),
         "pose": torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1),
         "pt3d_68": 90 + 20 * torch.randn(n, 68, 3, generator=g),
         "coord_convention_id": torch.zeros(n, dtype=torch.int32)}
    frames = ResidentFrames(Tag.POSE_WITH_LMKS_NO_SHAPE_PARAMS, {k: v.cuda() for k, v in f.items()})
    crop = GpuFocusRoiAugment(129, rotation_aug_angle=30.0, extension_factor=1.1, whiten=True, flip_rot_p=0.01, resample="area")
    steps = list(ResidentLoader([frames], [1.0], batchsize=32, steps_per_epoch=2, seed=1, crop=crop))
    assert len(steps) == 2
    for batches in steps:
        assert sum(b.meta.batchsize for b in batches) == 32
        for b in batches:
            m = b.meta.batchsize
            assert b["image"].shape == (m, 1, 129, 129) and b["image"].dtype == torch.float32
            assert torch.isfinite(b["image"]).all() and b["image"].min() >= -0.5 and b["image"].max() <= 0.5 and b["image"].std() > 0.05
            assert b["pt3d_68"].shape == (m, 68, 3) and torch.isfinite(b["pt3d_68"]).all() and torch.isfinite(b["coord"]).all()
