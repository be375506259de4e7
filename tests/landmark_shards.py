"""Tiny generated shards for the tests of the landmark-only / pose-only datasets (test_landmark_sets*.py, test_landmark_step_gpu.py): seeded numpy,
raw `images` arrays (no JPEG), written to a temporary directory - nothing here is committed as data.

Every frame carries its own index in two pixels (row 0, columns 0 and 1: index % 256, index // 256) and - the loaders pass unknown fields
through - in `individual`.  The face box sits around the frame's centre; landmark 30 (the nose tip, its own partner under a mirror) is planted
at the centre of the face box."""
import os

import numpy as np

PANOPTIC_N = 1100  # frames of the generated Panoptic shard: more than the 1024 validation frames the reference holds out
CENTRE_LANDMARK = 30

# what a shard of each kind stores (HDF5 names, as oracle/tools/h5_to_npz.py keeps them)
KINDS = {
    "pose_landmarks": ("rois", "quats", "coords", "pt3d_68", "shapeparams"),
    "pose_landmarks_2d": ("rois", "quats", "coords", "pt3d_68", "pt2d_68", "shapeparams"),
    "pose_landmarks_noshape": ("rois", "quats", "coords", "pt3d_68"),
    "pose": ("rois", "quats", "coords"),
    "landmarks": ("rois", "pt3d_68"),
    "landmarks_2d": ("rois", "pt2d_68"),
}


def make_arrays(kind, n, h, w, seed, roi_dtype=np.float32, zero_z=False):
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)
    idx = np.arange(n)
    images[:, 0, 0], images[:, 0, 1] = idx % 256, idx // 256
    cx, cy = 0.5 * w + rng.uniform(-1, 1, n), 0.5 * h + rng.uniform(-1, 1, n)
    half = 0.25 * min(h, w) + rng.uniform(-0.5, 0.5, n)
    rois = np.stack([cx - half, cy - half, cx + half, cy + half], -1)
    out = {"images": images, "individual": idx.astype(np.int32)}
    names = KINDS[kind]
    if "rois" in names:
        out["rois"] = rois.astype(roi_dtype)
    if "quats" in names:
        q = rng.normal(size=(n, 4))
        out["quats"] = (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(np.float32)
    if "coords" in names:
        out["coords"] = np.stack([cx, cy, half], -1).astype(np.float32)
    pts = np.stack([cx[:, None] + rng.uniform(-1, 1, (n, 68)) * half[:, None], cy[:, None] + rng.uniform(-1, 1, (n, 68)) * half[:, None],
                    rng.uniform(-1, 1, (n, 68)) * half[:, None]], -1)
    box = out["rois"].astype(np.float64) if "rois" in out else rois  # the centre of the box AS STORED (float16 boxes round)
    pts[:, CENTRE_LANDMARK, 0], pts[:, CENTRE_LANDMARK, 1] = 0.5 * (box[:, 0] + box[:, 2]), 0.5 * (box[:, 1] + box[:, 3])
    if zero_z:
        pts[..., 2] = 0.0
    if "pt3d_68" in names:
        out["pt3d_68"] = pts.astype(np.float32)
    if "pt2d_68" in names:
        out["pt2d_68"] = pts[..., :2].astype(np.float32)
    if "shapeparams" in names:
        out["shapeparams"] = rng.normal(size=(n, 50)).astype(np.float32) * 0.5
    return out


def write_shard(datadir, name, kind, n, h, w, seed, **kw):
    arrays = make_arrays(kind, n, h, w, seed, **kw)
    path = os.path.join(str(datadir), name + ".npz")
    np.savez(path, **arrays)
    return path


def frame_index_of_pixels(image):
    """The planted index of frames [N, 1, H, W] (uint8, as stored)."""
    image = np.asarray(image)
    return image[:, 0, 0, 0].astype(np.int64) + 256 * image[:, 0, 0, 1].astype(np.int64)


def write_training_mix(datadir):
    """The shards of the four-set mix (+ the AFLW2000-3D stand-in every run validates on): two frame sizes, 30-50 frames each, the Panoptic one
    with 1100 frames of 16 x 16 and float16 boxes as the reference's converter stores them (dsprocess_panoptic.py:870)."""
    write_shard(datadir, "aflw2k", "pose_landmarks", 16, 40, 48, 1)
    write_shard(datadir, "reproduction_300wlp-v12", "pose_landmarks", 50, 40, 48, 2)
    write_shard(datadir, "microsoft_synface_100000-v1.1", "landmarks", 40, 32, 32, 3, zero_z=True)
    write_shard(datadir, "panoptic-v2", "pose", PANOPTIC_N, 16, 16, 4, roi_dtype=np.float16)
    write_shard(datadir, "lapa", "landmarks_2d", 30, 32, 32, 5)
    return str(datadir)
