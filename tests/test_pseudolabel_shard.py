"""datasets/shards.write_pseudolabels: the labels of an ensemble written into a shard that decode_pose_shard reads back."""
import os

import numpy as np
import pytest

from landmark_shards import write_shard
from util import GOLDEN

MINI = os.path.join(GOLDEN, "aflw2kmini.npz")  # JPEG blobs (image_bytes + image_lengths) and labels of its own


def _labels(n, seed=0, S=50):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, 4))
    return {"pose": (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(np.float32),
            "coord": rng.uniform(0.3, 400, (n, 3)).astype(np.float32),
            "pt3d_68": (rng.uniform(0.3, 500, (n, 68, 3)) * [1, 1, -0.2]).astype(np.float32),  # x, y inside a frame (see _one_ulp); z of either sign
            "shapeparam": rng.standard_normal((n, S)).astype(np.float32), "rot_spread": rng.uniform(0, 0.2, n).astype(np.float32),
            "mean_quat_norm": rng.uniform(0.4, 1, n).astype(np.float32), "coord_spread": rng.uniform(0, 3, (n, 3)).astype(np.float32)}


def _one_ulp(got, want):
    """Within one float32 ulp of each value.  The writer stores x - 0.5 and the decoder adds 0.5 again, both in float32.  For x >= 1 each step
    rounds by at most ulp(x) / 2 (x - 0.5 lies in the binade of x or the one below); for 0.25 <= x <= 1 the subtraction is exact (Sterbenz)
    and the sum returns x itself.  Below 0.25 px the difference sits near -0.5 and carries its rounding of 2^-25, many ulps of a tiny x, so
    the statement is one about coordinates from a quarter pixel up - where the xy of the labels drawn here (and of faces in a frame) lie."""
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


def test_round_trip_through_decode_pose_shard(tmp_path):
    from trackertraincode.datasets.shards import decode_pose_shard, write_pseudolabels

    raw = np.load(MINI)
    n = len(raw["image_lengths"])
    lab = _labels(n)
    dst = str(tmp_path / "labelled.npz")
    assert write_pseudolabels(MINI, dst, lab, overwrite=True) == dst
    s = decode_pose_shard(dst)
    for k in ("pose", "coord", "pt3d_68", "shapeparam"):
        _one_ulp(s[k], lab[k])
    assert np.array_equal(s["pose"], lab["pose"]) and np.array_equal(s["shapeparam"], lab["shapeparam"])  # no offset: bitwise
    assert np.array_equal(s["image"], decode_pose_shard(MINI)["image"])
    out = np.load(dst)
    # image blobs and every array the labels do not replace: byte-identical, same dtype
    replaced = {"quats", "coords", "pt3d_68", "shapeparams"}
    for k in raw.files:
        if k not in replaced:
            assert out[k].dtype == raw[k].dtype and out[k].tobytes() == raw[k].tobytes(), k
    assert np.array_equal(out["pseudolabel_rot_spread"], lab["rot_spread"]) and np.array_equal(out["pseudolabel_mean_quat_norm"], lab["mean_quat_norm"])
    assert np.array_equal(out["pseudolabel_coord_spread"], lab["coord_spread"])
    assert not any(k.startswith("pseudolabel") for k in s)  # decode_pose_shard reads the names of its map only
    assert np.array_equal(out["coords"][:, 2], lab["coord"][:, 2]) and np.array_equal(out["pt3d_68"][..., 2], lab["pt3d_68"][..., 2])


def test_labels_are_added_to_a_shard_without_them_and_unknown_arrays_pass_through(tmp_path):
    from trackertraincode.datasets.shards import decode_pose_shard, write_pseudolabels

    src = write_shard(tmp_path, "lm", "landmarks_2d", 7, 24, 32, seed=3)  # rois + pt2d_68 + `individual` (unknown to the label map)
    raw = dict(np.load(src))
    lab = _labels(7, seed=1)
    del lab["pt3d_68"], lab["shapeparam"]
    dst = str(tmp_path / "out.npz")
    write_pseudolabels(src, dst, lab)  # nothing is replaced, dst does not exist: no overwrite needed
    out = np.load(dst)
    assert set(out.files) == set(raw) | {"quats", "coords", "pseudolabel_rot_spread", "pseudolabel_mean_quat_norm", "pseudolabel_coord_spread"}
    for k, v in raw.items():
        assert out[k].dtype == v.dtype and out[k].tobytes() == v.tobytes(), k
    s = decode_pose_shard(dst)
    _one_ulp(s["coord"], lab["coord"])
    assert "pt3d_68" not in s and "shapeparam" not in s


@pytest.mark.parametrize("blobs", [True, False])
def test_keep_mask_is_applied_to_every_per_frame_array(tmp_path, blobs):
    from trackertraincode.datasets.shards import decode_pose_shard, write_pseudolabels

    src = MINI if blobs else write_shard(tmp_path, "pl", "pose_landmarks_2d", 9, 24, 32, seed=5)
    raw = dict(np.load(src))
    n = len(raw["image_lengths"]) if blobs else len(raw["images"])
    keep = np.arange(n) % 3 != 1
    lab = _labels(n, seed=2)
    dst = str(tmp_path / "kept.npz")
    write_pseudolabels(src, dst, lab, keep=keep, overwrite=True)
    out = np.load(dst)
    m = int(keep.sum())
    for k in out.files:
        if k != "image_bytes":
            assert len(out[k]) == m, k
    for k in set(raw) - {"quats", "coords", "pt3d_68", "shapeparams", "image_bytes"}:
        assert np.array_equal(out[k], raw[k][keep]), k
    s, full = decode_pose_shard(dst), decode_pose_shard(src)
    assert np.array_equal(s["image"][:, :, :full["image"].shape[2], :full["image"].shape[3]][..., :s["image"].shape[2], :s["image"].shape[3]],
                          full["image"][keep][..., :s["image"].shape[2], :s["image"].shape[3]])
    assert np.array_equal(s["image_size"], full["image_size"][keep])
    _one_ulp(s["coord"], lab["coord"][keep])
    assert np.array_equal(s["pose"], lab["pose"][keep]) and np.array_equal(out["pseudolabel_rot_spread"], lab["rot_spread"][keep])
    if blobs:
        assert int(out["image_lengths"].sum()) == len(out["image_bytes"])


def _listing(path):
    return sorted(os.listdir(str(path)))


def test_refusals_leave_nothing_behind(tmp_path):
    from trackertraincode.datasets.shards import write_pseudolabels

    # a sequence dataset: frames cannot be dropped
    src = write_shard(tmp_path, "seq", "pose", 6, 16, 16, seed=7)
    arrays = dict(np.load(src))
    arrays["sequence_starts"] = np.array([0, 4, 6], np.int64)
    np.savez(src, **arrays)
    before, content = _listing(tmp_path), open(src, "rb").read()
    lab = _labels(6, seed=4)
    keep = np.array([1, 1, 0, 1, 1, 1], bool)
    with pytest.raises(ValueError, match="sequence_starts"):
        write_pseudolabels(src, str(tmp_path / "dropped.npz"), lab, keep=keep, overwrite=True)
    # existing labels are not replaced without overwrite, neither is an existing destination
    with pytest.raises(FileExistsError, match="overwrite"):
        write_pseudolabels(src, str(tmp_path / "new.npz"), lab)
    with pytest.raises(FileExistsError, match="overwrite"):
        write_pseudolabels(src, src, lab)
    with pytest.raises(ValueError, match="rows"):
        write_pseudolabels(src, str(tmp_path / "short.npz"), {k: v[:5] for k, v in lab.items()}, overwrite=True)
    with pytest.raises(ValueError, match="pose"):
        write_pseudolabels(src, str(tmp_path / "nopose.npz"), {"coord": lab["coord"]}, overwrite=True)
    assert _listing(tmp_path) == before and open(src, "rb").read() == content  # no partial file, no temporary file, the source untouched
    # all frames kept: the sequence shard is labelled, in place
    write_pseudolabels(src, src, lab, keep=np.ones(6, bool), overwrite=True)
    assert _listing(tmp_path) == before
    out = np.load(src)
    assert np.array_equal(out["quats"], lab["pose"]) and np.array_equal(out["sequence_starts"], arrays["sequence_starts"])
