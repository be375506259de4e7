"""Loader tables of the landmark-only / pose-only datasets (reference pipelines.py:72-156, 399-431, 590-595) and the shard decoder on the
shards such sets are converted to - CPU only."""
import numpy as np
import pytest
import torch

import landmark_shards as LS


def test_new_ids_resolve_to_shard_tag_weight_and_convention():
    import trackertraincode.pipelines as P

    expected = {
        P.Id.SYNFACE: ("microsoft_synface_100000-v1.1", P.Tag.ONLY_LANDMARKS_25D, 10_000.0, 0),
        P.Id.PANOPTIC_CMU: ("panoptic-v2", P.Tag.ONLY_POSE, 20_000.0, 1),
        P.Id._300VW: ("300vw", P.Tag.ONLY_LANDMARKS_2D, 5_000.0, 0),
        P.Id.LAPA: ("lapa", P.Tag.ONLY_LANDMARKS_2D, 20_000.0, 0),
        P.Id.WFLW_RELABEL: ("wflw_train", P.Tag.ONLY_LANDMARKS_2D, 10_000.0, 0),
    }
    for ds, (name, tag, weight, convention) in expected.items():
        got_name, got_tag, got_weight, subset = P._POSE_SHARDS[ds]
        assert (got_name, got_tag, got_weight) == (name, tag, weight), ds
        assert P._COORD_CONVENTION.get(got_name, 0) == convention, ds
        assert (subset is None) == (ds is not P.Id.PANOPTIC_CMU), ds
    # every set that was trainable before keeps its row and convention 0
    assert P._POSE_SHARDS[P.Id.REPO_300WLP] == ("reproduction_300wlp-v12", P.Tag.POSE_WITH_LANDMARKS, 60_000.0, None)
    assert P._POSE_SHARDS[P.Id.AFLW2k3d] == ("aflw2k", P.Tag.POSE_WITH_LANDMARKS, 1_000.0, (400, None))
    assert set(P._COORD_CONVENTION) == {"panoptic-v2"}
    assert set(P.Id) - set(P._POSE_SHARDS) == {P.Id.WIDER}


def test_panoptic_split_and_replicant_subset_are_the_references():
    import trackertraincode.pipelines as P

    N = LS.PANOPTIC_N
    test = np.random.RandomState(seed=1234567).choice(N, 1024, replace=False)
    train = np.setdiff1d(np.arange(N), test)
    got_train, got_test = P._POSE_SHARDS[P.Id.PANOPTIC_CMU][3](N), P._VALIDATION_SHARDS["panoptic"][1](N)
    assert np.array_equal(got_train, train) and np.array_equal(got_test, test)  # (the validation frames in `choice`'s order)
    assert not set(got_train) & set(got_test) and sorted(set(got_train) | set(got_test)) == list(range(N))
    assert P._VALIDATION_SHARDS["panoptic"][0] == "panoptic-v2"
    for n in (1001, 5000):
        assert np.array_equal(P._VALIDATION_SHARDS["replicantface-train"][1](n), np.random.default_rng(seed=42).integers(0, n - 1, size=1000))
    assert P._VALIDATION_SHARDS["replicantface-train"][0] == "replicant-face-v4-wider-100k"


def test_panoptic_train_and_validation_frames_of_a_shard(tmp_path):
    """Through the decoder and the frame selection, on host tensors: the planted pixel says which frame a row is."""
    import trackertraincode.pipelines as P
    from trackertraincode.datasets.shards import load_resident_frames

    N = LS.PANOPTIC_N
    path = LS.write_shard(tmp_path, "panoptic-v2", "pose", N, 16, 16, 4, roi_dtype=np.float16)
    frames = load_resident_frames(path, P.Tag.ONLY_POSE, "cpu", coord_convention_id=1)
    test = np.random.RandomState(seed=1234567).choice(N, 1024, replace=False)
    sub = P._select_frames(frames, P.panoptic_train_indices(N))
    assert len(sub) == N - 1024 and sub.tag is P.Tag.ONLY_POSE
    assert np.array_equal(LS.frame_index_of_pixels(sub.fields["image"].numpy()), np.setdiff1d(np.arange(N), test))
    assert torch.equal(sub.fields["roi"], frames.fields["roi"][torch.from_numpy(np.setdiff1d(np.arange(N), test))])
    assert int(sub.fields["coord_convention_id"].min()) == 1 == int(sub.fields["coord_convention_id"].max())
    # repeats and any order are fine (the Replicant-Face subset is drawn with replacement)
    again = P._select_frames(frames, [5, 3, 5])
    assert LS.frame_index_of_pixels(again.fields["image"].numpy()).tolist() == [5, 3, 5]
    with pytest.raises(IndexError):
        P._select_frames(frames, [N])
    # the validation set of the evaluation script: the held-out frames in `choice`'s order, convention id 1, stored boxes
    val = P.make_validation_dataset("panoptic", datadir=str(tmp_path))
    assert len(val) == 1024
    got = [(int(s["index"]), int(s["image"][0, 0]) + 256 * int(s["image"][0, 1]), int(s["coord_convention_id"])) for s in val]
    assert [g[0] for g in got] == test.tolist() and [g[1] for g in got] == test.tolist() and {g[2] for g in got} == {1}
    first = next(iter(val))
    assert set(first) == {"image", "roi", "pose", "coord", "individual", "index", "coord_convention_id"} and first["roi"].dtype == torch.float32


def test_replicantface_train_validation_set(tmp_path):
    import trackertraincode.pipelines as P

    n = 1003
    LS.write_shard(tmp_path, "replicant-face-v4-wider-100k", "pose_landmarks_noshape", n, 16, 16, 6)
    val = P.make_validation_loader("replicantface-train", use_head_roi=False, datadir=str(tmp_path))
    expected = np.random.default_rng(seed=42).integers(0, n - 1, size=1000)
    got = [(int(s["index"]), int(s["image"][0, 0]) + 256 * int(s["image"][0, 1])) for s in val]
    assert [g[0] for g in got] == expected.tolist() and [g[1] for g in got] == expected.tolist()
    assert "coord_convention_id" not in next(iter(val))  # convention 0: the samples look as those of every other set


def test_wider_is_refused_with_the_reason(tmp_path):
    import trackertraincode.pipelines as P

    with pytest.raises(NotImplementedError) as e:
        P.make_pose_estimation_loaders(129, 8, [P.Id.REPO_300WLP, P.Id.WIDER], datadir=str(tmp_path), device="cpu")
    msg = str(e.value)
    assert "FACE_DETECTION" in msg and "hasface" in msg and "enable_face_detector" in msg and "refused" in msg


@pytest.mark.parametrize("kind,roi_dtype", [("pose", np.float16), ("landmarks", np.float32), ("landmarks_2d", np.float32)])
def test_decode_pose_shard_of_partial_label_sets(tmp_path, kind, roi_dtype):
    from trackertraincode.datasets.shards import decode_pose_shard

    raw = LS.make_arrays(kind, 12, 16, 20, 7, roi_dtype=roi_dtype)
    path = LS.write_shard(tmp_path, "s", kind, 12, 16, 20, 7, roi_dtype=roi_dtype)
    assert raw["rois"].dtype == roi_dtype
    out = decode_pose_shard(path)
    mapped = {"rois": "roi", "quats": "pose", "coords": "coord", "pt3d_68": "pt3d_68", "pt2d_68": "pt2d_68"}
    assert set(out) == {"image", "image_size", "individual"} | {mapped[k] for k in LS.KINDS[kind]}
    for k in LS.KINDS[kind]:
        assert out[mapped[k]].dtype == np.float32, k
    # boxes and quaternions as stored (float16 boxes widened exactly); the xy of coord / pt3d_68 / pt2d_68 moved by half a pixel
    assert np.array_equal(out["roi"], raw["rois"].astype(np.float32))
    if kind == "pose":
        assert np.array_equal(out["pose"], raw["quats"])
        assert np.array_equal(out["coord"][:, :2], raw["coords"][:, :2] + np.float32(0.5)) and np.array_equal(out["coord"][:, 2], raw["coords"][:, 2])
    if kind == "landmarks":
        assert np.array_equal(out["pt3d_68"][..., :2], raw["pt3d_68"][..., :2] + np.float32(0.5))
        assert np.array_equal(out["pt3d_68"][..., 2], raw["pt3d_68"][..., 2])
    if kind == "landmarks_2d":
        assert np.array_equal(out["pt2d_68"], raw["pt2d_68"] + np.float32(0.5))
    plain = decode_pose_shard(path, half_pixel_offset=False)
    for k in LS.KINDS[kind]:
        assert np.array_equal(plain[mapped[k]], raw[k].astype(np.float32)), k
    assert out["image"].shape == (12, 1, 16, 20) and np.array_equal(out["image"][:, 0], raw["images"])
