"""The landmark-only / pose-only datasets through make_pose_estimation_loaders on the GPU: a four-set mix over generated shards
(tests/landmark_shards.py) with four Tags, two frame sizes, float16 boxes, an index-subset train split and a second coordinate convention."""
import numpy as np
import pytest
import torch

import landmark_shards as LS

pytestmark = pytest.mark.gpu

SEED = 3  # (with the default weights 60 : 10 : 20 : 20 both steps of this seed draw from all four sets)
COMMON = {"image", "roi", "coord_convention_id", "individual"}  # the crop, its box, the convention id; `individual` is an unknown field passed through


def _fields(P):
    return {P.Tag.POSE_WITH_LANDMARKS: COMMON | {"pose", "coord", "pt3d_68", "shapeparam"}, P.Tag.ONLY_LANDMARKS_25D: COMMON | {"pt3d_68"},
            P.Tag.ONLY_POSE: COMMON | {"pose", "coord"}, P.Tag.ONLY_LANDMARKS_2D: COMMON | {"pt2d_68"}}


@pytest.fixture(scope="module")
def mix(tmp_path_factory):
    """Two iterations of the four-set mix from device-placed and from host-placed frames (computed once, read by every test below)."""
    import trackertraincode.pipelines as P

    datadir = LS.write_training_mix(tmp_path_factory.mktemp("landmark_sets"))
    saved = P._TEST_SHARD
    P._TEST_SHARD = ("aflw2k", P.Tag.POSE_WITH_LANDMARKS, (0, 8))  # (the stand-in has 16 frames)
    try:
        ids = [P.Id.REPO_300WLP, P.Id.SYNFACE, P.Id.PANOPTIC_CMU, P.Id.LAPA]
        out = {"datadir": datadir}
        for placement in ("device", "host"):
            # rotation_aug_angle=0: with the 30 degree turn a face-box centre that the crop shifted by its full range can leave the crop by a few
            # per cent of its side; axis-aligned crops keep it inside by 0.2 of the box (the shift leaves that much of the box in view)
            train, test, total = P.make_pose_estimation_loaders(129, 16, ids, datadir=datadir, device="cuda", seed=SEED, steps_per_epoch=2,
                                                                rotation_aug_angle=0.0, frames_on=placement)
            torch.manual_seed(11)  # the Gaussian-noise augmentation draws from the global device generator
            steps = [[(b.meta.tag, {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}) for b in step] for step in train]
            out[placement] = dict(train=train, steps=steps, total=total)
    finally:
        P._TEST_SHARD = saved
    return out


def test_four_set_mix_fields_conventions_and_crop_coordinates(mix):
    import trackertraincode.pipelines as P

    steps, train = mix["device"]["steps"], mix["device"]["train"]
    assert len(steps) == 2 and mix["device"]["total"] == 50 + 40 + (LS.PANOPTIC_N - 1024) + 30
    expected = _fields(P)
    held_out = set(P.panoptic_test_indices(LS.PANOPTIC_N).tolist())
    for step in steps:
        assert {tag for tag, _ in step} == set(expected) and sum(int(b["image"].shape[0]) for _, b in step) == 16
        for tag, b in step:
            n = int(b["image"].shape[0])
            assert set(b) == expected[tag], (tag, sorted(b))
            assert b["image"].shape == (n, 1, 129, 129) and b["image"].dtype == torch.float32 and b["roi"].dtype == torch.float32
            assert all(v.is_cuda and v.shape[0] == n for v in b.values())
            # coord_convention_id: 1 in Panoptic rows, 0 everywhere else
            assert b["coord_convention_id"].tolist() == [1 if tag is P.Tag.ONLY_POSE else 0] * n
            if tag is P.Tag.ONLY_POSE:  # no row from a validation frame
                assert not set(b["individual"].tolist()) & held_out
            for k in ("pt3d_68", "pt2d_68"):
                if k in b:
                    assert b[k].shape == (n, 68, 3 if k == "pt3d_68" else 2)
                    xy = b[k][..., :2]
                    assert float(xy.abs().max()) < 3.0, k                        # crop coordinates, not source pixels (those reach 40)
                    assert float(xy[:, LS.CENTRE_LANDMARK].abs().max()) <= 1.0, k  # the landmark planted at the face-box centre is inside the crop
            if tag is P.Tag.ONLY_LANDMARKS_25D:
                assert float(b["pt3d_68"][..., 2].abs().max()) == 0.0  # the zero padding stays zero
            assert float(b["roi"].abs().max()) < 3.0
    # the resident Panoptic set holds exactly the train frames: the index planted in two pixels of every frame says so
    sets = {d.tag: d for d in train.datasets}
    assert len(train.datasets) == 4 and len(sets) == 4
    pan = sets[P.Tag.ONLY_POSE]
    assert np.array_equal(LS.frame_index_of_pixels(pan.fields["image"].cpu().numpy()), P.panoptic_train_indices(LS.PANOPTIC_N))
    assert pan.fields["roi"].dtype == torch.float32 and pan.fields["image"].is_cuda
    assert set(sets[P.Tag.ONLY_LANDMARKS_2D].fields) == {"image", "roi", "pt2d_68", "individual", "coord_convention_id"}


def test_four_set_mix_from_host_frames_is_bitwise_the_same(mix):
    dev, host = mix["device"], mix["host"]
    assert all(d.on_host and d.fields["image"].is_pinned() for d in host["train"].datasets) and not any(d.on_host for d in dev["train"].datasets)
    assert dev["total"] == host["total"] and len(dev["steps"]) == len(host["steps"]) == 2
    for sd, sh in zip(dev["steps"], host["steps"]):
        assert [t for t, _ in sd] == [t for t, _ in sh]
        for (_, x), (_, y) in zip(sd, sh):
            assert x.keys() == y.keys()
            for k in x:
                assert x[k].device == y[k].device and torch.equal(x[k], y[k]), k


def test_validation_names_serve_the_held_out_frames_in_order(mix, tmp_path):
    """The two validation sets with an index subset, as scripts/evaluate_pose_network.py --ds reaches them (make_validation_loader), through
    eval.Predictor's sample loop: the order of the samples is the order of the reference's index draws."""
    import trackertraincode.pipelines as P
    from trackertraincode import utils

    samples = P.make_validation_loader("panoptic", return_single_samples=True, datadir=mix["datadir"])
    expected = P.panoptic_test_indices(LS.PANOPTIC_N)
    got = []
    for chunk in utils.iter_batched(samples, 256):
        idx = torch.stack([s["index"] for s in chunk]).cuda()
        pix = torch.stack([s["image"][0, 0].long() + 256 * s["image"][0, 1].long() for s in chunk]).cuda()
        assert torch.equal(idx.long(), pix) and {int(s["coord_convention_id"]) for s in chunk} == {1}
        got += idx.tolist()
    assert got == expected.tolist()
    LS.write_shard(tmp_path, "replicant-face-v4-wider-100k", "pose_landmarks_noshape", 1003, 16, 16, 6)
    rep = P.make_validation_loader("replicantface-train", use_head_roi=False, datadir=str(tmp_path))
    assert [int(s["index"]) for s in rep] == np.random.default_rng(seed=42).integers(0, 1002, size=1000).tolist()
