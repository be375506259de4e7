"""Host side of the flat training step (train.flatten_batches, train.loss_terms), the synthetic loader's per-step Tag split and the
train script's --graph-layout flag - everything of the feature that runs without a GPU.  The GPU side: tests/test_flat_step_gpu.py."""
import numpy as np
import pytest
import torch

from oracle.synth import make_inputs, make_labels
from util import load_golden, make_batches, script_args, train_script

NAN = float("nan")


def _other_split(n_lm=2, n_noshape=3, n_pose=3, seed=77):
    """Three sub-batches built from oracle.synth.make_labels with a split the goldens do not have (CPU tensors)."""
    from trackertraincode.datasets.batch import Batch, Metadata
    from trackertraincode.pipelines import Tag

    B = n_lm + n_noshape + n_pose
    image, ids = make_inputs(B, seed=seed)
    lab = make_labels(B, seed=seed)
    t = lambda a: torch.from_numpy(a.copy())
    out, off = [], 0
    for tag, n, fields in ((Tag.POSE_WITH_LANDMARKS, n_lm, ("pose", "coord", "roi", "pt3d_68", "shapeparam", "dataset_weight")),
                           (Tag.POSE_WITH_LMKS_NO_SHAPE_PARAMS, n_noshape, ("pose", "coord", "roi", "pt3d_68")),
                           (Tag.ONLY_POSE, n_pose, ("pose", "coord", "roi"))):
        rows = slice(off, off + n)
        out.append(Batch(Metadata(129, batchsize=n, tag=tag), dict(image=t(image[rows]), coord_convention_id=t(ids[rows]), **{k: t(lab[k][rows]) for k in fields})))
        off += n
    return out, lab


def test_flatten_batches_rows_codes_and_fill():
    import trackertraincode.train as train

    _, meta = load_golden("model_full.npz")
    batches = make_batches(meta, "cpu")
    split, B = meta["split"], meta["B"]
    flat = train.flatten_batches(batches, fill=NAN)
    assert flat.meta.batchsize == B and flat.meta.prefixshape == (B,)
    assert flat["tag_code"].dtype == torch.int32 and flat["tag_code"].tolist() == [1] * split + [7] * (B - split)
    assert flat["dataset_weight"].dtype == torch.float32 and flat["dataset_weight"].tolist() == [1.0] * B
    for k in ("image", "coord_convention_id", "pose", "coord", "roi"):  # in every sub-batch: rows in sub-batch order
        assert torch.equal(flat[k], torch.concat([b[k] for b in batches])) and flat[k].dtype == batches[0][k].dtype, k
    for k in ("pt3d_68", "shapeparam"):  # only the landmark Tag has them
        assert flat[k].shape == (B,) + tuple(batches[0][k].shape[1:])
        assert torch.equal(flat[k][:split], batches[0][k]) and bool(flat[k][split:].isnan().all()), k
    zero = train.flatten_batches(batches)  # the default fill
    assert not bool(zero["shapeparam"][split:].any()) and torch.equal(zero["shapeparam"][:split], batches[0]["shapeparam"])
    # dataset weights where the sub-batches carry them
    dw = train.flatten_batches(make_batches(meta, "cpu", with_dataset_weight=True))["dataset_weight"]
    np.testing.assert_array_equal(dw.numpy(), make_labels(B, seed=meta["input_seed"])["dataset_weight"])


def test_flatten_batches_other_split_and_mismatch():
    import trackertraincode.train as train

    batches, lab = _other_split()
    flat = train.flatten_batches(batches, fill=-3.0)
    assert flat["tag_code"].tolist() == [1, 1, 11, 11, 11, 7, 7, 7]
    np.testing.assert_array_equal(flat["dataset_weight"].numpy(), np.concatenate([lab["dataset_weight"][:2], np.ones(6, np.float32)]))
    np.testing.assert_array_equal(flat["pose"].numpy(), lab["pose"])
    np.testing.assert_array_equal(flat["pt3d_68"][:5].numpy(), lab["pt3d_68"][:5])
    assert bool((flat["pt3d_68"][5:] == -3.0).all())
    np.testing.assert_array_equal(flat["shapeparam"][:2].numpy(), lab["shapeparam"][:2])
    assert bool((flat["shapeparam"][2:] == -3.0).all())
    batches[2]["roi"] = torch.zeros(3, 5)  # trailing shape disagrees
    with pytest.raises(ValueError, match="roi"):
        train.flatten_batches(batches)
    batches, _ = _other_split()
    batches[1]["coord"] = batches[1]["coord"].double()  # dtype disagrees
    with pytest.raises(ValueError, match="coord"):
        train.flatten_batches(batches)


@pytest.mark.parametrize("cfg", ["full", "default"])
def test_loss_terms_names_sets_and_weights(cfg):
    import trackertraincode.train as train
    from trackertraincode.pipelines import Tag

    d, meta = load_golden(f"model_{cfg}.npz")
    crit, _ = train_script().setup_losses(script_args(meta["flags"]), None)
    terms = train.loss_terms(crit)
    split = meta["split"]
    for epoch in (0, 20, 150):
        names = [k.split("/")[3] for k in d.files if k.startswith(f"train/e{epoch}/loss/") and k.endswith("/values")]
        assert list(dict.fromkeys(t.name for t in terms)) == names
        # the goldens' batch: rows [:split] POSE_WITH_LANDMARKS, rows [split:] ONLY_POSE, values concatenated over the sub-batches that have the term
        for t in [t for t in terms if Tag.ONLY_LANDMARKS_25D not in t.tags]:
            w = d[f"train/e{epoch}/loss/{t.name}/weights"]
            assert Tag.POSE_WITH_LANDMARKS in t.tags
            np.testing.assert_allclose(t.weight(Tag.POSE_WITH_LANDMARKS, epoch), w[0], rtol=1e-6, err_msg=t.name)
            if Tag.ONLY_POSE in t.tags:
                assert len(w) == meta["B"]
                np.testing.assert_allclose(t.weight(Tag.ONLY_POSE, epoch), w[split], rtol=1e-6, err_msg=t.name)
            else:
                assert len(w) == split, t.name
    by_name = {}
    for t in terms:
        by_name.setdefault(t.name, []).append(t)
    if meta["flags"]["with_pointhead"]:
        for n in ("points3d", "shp_l2"):
            assert all(Tag.ONLY_POSE not in t.tags for t in by_name[n]) and any(Tag.POSE_WITH_LANDMARKS in t.tags for t in by_name[n])
        # Points3dLoss in 3D and in 2.5D share the name, not the callable: two terms, the 2.5D one for ONLY_LANDMARKS_25D alone
        assert len(by_name["points3d"]) == 2 and by_name["points3d"][0].f is not by_name["points3d"][1].f
        assert sorted(len(t.tags) for t in by_name["points3d"]) == [1, 4]
        assert [t.tags for t in by_name["points3d"] if len(t.tags) == 1] == [(Tag.ONLY_LANDMARKS_25D,)]
        assert by_name["shp_l2"][0].tag_set == (1 << Tag.POSE_WITH_LANDMARKS.value) | (1 << Tag.POSE_WITH_LANDMARKS_3D_AND_2D.value)
    assert by_name["rot"][0].tag_set & (1 << Tag.ONLY_POSE.value) and not by_name["rot"][0].tag_set & (1 << Tag.ONLY_LANDMARKS.value)


def test_loss_terms_group_weights_multiply_like_evaluate():
    import trackertraincode.train as train

    f, g = (lambda p, b: p["x"]), (lambda p, b: p["x"] * 2)
    ramp = lambda step: 0.1 * step
    inner = train.CriterionGroup([train.Criterion("a", f, 0.5), train.Criterion("b", g, ramp)], "in_", 3.0)
    crit = {"T1": train.CriterionGroup([inner, train.Criterion("c", f, 2.0)], "out_", lambda step: 1.0 + step), "T2": train.CriterionGroup([train.Criterion("c", f, 7.0)])}
    terms = {t.name: t for t in train.loss_terms({4: crit["T1"], 9: crit["T2"]})}
    assert list(terms) == ["out_in_a", "out_in_b", "out_c", "c"]  # same callable, other name: a term of its own
    ev = {v.name: v.weight for v in crit["T1"].evaluate({"x": torch.ones(2)}, None, 3)}
    for n in ("out_in_a", "out_in_b", "out_c"):
        assert terms[n].weight(4, 3) == ev[n] and terms[n].tag_set == 1 << 4
    assert terms["c"].weight(9, 3) == 7.0 and terms["c"].tags == (9,)
    with pytest.raises(ValueError):
        train.loss_terms({40: crit["T2"]})[0].tag_set  # Tag codes are 0..31


def test_synthetic_loader_vary_split():
    from trackertraincode.pipelines import SyntheticPoseLoader, Tag

    mix = [(Tag.POSE_WITH_LANDMARKS, 11), (Tag.POSE_WITH_LMKS_NO_SHAPE_PARAMS, 1), (Tag.ONLY_POSE, 2)]
    kw = dict(device="cpu", seed=3, inputsize=9, steps_per_epoch=8)

    def sizes(loader):
        return [tuple((b.meta.tag, b.meta.batchsize) for b in bs) for bs in loader]

    a, b = sizes(SyntheticPoseLoader(16, mix, vary_split=True, **kw)), sizes(SyntheticPoseLoader(16, mix, vary_split=True, **kw))
    assert a == b, "same seed, same splits"
    assert all(sum(n for _, n in step) == 16 and all(n > 0 for _, n in step) for step in a)
    assert len(set(a)) > 1, "the split must change between steps"
    assert a != sizes(SyntheticPoseLoader(16, mix, vary_split=True, **dict(kw, seed=4)))
    for step in SyntheticPoseLoader(16, mix, vary_split=True, **kw):  # sub-batches stay well-formed
        for sub in step:
            assert all(v.shape[0] == sub.meta.batchsize for v in sub.values())
    # without the argument, and with False: bitwise the batches of today
    for x, y in zip(SyntheticPoseLoader(16, mix, **kw), SyntheticPoseLoader(16, mix, vary_split=False, **kw)):
        assert [s.meta.tag for s in x] == [s.meta.tag for s in y]
        for s, t in zip(x, y):
            assert list(s.keys()) == list(t.keys()) and all(torch.equal(s[k], t[k]) for k in s.keys())
    assert sizes(SyntheticPoseLoader(16, mix, **kw))[0] == ((Tag.POSE_WITH_LANDMARKS, 13), (Tag.POSE_WITH_LMKS_NO_SHAPE_PARAMS, 1), (Tag.ONLY_POSE, 2))


def test_graph_layout_flag():
    S = train_script()
    p = S.make_parser()
    assert p.parse_args([]).graph_layout == "per-tag" and S.graph_mode(p.parse_args([])) is False
    assert S.graph_mode(p.parse_args(["--graph-steps"])) is True
    a = p.parse_args(["--graph-steps", "--graph-layout", "flat"])
    assert a.graph_layout == "flat" and S.graph_mode(a) == "flat"
    assert S.graph_mode(p.parse_args(["--graph-layout", "flat"])) is False  # only with --graph-steps
    with pytest.raises(SystemExit):
        p.parse_args(["--graph-layout", "rows"])


def test_graphed_step_rejects_unknown_layout():
    import trackertraincode.train as train

    opt = train.ClipAdam([torch.nn.Parameter(torch.zeros(1))])
    with pytest.raises(ValueError, match="layout"):
        train.GraphedTrainStep(torch.nn.Linear(1, 1), {}, opt, layout="rows")
    assert train.GraphedTrainStep(torch.nn.Linear(1, 1), {}, opt).layout == "per_tag"
