"""A training step whose sub-batches include a Tag WITHOUT pose / coord / roi (ONLY_LANDMARKS_25D: Face Synthetics rows; from the synthetic
loader such rows carry just image, coord_convention_id and pt3d_68) in all three forms of the step: per-Tag eager, GraphedTrainStep per-Tag,
and flat (flat_training_step, GraphedTrainStep(layout="flat")).  B = 8: 3 POSE_WITH_LANDMARKS + 2 ONLY_POSE + 3 ONLY_LANDMARKS_25D rows of
oracle.synth's inputs.

Tolerances.  tests/test_loss_bookkeeping_gpu.py holds its two-Tag batch to: loss and per-sample values BITWISE between two ways of launching
the same kernels, gradients to rtol 1e-6 / atol 1e-9; and values against a plain float64 formula to rtol 1e-6 / atol 1e-7, a weighted sum to
1e-6 |ref| + 1e-7.  The first pair is applied here to batched against unbatched launches, the second to the step's losses against
oracle.refmodel evaluated in float64 ON THE STEP'S OWN PREDICTIONS (so that the backbone's fp32 rounding, which the bookkeeping file never
sees either, stays out of the comparison).  Flat against per-Tag: bitwise - forward outputs, loss and every parameter gradient (without
dataset weights every product w * val is the same single rounding in both forms, and the double-precision sums differ in order only)."""
import itertools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import landmark_shards as LS
from oracle import refmodel as R
from oracle.synth import make_inputs, make_labels
from util import GOLDEN, REPO, build_net, load_golden, script_args, train_script

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
RAMP_EPOCH = 30  # --with-nll-loss --rampup-nll-losses over 200 epochs ramps from epoch 20 to 40
CASES = {"default": ("model_default.npz", 150), "nll_ramp": ("model_full.npz", RAMP_EPOCH)}
FIELDS = {"POSE_WITH_LANDMARKS": ("pose", "coord", "roi", "pt3d_68", "shapeparam"), "ONLY_POSE": ("pose", "coord", "roi"), "ONLY_LANDMARKS_25D": ("pt3d_68",)}


def _layout(n25=3):
    """[(Tag name, row slice)]: 3 landmark + pose rows, then pose-only rows, then n25 landmark-only rows (left out when there are none)."""
    out = [("POSE_WITH_LANDMARKS", slice(0, 3)), ("ONLY_POSE", slice(3, 8 - n25))]
    return out + ([("ONLY_LANDMARKS_25D", slice(8 - n25, 8))] if n25 else [])


def _batches(meta, n25=3, flip=False):
    from trackertraincode.datasets.batch import Batch, Metadata
    from trackertraincode.pipelines import Tag

    image, ids = make_inputs(8, seed=meta["input_seed"])
    if flip:
        image = image[..., ::-1]
    lab = make_labels(8, seed=meta["input_seed"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return [Batch(Metadata(129, batchsize=len(range(8)[rows]), tag=Tag[name]),
                  dict(image=t(image[rows]), coord_convention_id=t(ids[rows]), **{f: t(lab[f][rows]) for f in FIELDS[name]})) for name, rows in _layout(n25)]


def _oracle_batches(meta, n25=3):
    lab = make_labels(8, seed=meta["input_seed"])
    return [dict({f: torch.from_numpy(lab[f][rows].copy()).double() for f in FIELDS[name]}, tag=name, n=len(range(8)[rows])) for name, rows in _layout(n25)]


def _net_and_criterions(meta):
    S = train_script()
    net = build_net(meta, DEV).train()
    crit, _ = S.setup_losses(script_args(meta["flags"]), net)
    return net, crit


def _val(v):
    return (v.value if hasattr(v, "value") else v).detach()


@pytest.mark.parametrize("case", sorted(CASES))
def test_per_tag_eager_step_against_the_oracle(case, monkeypatch):
    import trackertraincode.train as train
    from trackertraincode.neuralnets import _hipops

    golden, epoch = CASES[case]
    _, meta = load_golden(golden)
    net, crit = _net_and_criterions(meta)
    batches = _batches(meta)
    seen = {}
    net.register_forward_hook(lambda m, a, o: seen.update(o))
    out = train.training_step(net, batches, epoch, crit)
    out["loss"].backward()
    torch.cuda.synchronize()
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    # the oracle's loss on these predictions, float64; its 2-D points loss is loss_points3d(p, s, 2)
    fl = meta["flags"]
    ocrit, _ = R.setup_losses(with_pointhead=fl["with_pointhead"], with_nll_loss=fl["with_nll_loss"], rampup_nll_losses=fl["rampup_nll_losses"], epochs=200,
                              gmm=R.ShapeGmm(os.path.join(GOLDEN, "shapeparams_gmm.npz")))
    p64 = {k: _val(v).double().cpu() for k, v in seen.items()}
    ref_loss, by_name = R.compute_loss(p64, _oracle_batches(meta), epoch, ocrit)
    assert list(out["mt_losses"]) == list(by_name)
    n_rows = {"rot": 5, "xy": 5, "sz": 5, "box": 5, "points3d": 6, "shp_l2": 3, "quatregularization1": 8, "nll_shp_gmm": 8, "nllrot": 5, "nllcoord": 5,
              "nllbox": 5, "nllpoints3d": 6}
    for name, (v, _) in by_name.items():
        got = out["mt_losses"][name].cpu().numpy()
        assert got.shape == (n_rows[name],) == tuple(v.shape), name
        err = np.abs(got - v.numpy())
        print(f"{case} {name}: max |hip - oracle64| {err.max():.3e} (values up to {np.abs(v.numpy()).max():.3e})")
    print(f"{case} loss_sum hip {out['loss'].item():.9g} oracle64 {ref_loss.item():.9g} |diff| {abs(out['loss'].item() - ref_loss.item()):.3e}")
    for name, (v, _) in by_name.items():
        np.testing.assert_allclose(out["mt_losses"][name].cpu().numpy(), v.numpy(), rtol=1e-6, atol=1e-7, err_msg=name)
    assert abs(out["loss"].item() - ref_loss.item()) <= 1e-6 * abs(ref_loss.item()) + 1e-7
    # batched against unbatched launches on the same predictions: the two-Tag statement of test_loss_bookkeeping_gpu.py for three Tags
    def run(batching):
        monkeypatch.setattr(_hipops, "_BATCHING", batching)
        preds = {k: (type(v)(v.value.detach().clone().requires_grad_(True)) if hasattr(v, "value") else v.detach().clone().requires_grad_(True)) for k, v in seen.items()}
        leaves = {k: (v.value if hasattr(v, "value") else v) for k, v in preds.items()}
        loss, vals = train.default_compute_loss(preds, batches, epoch, crit)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach(), train.concatenated_values_by_name(itertools.chain.from_iterable(vals)), {k: t.grad for k, t in leaves.items()}

    la, va, ga = run(True)
    lb, vb, gb = run(False)
    assert torch.equal(la, lb) and va.keys() == vb.keys() and all(torch.equal(va[k], vb[k]) for k in va)
    for k in ga:
        assert (ga[k] is None) == (gb[k] is None), k
        if ga[k] is not None:
            torch.testing.assert_close(ga[k], gb[k], rtol=1e-6, atol=1e-9, msg=k)
    for k in ("coord", "roi"):  # nothing reaches the pose / box predictions of the landmark-only rows
        assert ga[k] is not None and not bool(ga[k][5:].any()) and bool(ga[k][:5].any()), k


def _run_step(meta, epoch, flat, fill=NAN):
    import trackertraincode.train as train

    net, crit = _net_and_criterions(meta)
    seen, kept = {}, {}

    def hook(m, a, o):
        seen.update(o)
        for k in ("coord", "roi"):
            t = o[k].value if hasattr(o[k], "value") else o[k]
            t.retain_grad()
            kept[k] = t

    net.register_forward_hook(hook)
    batches = _batches(meta)
    if flat:
        out = train.flat_training_step(net, train.flatten_batches(batches, fill=fill), epoch, crit)
    else:
        out = train.training_step(net, batches, epoch, crit)
    out["loss"].backward()
    torch.cuda.synchronize()
    return ({n: _val(v) for n, v in seen.items()}, out["loss"].detach().clone(), {n: p.grad for n, p in net.named_parameters()},
            {k: t.grad for k, t in kept.items()}, out)


@pytest.mark.parametrize("case", sorted(CASES))
def test_flat_step_equals_per_tag_step_and_never_reads_dead_rows(case, monkeypatch):
    import trackertraincode.backbones.mobilenet_v1 as MB

    monkeypatch.setattr(MB, "_DETERMINISTIC", True)
    golden, epoch = CASES[case]
    _, meta = load_golden(golden)
    p_e, loss_e, g_e, _, _ = _run_step(meta, epoch, flat=False)
    p_f, loss_f, g_f, pg_f, out_f = _run_step(meta, epoch, flat=True, fill=NAN)
    p_z, loss_z, g_z, pg_z, _ = _run_step(meta, epoch, flat=True, fill=0.0)
    # dead rows: NaN in every label row a sub-batch does not have changes nothing, bit for bit
    assert bool(torch.isfinite(loss_f)) and torch.equal(loss_f, loss_z)
    for n in g_z:
        assert (g_f[n] is None) == (g_z[n] is None), n
        if g_f[n] is not None:
            assert bool(torch.isfinite(g_f[n]).all()) and torch.equal(g_f[n], g_z[n]), n
    for k in ("coord", "roi"):  # the gradients ARRIVING at the pose / box predictions are exactly 0 in the landmark-only rows
        assert pg_f[k] is not None and pg_f[k].shape[0] == 8
        assert not bool(pg_f[k][5:].any()) and bool(pg_f[k][:5].any()) and torch.equal(pg_f[k], pg_z[k]), k
    rows = out_f["mt_rows"]
    assert rows["rot"].tolist() == [True] * 5 + [False] * 3 and rows["points3d"].tolist() == [True] * 3 + [False] * 2 + [True] * 3
    assert rows["shp_l2"].tolist() == [True] * 3 + [False] * 5 and rows["quatregularization1"].tolist() == [True] * 8
    assert all(bool(torch.isfinite(v).all()) and not bool(v[~rows[n]].any()) for n, v in out_f["mt_losses"].items())
    # flat against per-Tag: the same bits in the forward outputs, the loss and every parameter gradient
    assert list(p_f) == list(p_e)
    for n in p_e:
        assert torch.equal(p_f[n], p_e[n]), f"forward output {n}"
    print(f"{case} loss flat {loss_f.item():.9g} per-Tag {loss_e.item():.9g}")
    differing = [(n, float((g_f[n].double() - g_e[n].double()).abs().max()), float(g_e[n].abs().max())) for n in g_e
                 if g_e[n] is not None and g_f[n] is not None and not torch.equal(g_f[n], g_e[n])]
    print(f"{case} parameter gradients that differ between flat and per-Tag: {len(differing)} of {len(g_e)}; worst {sorted(differing, key=lambda d: -d[1])[:3]}")
    assert torch.equal(loss_f, loss_e)
    for n in g_e:
        assert (g_f[n] is None) == (g_e[n] is None), n
    assert not differing


SEQ_N25 = [3, 1, 0]


def _make_run(meta, precision=None):
    S = train_script()
    net = build_net(meta, DEV).train()
    if precision:
        net.convnet.set_precision(precision)
    crit, _ = S.setup_losses(script_args(meta["flags"]), net)
    opt, _ = S.create_optimizer(net, script_args(meta["flags"], epochs=20))
    return net, crit, opt


def _eager_losses(meta, seq, epoch, precision=None):
    import trackertraincode.train as train

    net, crit, opt = _make_run(meta, precision)
    losses = []
    for i, n25 in enumerate(seq):
        opt.zero_grad(set_to_none=True)
        out = train.training_step(net, _batches(meta, n25, flip=i % 2 == 1), epoch, crit)
        out["loss"].backward()
        opt.step()
        losses.append(out["loss"].item())
    return losses


@pytest.mark.parametrize("precision", [None, "bf16-compute"], ids=["fp32", "bf16_compute"])
def test_flat_graph_replays_steps_whose_landmark_only_count_changes(precision, monkeypatch):
    """3, 1, 0 landmark-only rows: ONE capture (the first step shows every field), no fallback, no warning, and the losses of the eager per-Tag
    run (fp32: the tolerances of test_flat_step_gpu.test_one_graph_serves_a_varying_split for its first three steps; bf16-compute: its loosest
    tier for the two replayed steps - parameters that differ in the last bits after one Adam step move bf16 roundings in the backbone)."""
    import trackertraincode.backbones.mobilenet_v1 as MB
    import trackertraincode.train as train

    monkeypatch.setattr(MB, "_DETERMINISTIC", True)
    _, meta = load_golden("model_full.npz")
    ref = _eager_losses(meta, SEQ_N25, RAMP_EPOCH, precision)
    net, crit, opt = _make_run(meta, precision)
    g = train.GraphedTrainStep(net, crit, opt, layout="flat")
    got = []
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        for i, n25 in enumerate(SEQ_N25):
            out = g.run(_batches(meta, n25, flip=i % 2 == 1), RAMP_EPOCH)
            got.append(out["loss"].item())
            assert out["mt_rows"]["rot"].tolist() == [True] * (8 - n25) + [False] * n25
            assert out["mt_rows"]["points3d"].tolist() == [True] * 3 + [False] * (5 - n25) + [True] * n25
            assert bool(torch.isfinite(out["mt_losses"]["points3d"]).all()) and not bool(out["mt_losses"]["rot"][8 - n25:].any())
    torch.cuda.synchronize()
    print(f"flat graph {precision or 'fp32'} losses {got} eager {ref}")
    assert g.captures == 1 and g.eager_only is False and opt._t == 3
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
    if precision is None:
        np.testing.assert_allclose(got[:2], ref[:2], rtol=1e-4)
        np.testing.assert_allclose(got[2:], ref[2:], rtol=2e-3)
    else:
        np.testing.assert_allclose(got[:1], ref[:1], rtol=1e-4)  # (the first step runs eagerly in both)
        np.testing.assert_allclose(got[1:], ref[1:], rtol=6e-2)


def test_per_tag_graph_replays_a_landmark_only_layout_and_still_falls_back(monkeypatch):
    import trackertraincode.backbones.mobilenet_v1 as MB
    import trackertraincode.train as train

    monkeypatch.setattr(MB, "_DETERMINISTIC", True)
    _, meta = load_golden("model_full.npz")
    # the same layout twice: one capture, the second step is a replay of a graph whose third sub-batch has neither pose nor coord nor roi
    ref = _eager_losses(meta, [3, 3], RAMP_EPOCH)
    net, crit, opt = _make_run(meta)
    g = train.GraphedTrainStep(net, crit, opt)
    got = [g.run(_batches(meta, 3, flip=i % 2 == 1), RAMP_EPOCH)["loss"].item() for i in range(2)]
    torch.cuda.synchronize()
    assert g.layout == "per_tag" and g.captures == 1 and not g.eager_only and opt._t == 2
    np.testing.assert_allclose(got, ref, rtol=1e-4)
    # a count that changes every step: three misses, the warning, eager from there on - as for every other varying split
    ref = _eager_losses(meta, SEQ_N25, RAMP_EPOCH)
    net, crit, opt = _make_run(meta)
    g = train.GraphedTrainStep(net, crit, opt)
    got = []
    with pytest.warns(RuntimeWarning, match="sub-batch layout changed"):
        for i, n25 in enumerate(SEQ_N25):
            out = g.run(_batches(meta, n25, flip=i % 2 == 1), RAMP_EPOCH)
            got.append(out["loss"].item())
            assert "mt_rows" not in out
    assert g.eager_only is True and g.captures == 2 and opt._t == 3
    np.testing.assert_allclose(got[:2], ref[:2], rtol=1e-4)
    np.testing.assert_allclose(got[2:], ref[2:], rtol=2e-3)


WRAP = r"""
import sys, os, runpy
sys.argv = [sys.argv[1]] + sys.argv[2:]
import trackertraincode.pipelines as P
_orig = P.make_pose_estimation_loaders
def short(*a, **k):
    P._TEST_SHARD = ("aflw2k", P.Tag.POSE_WITH_LANDMARKS, (0, 8))  # the generated stand-in has 16 frames
    k["steps_per_epoch"] = 4
    tr, te, n = _orig(*a, **k)
    sets = sorted((d.tag.name, len(d)) for d in tr.datasets)
    print("TRAIN SETS", sets, flush=True)
    return tr, te, n
P.make_pose_estimation_loaders = short
runpy.run_path(sys.argv[0], run_name="__main__")
"""


def test_train_script_over_a_landmark_only_mix(tmp_path):
    """scripts/train_poseestimator.py --ds repro_300_wlp+synface:8 as a program over generated shards (the epoch cut to four steps)."""
    from trackertraincode.neuralnets.models import load_model

    script = os.path.join(REPO, "neuralnet-tracker-traincode_amd", "scripts", "train_poseestimator.py")
    wrap = tmp_path / "wrap.py"
    wrap.write_text(WRAP)
    data = tmp_path / "data"
    data.mkdir()
    LS.write_training_mix(data)
    env = dict(os.environ, DATADIR=str(data), PYTHONPATH=os.path.join(REPO, "neuralnet-tracker-traincode_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    flags = ["--ds", "repro_300_wlp+synface:8", "--epochs", "1", "--batchsize", "16"]
    out = subprocess.run([sys.executable, str(wrap), script, *flags, "--outdir", str(tmp_path / "out")], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "TRAIN SETS [('ONLY_LANDMARKS_25D', 40), ('POSE_WITH_LANDMARKS', 50)]" in out.stdout, out.stdout[-2000:]
    net = load_model(str(tmp_path / "out" / "NetworkWithPointHead_mobilenetv1" / "last.ckpt"))
    assert all(torch.isfinite(v).all() for v in net.state_dict().values() if v.is_floating_point())
