"""Width-scaled MobileNet backbones (MobileNet(widen_factor=w)) on the MI355X: the mixed chain of tuned and any-channel-count kernels
(MobileNet.kernel_plan) against the CPU oracle with its block table swapped (tests/width_util.py; pinned against the reference's own
fixtures by tests/test_width_host.py) and against the reference's fixtures themselves.  Every test copies the body and the criteria of its
width-1.0 sibling (named in its docstring)."""
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import refmodel as R
from oracle.synth import digest_close, make_inputs, make_state
from util import GOLDEN, build_net, load_golden, make_batches, script_args, train_script
from width_util import FIXTURES, backbone_state, oracle_width

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_TOL = 1.0e-3  # tests/test_model_gpu.py
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_into(net, sd):
    net.load_state_dict({k[len("convnet."):]: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _run_oracle(sd, image, G, dtype):
    st = {}
    for k, v in sd.items():
        t = torch.from_numpy(np.array(v))
        if t.is_floating_point():
            t = t.to(dtype)
        if not R.is_buffer(k):
            t.requires_grad_(True)
        st[k] = t
    feat, _ = R.mobilenet_forward(st, torch.from_numpy(image).to(dtype), True)
    (feat * torch.from_numpy(G).to(dtype)).sum().backward()
    return feat.detach(), st


# Input seeds: for each case the fp32 AND the fp64 oracle were evaluated on the CPU (8 threads) over seeds 7, 8, ...; kept is the first seed
# for which the fp32 oracle's own parameter gradients all lie within 1e-4 (relative l2) of the fp64 ones, i.e. the CPU evaluation carries no
# flipped ReLU / mask decision of its own (tests/test_backbone_gpu.py's docstring: one flip moves the gradients upstream of it by several
# 1e-3, and whether both fp32 evaluations carry the same flip depends on the host).  Worst tensor at the kept seed: 5e-6 .. 6e-5.
# (1.5, 8): none of the seeds 7..59 is free of a flip on the CPU side (the widest net has the most pre-activations); seed 24 has the
# smallest (1.5e-3 on one tensor) - the one-decision envelope of the sibling's criteria covers it.
SEEDS = {(0.25, 3, False): 8, (0.25, 8, False): 7, (0.5, 3, False): 12, (0.5, 8, False): 25, (0.75, 3, False): 13, (0.75, 8, False): 35,
         (1.5, 3, False): 38, (1.5, 8, False): 24, (0.75, 8, True): 8}


@pytest.mark.parametrize("w,B,blur", sorted(SEEDS))
def test_width_backbone_train_fwd_bwd_matches_oracle(w, B, blur, monkeypatch):
    """tests/test_backbone_gpu.py::test_backbone_train_fwd_bwd_matches_oracle, criteria verbatim: 3 * e_cpu + 2e-5, the envelope of one
    mask decision, the running statistics."""
    from trackertraincode.backbones.mobilenet_v1 import MobileNet

    oracle_width(monkeypatch, w)
    sd, _ = backbone_state(w, blur=blur)
    image, _ = make_inputs(B, seed=SEEDS[(w, B, blur)])
    F_ = int(1024 * w)
    G = np.random.default_rng(5).standard_normal((B, F_)).astype(np.float32)
    f64, st64 = _run_oracle(sd, image, G, torch.float64)
    f32, st32 = _run_oracle(sd, image, G, torch.float32)
    net = MobileNet(num_classes=None, widen_factor=w, use_blurpool=blur).cuda()
    _load_into(net, sd)
    net.train()
    feat = net.forward_features(torch.from_numpy(image).cuda())
    (feat * torch.from_numpy(G).cuda()).sum().backward()
    torch.cuda.synchronize()
    print(f"w={w} B={B} blur={blur}: features hip {_rel(feat.detach().cpu(), f64):.2e} cpu32 {_rel(f32, f64):.2e}")
    assert _rel(feat.detach().cpu(), f64) < 3 * _rel(f32, f64) + 2e-5
    assert _rel(feat.detach().cpu(), f32) < 1e-4
    for k, v in net.state_dict().items():
        ref = st32["convnet." + k].detach()
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref) == 1
        elif "running_" in k:
            np.testing.assert_allclose(v.cpu().numpy(), ref.numpy(), rtol=2e-4, atol=1e-6, err_msg=k)
    flip_tol = 5e-2 if B <= 3 else 2e-2  # per tensor, when the factor-3 criterion does not hold
    bad, loose = [], []
    num = den = num32 = 0.0
    for k, p_ in net.named_parameters():
        g64 = st64["convnet." + k].grad
        e_hip, e_cpu = _rel(p_.grad.cpu(), g64), _rel(st32["convnet." + k].grad, g64)
        num += float((p_.grad.double().cpu() - g64).square().sum())
        num32 += float((st32["convnet." + k].grad.double() - g64).square().sum())
        den += float(g64.square().sum())
        if e_hip > 3 * e_cpu + 2e-5:
            loose.append((k, e_hip, e_cpu))
            if e_hip > flip_tol:
                bad.append((k, e_hip, e_cpu))
    e_all, e_all32 = (num / den) ** 0.5, (num32 / den) ** 0.5
    print(f"w={w} B={B} blur={blur}: all gradients hip {e_all:.2e} cpu32 {e_all32:.2e}; outside factor 3: {[(k, f'{a:.1e}', f'{b:.1e}') for k, a, b in loose[:4]]}")
    assert not bad, f"gradients outside the envelope of one mask decision: {bad[:5]}"
    assert e_all < max(3 * e_all32 + 2e-5, 2e-2 if B <= 3 else 1e-2), (e_all, e_all32, loose[:5])


@pytest.mark.parametrize("w", [0.5, 0.75])
def test_width_backbone_eval_and_intermediates(w, monkeypatch):
    """tests/test_backbone_gpu.py::test_backbone_eval_and_intermediates."""
    from trackertraincode.backbones.mobilenet_v1 import MobileNet

    oracle_width(monkeypatch, w)
    sd, _ = backbone_state(w)
    B = 4
    image, _ = make_inputs(B, seed=9)
    st = R.state_from_numpy(sd, requires_grad=False)
    with torch.no_grad():
        R.mobilenet_forward(st, torch.from_numpy(image), True, momentum=1.0)  # calibrate running stats
        sd_cal = {k: v.numpy().copy() for k, v in st.items()}
        feat_ref, inter_ref = R.mobilenet_forward(st, torch.from_numpy(image), False)
    net = MobileNet(num_classes=None, widen_factor=w).cuda()
    _load_into(net, sd_cal)
    net.eval()
    with torch.no_grad():
        feat, inter = net(torch.from_numpy(image).cuda())
    assert _rel(feat.cpu(), feat_ref) < 2e-4
    assert [tuple(t.shape) for t in inter] == [tuple(t.shape) for t in inter_ref]
    assert [t.shape[1] for t in inter] == net.num_intermediate_features
    for a, b in zip(inter, inter_ref):
        assert _rel(a.cpu(), b) < 2e-4


def _val(v):
    return (v.value if hasattr(v, "value") else v).detach().cpu().numpy()


@pytest.mark.parametrize("w", sorted(FIXTURES))
def test_width_train_step_and_eval_match_reference_golden(w):
    """tests/test_model_gpu.py::test_train_step_matches_reference_golden and ::test_eval_forward_matches_reference_golden on the reference's
    NetworkWithPointHead(backbone_args={"widen_factor": w}) fixtures (tools/gen_golden_width.py)."""
    import trackertraincode.train as train

    d, meta = load_golden(FIXTURES[w])
    S = train_script()
    for epoch in (0, 20, 150):
        net = build_net(meta, DEV).train()
        assert net.convnet.num_features == int(1024 * w)
        crit, _ = S.setup_losses(script_args(meta["flags"]), net)
        batches = make_batches(meta, DEV)
        inputs = torch.concat([b["image"] for b in batches], dim=0)
        ids = torch.concat([b["coord_convention_id"] for b in batches], dim=0)
        preds = net(inputs, ids)
        loss_sum, all_lossvals = train.default_compute_loss(preds, batches, epoch, crit)
        by_name = train.concatenated_lossvals_by_name(itertools.chain.from_iterable(all_lossvals))
        names = [k.split("/")[3] for k in d.files if k.startswith(f"train/e{epoch}/loss/") and k.endswith("/values")]
        assert list(by_name.keys()) == names
        for n in names:
            np.testing.assert_allclose(_val(by_name[n][0]), d[f"train/e{epoch}/loss/{n}/values"], rtol=LOSS_TOL, atol=LOSS_TOL, err_msg=n)
            np.testing.assert_allclose(_val(by_name[n][1]), d[f"train/e{epoch}/loss/{n}/weights"], rtol=1e-6, err_msg=n)
        assert abs(loss_sum.item() - float(d[f"train/e{epoch}/loss_sum"])) < LOSS_TOL
    for k in [k for k in d.files if k.startswith("train/out/")]:
        np.testing.assert_allclose(_val(preds[k[len("train/out/"):]]), d[k], rtol=1e-3, atol=1e-4, err_msg=k)
    loss_sum.backward()
    torch.cuda.synchronize()
    params = dict(net.named_parameters())
    bad = []
    for k in [k for k in d.files if k.startswith("train/grad/")]:
        g = params[k[len("train/grad/"):]].grad
        g = torch.zeros_like(params[k[len("train/grad/"):]]) if g is None else g
        ok, msg = digest_close(d[k], g.cpu().numpy(), rtol=2e-2, atol=1e-6, rtol_samples=1e-1)
        if not ok:
            bad.append((k, msg))
    assert not bad, bad[:5]
    sd = net.state_dict()
    for k in [k for k in d.files if k.startswith("train/after/")]:
        ok, msg = digest_close(d[k], sd[k[len("train/after/"):]].cpu().numpy(), rtol=2e-4, atol=1e-6)
        assert ok, f"{k}: {msg}"
    # eval forward on the calibrated running statistics, with and without dataset ids
    cal = {k[len("calib/"):]: d[k] for k in d.files if k.startswith("calib/")}
    net = build_net(meta, DEV, cal).eval()
    image, ids = make_inputs(meta["B"], seed=meta["input_seed"])
    with torch.no_grad():
        out = net(torch.from_numpy(image).to(DEV), torch.from_numpy(ids).to(DEV))
        out_noid = net(torch.from_numpy(image).to(DEV))
    for prefix, o in (("eval/", out), ("eval_noid/", out_noid)):
        keys = [k[len(prefix):] for k in d.files if k.startswith(prefix)]
        assert set(keys) == set(o.keys())
        for k in keys:
            np.testing.assert_allclose(_val(o[k]), d[prefix + k], rtol=1e-3, atol=1e-4, err_msg=prefix + k)


@pytest.mark.parametrize("w", sorted(FIXTURES))
def test_width_step_at_benchmark_size_matches_oracle(w, monkeypatch):
    """tests/test_fullsize_gpu.py::test_step_at_benchmark_size_matches_oracle at B = 512 (its structure, its oracle helper, its criteria):
    losses within 1e-3, features within 1e-4, every parameter gradient within 3 x the fp32 CPU path's error + 1e-5 of the fp64 oracle."""
    import trackertraincode.train as train
    from test_fullsize_gpu import _oracle
    from test_fullsize_gpu import _rel as rel

    oracle_width(monkeypatch, w)
    B, epoch = 512, 0
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    _, meta = load_golden(FIXTURES[w])
    meta = dict(meta, B=B, split=(B * 5) // 8)
    shapes = {k: tuple(v) for k, v in meta["shapes"].items()}
    image, ids = make_inputs(B, seed=meta["input_seed"])
    S = train_script()

    net = build_net(meta, DEV).train()
    crit, _ = S.setup_losses(script_args(meta["flags"]), net)
    feats = []
    orig = net.convnet.forward_features
    net.convnet.forward_features = lambda x: feats.append(orig(x)) or feats[-1]
    batches = make_batches(meta, DEV)
    inputs = torch.concat([b["image"] for b in batches], dim=0)
    ids_d = torch.concat([b["coord_convention_id"] for b in batches], dim=0)
    preds = net(inputs, ids_d)
    loss_sum, all_lossvals = train.default_compute_loss(preds, batches, epoch, crit)
    by_name = train.concatenated_lossvals_by_name(itertools.chain.from_iterable(all_lossvals))
    loss_sum.backward()
    torch.cuda.synchronize()
    hip_grads = {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in net.named_parameters()}
    hip_feat = feats[0].detach().cpu()
    hip_loss = loss_sum.item()
    hip_vals = {k: v[0].detach().cpu() for k, v in by_name.items()}
    hip_state = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    del net, preds, loss_sum, by_name, all_lossvals, feats
    torch.cuda.empty_cache()

    o32 = _oracle(meta, shapes, image, ids, epoch, torch.float32, want_grads=True)
    assert abs(hip_loss - o32["loss"]) < 1e-3, (hip_loss, o32["loss"])
    assert list(hip_vals.keys()) == list(o32["by_name"].keys())
    for n, v in o32["by_name"].items():
        np.testing.assert_allclose(hip_vals[n].numpy(), v.numpy(), rtol=1e-3, atol=1e-3, err_msg=n)
    e_feat = rel(hip_feat, o32["feat"])
    assert e_feat < 1e-4, e_feat
    for k, v in o32["running"].items():
        np.testing.assert_allclose(hip_state[k].numpy(), v.numpy(), rtol=2e-4, atol=2e-6, err_msg=k)
    o64 = _oracle(meta, shapes, image, ids, epoch, torch.float64, want_grads=True)
    assert abs(hip_loss - o64["loss"]) < 1e-3
    bad, worst = [], (0.0, "")
    for k, g in hip_grads.items():
        g64 = o64["grads"][k]
        if g64 is None:
            assert g is None or float(g.abs().max()) == 0.0, k
            continue
        e_hip, e_cpu = rel(g, g64), rel(o32["grads"][k], g64)
        if e_hip > worst[0]:
            worst = (e_hip, k)
        if e_hip > 3 * e_cpu + 1e-5:
            bad.append((k, f"hip {e_hip:.2e}", f"cpu32 {e_cpu:.2e}"))
    print(f"w={w} B={B} epoch={epoch}: loss {hip_loss:.6f} (oracle {o32['loss']:.6f}), features rel {e_feat:.1e}, worst gradient rel {worst[0]:.1e} ({worst[1]})")
    assert not bad, bad[:8]


def test_width_graphed_train_step_matches_eager(monkeypatch):
    """tests/test_model_gpu.py::test_graphed_train_step_matches_eager at w = 0.5 (a chain that mixes both kernel families): the captured
    step walks the eager step's trajectory; the new launch path makes no synchronisation and no host read (a capture would fail)."""
    import trackertraincode.backbones.mobilenet_v1 as MB
    import trackertraincode.train as train

    monkeypatch.setattr(MB, "_DETERMINISTIC", True)  # (the TUNED layers' weight gradients in their fixed-order form, as in the sibling)
    d, meta = load_golden(FIXTURES[0.5])
    S = train_script()

    def make():
        net = build_net(meta, DEV).train()
        crit, _ = S.setup_losses(script_args(meta["flags"]), net)
        opt, sch = S.create_optimizer(net, script_args(meta["flags"], epochs=20))
        return net, crit, opt, sch

    batches = make_batches(meta, DEV)
    other = make_batches(meta, DEV)
    for b in other:
        b["image"] = b["image"].flip(-1).contiguous()
    seq = [batches, other, batches, other, other, batches]
    epochs = [0, 0, 0, 1, 1, 1]

    net_e, crit_e, opt_e, sch_e = make()
    losses_e = []
    for i, (bs, ep) in enumerate(zip(seq, epochs)):
        if i == 3:
            sch_e.step()
        opt_e.zero_grad(set_to_none=True)
        out = train.training_step(net_e, bs, ep, crit_e)
        out["loss"].backward()
        opt_e.step()
        losses_e.append(out["loss"].item())

    net_g, crit_g, opt_g, sch_g = make()
    g = train.GraphedTrainStep(net_g, crit_g, opt_g)
    losses_g = []
    for i, (bs, ep) in enumerate(zip(seq, epochs)):
        if i == 3:
            sch_g.step()
        losses_g.append(g.run(bs, ep)["loss"].item())
    torch.cuda.synchronize()
    assert g.captures == 1, "a learning-rate change must not force a re-capture"
    assert opt_g._t == opt_e._t == len(seq)
    np.testing.assert_allclose(losses_g[:2], losses_e[:2], rtol=1e-4)
    np.testing.assert_allclose(losses_g[2:4], losses_e[2:4], rtol=2e-3)
    np.testing.assert_allclose(losses_g[4:], losses_e[4:], rtol=6e-2)
    lr = max(gr["lr"] for gr in opt_e.param_groups)
    for (k, a), (_, b) in zip(net_g.state_dict().items(), net_e.state_dict().items()):
        if a.is_floating_point():
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=2.5 * lr * len(seq), err_msg=k)
        else:
            assert int(a) == int(b), k


@pytest.mark.parametrize("B,blur", [(3, False), (8, False), (8, True)])
def test_width_frozen_batchnorm_backward(B, blur, monkeypatch):
    """tests/test_finetune_gpu.py::test_mobilenet_frozen_batchnorm_backward at w = 0.75 (its helpers, its criteria: 3 * e_cpu + 3e-5)."""
    from test_finetune_gpu import _check, _state
    from trackertraincode.backbones.mobilenet_v1 import MobileNet

    w = 0.75
    oracle_width(monkeypatch, w)
    _, shapes = backbone_state(w, blur=blur)
    net = MobileNet(num_classes=None, widen_factor=w, use_blurpool=blur).cuda()
    assert _check(net, _state(shapes, 2), R.mobilenet_forward, int(1024 * w), B, "convnet.") == 27


def test_width_two_steps_are_bitwise_equal():
    """Two identical steps at w = 0.75 (every layer on the any-channel-count family) give bitwise equal features and parameter gradients
    WITHOUT TTK_DETERMINISTIC: the family has no float atomics."""
    import trackertraincode.backbones.mobilenet_v1 as MB

    assert not MB._DETERMINISTIC, "run without TTK_DETERMINISTIC: the point is the default mode"
    w, B = 0.75, 24
    for blur in (False, True):
        torch.manual_seed(0)
        net = MB.MobileNet(num_classes=None, widen_factor=w, use_blurpool=blur).cuda().train()
        assert all(f == "anyc" for _, f in net.kernel_plan())
        x = torch.randn(B, 1, 129, 129, device=DEV)
        G = torch.randn(B, net.num_features, device=DEV)
        start = {k: v.clone() for k, v in net.state_dict().items()}
        runs = []
        for _ in range(2):
            net.load_state_dict(start)  # the running means are the pivot of the BatchNorm sums: part of the input
            net.zero_grad(set_to_none=True)
            feat = net.forward_features(x)
            (feat * G).sum().backward()
            torch.cuda.synchronize()
            runs.append([feat.detach().clone()] + [p_.grad.clone() for p_ in net.parameters()])
        assert all(torch.equal(a, b) for a, b in zip(*runs)), blur
        assert all(torch.isfinite(t).all() and float(t.abs().max()) > 0 for t in runs[0])


def test_width_train_script_end_to_end(tmp_path):
    """tests/test_train_script_gpu.py::test_script_main with --widen-factor 0.5 on the synthetic loader, two epochs: the loss is finite
    and decreases in the mean, the checkpoint carries the width and loads, and scripts/evaluate_pose_network.py runs on it over the
    bundled aflw2kmini.npz."""
    import importlib.util
    import json

    from test_train_script_gpu import WRAP
    from trackertraincode.neuralnets.models import load_model

    script = os.path.join(REPO, "neuralnet-tracker-traincode_amd", "scripts", "train_poseestimator.py")
    wrap = tmp_path / "wrap.py"
    # (the wrapper of the sibling test, plus a line per step with the loss)
    wrap.write_text(WRAP.replace('runpy.run_path(', '''import trackertraincode.train as T
_step = T.training_step
def logged(*a, **k):
    out = _step(*a, **k)
    print("STEPLOSS", float(out["loss"]), flush=True)
    return out
T.training_step = logged
runpy.run_path('''))
    data = tmp_path / "data"
    data.mkdir()
    shutil.copy(os.path.join(GOLDEN, "aflw2kmini.npz"), data / "aflw2k.npz")
    env = dict(os.environ, DATADIR=str(data), PYTHONPATH=os.path.join(REPO, "neuralnet-tracker-traincode_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    flags = ["--ds", "synthetic", "--batchsize", "32", "--epochs", "2", "--widen-factor", "0.5"]
    out = subprocess.run([sys.executable, str(wrap), script, *flags, "--outdir", str(tmp_path / "out")], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    losses = [float(l.split()[1]) for l in out.stdout.splitlines() if l.startswith("STEPLOSS")]
    assert len(losses) >= 4 and all(np.isfinite(losses)), losses
    half = len(losses) // 2
    assert np.mean(losses[half:]) < np.mean(losses[:half]), losses
    ck = str(tmp_path / "out" / "NetworkWithPointHead_mobilenetv1" / "last.ckpt")
    net = load_model(ck)
    assert all(torch.isfinite(v).all() for v in net.state_dict().values() if v.is_floating_point())
    assert net.get_config()["backbone_args"] == {"use_blurpool": False, "widen_factor": 0.5} and net.convnet.num_features == 512
    spec = importlib.util.spec_from_file_location("amd_eval_script", os.path.join(REPO, "neuralnet-tracker-traincode_amd", "scripts", "evaluate_pose_network.py"))
    E = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(E)
    shutil.copy(os.path.join(GOLDEN, "aflw2kmini.npz"), tmp_path / "aflw2k.npz")
    out_json = str(tmp_path / "t.json")
    E.main([ck, "--ds", "aflw2k3d", "--datadir", str(tmp_path), "--json", out_json, "--allow-landmark-roi-fallback"])
    (model, cols), = json.load(open(out_json)).items()
    assert len(cols["Data"]) >= 1 and all(np.isfinite(v).all() for k, v in cols.items() if k != "Data" and isinstance(v, list) and v and isinstance(v[0], float))
