"""Width-scaled MobileNet backbones (MobileNet(widen_factor=w), reference backbones/mobilenet_v1.py:113-146), host side; CPU only:
construction and the checkpoint surface against the reference's recorded shapes, the per-layer kernel plan, the checkpoint round trip, the
CPU oracle with its block table swapped against the reference fixtures (what licenses that oracle for the GPU tests of
tests/test_width_gpu.py), the train script's flag, the precision refusal and the layout helpers."""
import pytest
import torch

import numpy as np

from oracle import refmodel as R
from oracle.synth import make_inputs, make_state
from util import GOLDEN, load_golden, script_args, train_script
from width_util import FIXTURES, WIDTHS, oracle_width, scaled_blocks, scaled_channels


@pytest.mark.parametrize("w", WIDTHS + [2.0])
def test_constructs_with_the_references_shapes(w):
    from trackertraincode.backbones.mobilenet_v1 import MobileNet

    net = MobileNet(num_classes=None, widen_factor=w)
    c0, blocks = scaled_channels(w), scaled_blocks(w)
    assert net.num_features == int(1024 * w)
    assert net.num_intermediate_features == [int(64 * w), int(128 * w), int(256 * w), int(512 * w), int(1024 * w)]
    mine = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    if w in FIXTURES:  # the reference's own state_dict, recorded by tools/gen_golden_width.py
        _, meta = load_golden(FIXTURES[w])
        ref = {k[len("convnet."):]: tuple(v) for k, v in meta["shapes"].items() if k.startswith("convnet.")}
        assert list(mine.keys()) == list(ref.keys())
        assert mine == ref
    assert mine["conv1.weight"] == (c0, 1, 5, 5) and mine["bn1.running_var"] == (c0,)
    for name, cin, cout, _ in blocks:
        assert mine[f"{name}.conv_dw.weight"] == (cin, 1, 3, 3) and mine[f"{name}.bn_dw.weight"] == (cin,)
        assert mine[f"{name}.conv_sep.weight"] == (cout, cin, 1, 1) and mine[f"{name}.bn_sep.bias"] == (cout,)
    assert MobileNet(num_classes=10, widen_factor=w).fc.weight.shape == (10, int(1024 * w))


def test_widths_outside_the_domain_raise():
    from trackertraincode.backbones.mobilenet_v1 import MobileNet

    with pytest.raises(ValueError, match=r"= 9\b"):  # int(32 * 0.3) = 9: the offending channel count is named
        MobileNet(num_classes=None, widen_factor=0.3)
    with pytest.raises(ValueError, match="4096"):
        MobileNet(num_classes=None, widen_factor=4.0)
    with pytest.raises(NotImplementedError):
        MobileNet(num_classes=None, widen_factor=0.5, input_channel=3)
    with pytest.raises(NotImplementedError):
        MobileNet(num_classes=None, widen_factor=0.5, return_only_featuremap=True)


def test_kernel_plan():
    from trackertraincode.backbones.mobilenet_v1 import MobileNet

    plan = lambda w: MobileNet(num_classes=None, widen_factor=w).kernel_plan()
    p1 = plan(1.0)
    assert len(p1) == 1 + 2 * 13 + 1 and all(f == "tuned" for _, f in p1)
    assert [n for n, f in plan(0.5) if f == "anyc"] == ["conv1", "dw2_1.conv_dw", "dw2_1.conv_sep"]
    assert all(f == "tuned" for n, f in plan(0.5) if n not in ("conv1", "dw2_1.conv_dw", "dw2_1.conv_sep"))
    for w in (0.75, 1.5):
        assert all(f == "anyc" for _, f in plan(w)), w
    assert [n for n, _ in plan(0.75)] == [n for n, _ in p1]


@pytest.mark.parametrize("w", [0.5, 0.75])
def test_checkpoint_round_trip(w, tmp_path):
    from trackertraincode.neuralnets.models import NetworkWithPointHead, load_model, save_model

    torch.manual_seed(3)
    net = NetworkWithPointHead(enable_point_head=True, enable_uncertainty=True, config="mobilenetv1",
                               backbone_args={"widen_factor": w, "use_blurpool": False}).eval()
    for m in net.modules():  # running statistics that are not the identity
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    path = str(tmp_path / "w.ckpt")
    save_model(net, path)
    back = load_model(path).eval()
    assert back.get_config()["backbone_args"]["widen_factor"] == w and back.convnet.num_features == int(1024 * w)
    assert back.convnet.kernel_plan() == net.convnet.kernel_plan()
    x = torch.from_numpy(make_inputs(2, seed=5)[0])
    with torch.no_grad():
        a, b = net(x), back(x)
    assert set(a) == set(b)
    for k in a:
        va, vb = (getattr(v, "value", v) for v in (a[k], b[k]))
        assert torch.equal(va, vb), k


@pytest.mark.parametrize("w", sorted(FIXTURES))
def test_oracle_with_swapped_table_matches_reference_fixture(w, monkeypatch, golden_dir):
    """The assertions of tests/test_oracle_golden.py (test_eval_forward, test_train_step_losses_and_grads) for model_default.npz, on the
    width fixtures: oracle.refmodel reads MOBILENET_BLOCKS at call time, the heads read the feature count from the weights."""
    from oracle.synth import digest_close
    from test_oracle_golden import _batches, _criterions

    oracle_width(monkeypatch, w)
    d, meta = load_golden(FIXTURES[w])
    assert meta["config"]["backbone_args"]["widen_factor"] == w
    shapes = {k: tuple(v) for k, v in meta["shapes"].items()}
    image, ids = make_inputs(meta["B"], seed=meta["input_seed"])
    # eval forward
    sd = make_state(shapes, meta["state_seed"])
    sd.update({k[len("calib/"):]: d[k] for k in d.files if k.startswith("calib/")})
    st = R.state_from_numpy(sd, requires_grad=False)
    with torch.no_grad():
        out, _ = R.network_forward(st, torch.from_numpy(image), torch.from_numpy(ids), meta["config"], False)
        out_noid, _ = R.network_forward(st, torch.from_numpy(image), None, meta["config"], False)
    for prefix, o in (("eval/", out), ("eval_noid/", out_noid)):
        keys = [k[len(prefix):] for k in d.files if k.startswith(prefix)]
        assert set(keys) == set(o.keys())
        for k in keys:
            np.testing.assert_allclose(o[k].numpy(), d[prefix + k], rtol=2e-4, atol=2e-5, err_msg=k)
    # train step: losses, outputs, features, gradients, running statistics
    crit, _ = _criterions(meta, golden_dir)
    for epoch in (0, 20, 150):
        st = R.state_from_numpy(make_state(shapes, meta["state_seed"]))
        out, feat = R.network_forward(st, torch.from_numpy(image), torch.from_numpy(ids), meta["config"], True)
        loss_sum, by_name = R.compute_loss(out, _batches(meta), epoch, crit)
        names = [k.split("/")[3] for k in d.files if k.startswith(f"train/e{epoch}/loss/") and k.endswith("/values")]
        assert list(by_name.keys()) == names
        for n in names:
            np.testing.assert_allclose(by_name[n][0].detach().numpy(), d[f"train/e{epoch}/loss/{n}/values"], rtol=3e-4, atol=3e-5, err_msg=n)
            np.testing.assert_allclose(by_name[n][1].detach().numpy(), d[f"train/e{epoch}/loss/{n}/weights"], rtol=1e-6, atol=0, err_msg=n)
        np.testing.assert_allclose(loss_sum.item(), d[f"train/e{epoch}/loss_sum"], rtol=1e-4)
    for k in [k for k in d.files if k.startswith("train/out/")]:
        np.testing.assert_allclose(out[k[len("train/out/"):]].detach().numpy(), d[k], rtol=3e-4, atol=3e-5, err_msg=k)
    assert feat.shape[1] == int(1024 * w)
    np.testing.assert_allclose(feat.detach().numpy(), d["train/features"], rtol=2e-4, atol=2e-5)
    loss_sum.backward()
    for k in [k for k in d.files if k.startswith("train/grad/")]:
        p = st[k[len("train/grad/"):]]
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        ok, msg = digest_close(d[k], g.numpy(), rtol=2e-3, atol=1e-7)
        assert ok, f"{k}: {msg}"
    for k in [k for k in d.files if k.startswith("train/after/")]:
        ok, msg = digest_close(d[k], st[k[len("train/after/"):]].detach().numpy(), rtol=1e-4, atol=1e-7)
        assert ok, f"{k}: {msg}"


def test_train_script_flag():
    S = train_script()
    args = S.make_parser().parse_args(["--widen-factor", "0.5"])
    net = S.create_net(args)
    assert net.get_config()["backbone_args"] == {"use_blurpool": False, "widen_factor": 0.5}
    assert net.convnet.num_features == 512 and net.boxnet.linear.in_features == 512
    args = S.make_parser().parse_args([])
    assert args.widen_factor == 1.0
    assert S.create_net(args).get_config()["backbone_args"] == {"use_blurpool": False}  # the default leaves the saved config as it was
    assert S.create_net(script_args({"with_pointhead": True, "with_nll_loss": False})).get_config()["backbone_args"] == {"use_blurpool": False}


def test_bf16_compute_refuses_other_widths():
    import trackertraincode.backbones.mobilenet_v1 as MB

    net = MB.MobileNet(num_classes=None, widen_factor=0.5)
    with pytest.raises(ValueError, match="widen_factor"):
        net.set_precision("bf16-compute")
    assert net.effective_precision() == "fp32"
    assert MB.MobileNet(num_classes=None, widen_factor=1.0).set_precision("bf16-compute").effective_precision() == "bf16-compute"
    MB.set_activation_dtype("bf16-compute")  # the module-wide default reaches the instance at the forward pass: refused there, no fallback
    try:
        with pytest.raises(ValueError, match="widen_factor"):
            net._check_width_precision(net.effective_precision())
    finally:
        MB.set_activation_dtype("fp32")


def test_block_layout_helpers():
    import trackertraincode._hip as H

    g = torch.Generator().manual_seed(1)
    for C in (8, 24, 48, 96, 32, 64, 256):
        t = torch.randn(3, 5, 7, C, generator=g)
        b = H.to_blocks_any(t)
        assert b.shape == t.shape and b.is_contiguous()
        assert torch.equal(H.from_blocks_any(b), t)
        if C % 32 == 0:
            assert torch.equal(b, H.to_blocks(t)) and torch.equal(H.from_blocks_any(b), H.from_blocks(b))
        # the layout formula of include/ttk.h: element (m, c) of block c >> 5 at  b * M * 32 + m * width(b) + (c & 31)
        M, flat, rows = 3 * 5 * 7, b.reshape(-1), t.reshape(-1, C)
        for m, c in ((0, 0), (M - 1, C - 1), (17, C // 2), (50, 7)):
            blk = c >> 5
            width = min(32, C - 32 * blk)
            assert flat[blk * M * 32 + m * width + (c & 31)] == rows[m, c]
    for C in (8, 16, 24):  # plain channels-last rows
        t = torch.randn(11, C, generator=g)
        assert torch.equal(H.to_blocks_any(t), t)


@pytest.mark.parametrize("w", sorted(FIXTURES))
def test_export_runs_on_a_width_scaled_checkpoint(w, tmp_path):
    """scripts/export_model.py (tests/test_export.py::test_convert_writes_traced_graph_and_contract) on a width-scaled network: denormal flush,
    BatchNorm folding, torch.jit.trace equal to the eager CPU eval path to 1e-5."""
    import importlib.util
    import os

    from util import PKG, build_net

    spec = importlib.util.spec_from_file_location("amd_export_script", os.path.join(PKG, "scripts", "export_model.py"))
    E = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(E)
    d, meta = load_golden(FIXTURES[w])
    cal = {k[len("calib/"):]: d[k] for k in d.files if k.startswith("calib/")}
    net = build_net(meta, "cpu", cal).eval()
    contract = E.convert_posemodel_onnx(net, str(tmp_path / "model.ckpt"), for_opentrack=True, check_tol=1e-5)
    assert contract["batchnorm_folded"] and contract["max_rel_delta_traced_vs_eager"] <= 1e-5
    traced = torch.jit.load(contract["file"])
    x = torch.from_numpy(make_inputs(1, seed=3)[0])
    wrapped = E.ModelForOpenTrack(net).eval()
    with torch.no_grad():
        for a, b in zip(wrapped(x), traced(x)):
            # folding BatchNorm into the convolutions moves fp32 roundings: the script's own criterion, 1e-5 of the tensor's scale
            a = getattr(a, "value", a).numpy()
            np.testing.assert_allclose(a, b.numpy(), rtol=0, atol=1e-5 * float(np.abs(a).max()))
