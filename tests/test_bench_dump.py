"""bench.py --dump-outputs on the CPU: what dump_outputs() writes for a small network, the float32 / float64 rule, and the fixed seeded
sample that keeps the files under 64 MB - the same call twice gives the same bytes."""
import os

import numpy as np
import torch

import bench


def _step():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.BatchNorm1d(32))
    loss = net(torch.randn(8, 64)).square().mean()
    loss.backward()
    return net, {"loss": loss, "mt_losses": {"rot": torch.rand(8), "pts/3d": torch.rand(8, dtype=torch.float64)}}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_writes_what_the_step_computed(tmp_path):
    net, out = _step()
    bench.dump_outputs(str(tmp_path), out, net)
    got = _load(str(tmp_path))
    want = {"loss", "mt_loss.rot", "mt_loss.pts_3d", "buffer.1.running_mean", "buffer.1.running_var"}
    want |= {f"{kind}.{n}" for n, _ in net.named_parameters() for kind in ("param", "grad")}
    assert set(got) == want
    assert got["loss"].dtype == np.float32 and got["loss"] == np.float32(out["loss"].item())
    assert got["mt_loss.pts_3d"].dtype == np.float64
    np.testing.assert_array_equal(got["grad.0.weight"], net[0].weight.grad.numpy())
    np.testing.assert_array_equal(got["param.1.bias"], net[1].bias.detach().numpy())


def test_dump_samples_large_outputs_the_same_way_every_time(tmp_path, monkeypatch):
    net = torch.nn.Linear(1 << 11, 1 << 10)  # 2^21 weights: above the 2^20 elements from which an array may be sampled
    net.weight.grad = torch.randn_like(net.weight)
    out = {"loss": torch.tensor(1.0), "mt_losses": {}}
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 << 20)
    bench.dump_outputs(str(tmp_path / "a"), out, net)
    bench.dump_outputs(str(tmp_path / "b"), out, net)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(v.nbytes for v in a.values()) <= 3 << 20
    assert a["param.weight"].size < net.weight.numel() and a["param.bias"].size == net.bias.numel()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    assert np.isin(a["param.weight"], net.weight.detach().numpy().reshape(-1)).all()
