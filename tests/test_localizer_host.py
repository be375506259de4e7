"""LocalizerNet on the host: the reference's state dict (keys, order, shapes), its CPU forward in float32 and float64 against the
reference's own outputs (tests/golden/localizer.npz), the refusal of device training, the export script."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from trackertraincode.neuralnets.modelcomponents import CenterOfMass, CenterOfMassAndStd
from trackertraincode.neuralnets.models import LocalizerNet, load_localizer
from util import GOLDEN, PKG


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLDEN, "localizer.npz"))
    meta = json.loads(str(d["meta"]))
    return d, meta, {k: torch.from_numpy(d["sd/" + k]) for k in meta["keys"]}


def test_state_dict_is_the_references(gold):
    _, meta, sd = gold
    net = LocalizerNet()
    ours = net.state_dict()
    assert list(ours.keys()) == meta["keys"]
    assert [list(v.shape) for v in ours.values()] == meta["shapes"]
    assert "initial_stage.0.weight" in ours and "convnet.0.0.weight" in ours and "convnet.2.layers.1.num_batches_tracked" in ours
    assert float(ours["boxstddev.half_size"]) == 1.5 and net.input_resolution == (224, 288)
    net.load_state_dict(sd, strict=True)
    assert net.convnet[0] is net.initial_stage
    assert net.convnet[1][1].momentum == 0.001 and net.convnet[2].layers[1].momentum == 0.1
    assert [b.apply_residual for b in list(net.convnet)[2:14]] == [i == o and s == 1 for i, o, k, s, e in LocalizerNet.BLOCKS]


def test_cpu_forward_against_the_reference(gold):
    d, meta, sd = gold
    net = LocalizerNet()
    net.load_state_dict(sd, strict=True)
    net.eval()
    x = (torch.from_numpy(d["frames"]).to(torch.float32) * meta["mul"] + meta["add"])[:, None]
    with torch.no_grad():
        out32 = net(x)
        assert out32.shape == (3, 5) and net.attentionmap.shape == (3, 7, 9)
        assert np.abs(out32.double().numpy() - d["out64"]).max() <= 2 * float(d["fp32_dev"])
        assert np.abs(out32.numpy() - d["out32"]).max() <= float(d["fp32_dev"])
        inf = net.inference(x)
        assert torch.equal(inf["hasface"], torch.sigmoid(out32[:, 0])) and torch.equal(inf["roi"], out32[:, 1:])
        net = net.double()
        out64 = net(x.double())
        assert np.abs(out64.numpy() - d["out64"]).max() < 1e-12
        assert np.abs(net.attentionmap.numpy() - d["attention64"]).max() < 1e-12


def test_centre_of_mass_arithmetic():
    m = torch.zeros(1, 7, 9, dtype=torch.float64)
    m[0, 6, 8] = 1.0
    assert torch.equal(CenterOfMass(half_size=1.5)(m), torch.tensor([[1.5, 1.5]], dtype=torch.float64))
    mean, std = CenterOfMassAndStd(half_size=1.5)(m)
    # the reference's deviation: the unscaled position code (1, 1) against the scaled mean (1.5, 1.5)
    assert torch.allclose(std, torch.full((1, 2), (0.25 + 1.0e-4) ** 0.5, dtype=torch.float64), atol=1e-15)


def test_checkpoint_formats(tmp_path, gold):
    _, _, sd = gold
    plain, wrapped = str(tmp_path / "plain.ckpt"), str(tmp_path / "wrapped.ckpt")
    torch.save(sd, plain)
    torch.save({"state_dict": sd, "class_name": "LocalizerNet", "config": {}}, wrapped)
    a, b = load_localizer(plain), load_localizer(wrapped)
    assert not a.training and all(torch.equal(u, v) for u, v in zip(a.state_dict().values(), b.state_dict().values()))
    torch.save({"state_dict": sd, "class_name": "NetworkWithPointHead", "config": {}}, wrapped)
    with pytest.raises(ValueError, match="NetworkWithPointHead"):
        load_localizer(wrapped)


def test_export_script_writes_graph_and_contract(tmp_path):
    spec = importlib.util.spec_from_file_location("amd_export_script_loc", os.path.join(PKG, "scripts", "export_model.py"))
    E = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(E)
    torch.manual_seed(3)
    ckpt = str(tmp_path / "loc.ckpt")
    torch.save(LocalizerNet().state_dict(), ckpt)
    contract = E.convert_localizer(load_localizer(ckpt), ckpt)
    assert contract["file"] == str(tmp_path / "loc.pt") and os.path.exists(contract["file"])
    stored = json.load(open(str(tmp_path / "loc.contract.json")))
    assert stored == contract
    assert stored["inputs"] == [{"name": "x", "shape": [1, 1, 224, 288], "dtype": "float32"}]
    assert stored["outputs"] == [{"name": "logit_box", "shape": [1, 5], "dtype": "float32"}]
    assert stored["opset_version"] == 12 and stored["max_rel_delta_traced_vs_eager"] <= 1e-5
    x = torch.randn(1, 1, 224, 288)
    with torch.no_grad():
        assert torch.allclose(torch.jit.load(contract["file"])(x), load_localizer(ckpt)(x), atol=1e-5)
