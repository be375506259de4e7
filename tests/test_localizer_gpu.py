"""The localizer's whole forward on the device against the reference's float64 outputs (tests/golden/localizer.npz), its repeatability
and graph capture, and `eval.Localizer`."""
import json
import os

import numpy as np
import pytest
import torch

import localizer_ref as R
import trackertraincode._hip as H
from trackertraincode.neuralnets.models import LocalizerNet
from util import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLDEN, "localizer.npz"))
    meta = json.loads(str(d["meta"]))
    net = LocalizerNet()
    net.load_state_dict({k: torch.from_numpy(d["sd/" + k]) for k in meta["keys"]}, strict=True)
    return d, meta, net.cuda().eval()


def _inputs(d, meta, B):
    idx = np.arange(B) % 3
    x = (torch.from_numpy(d["frames"][idx]).to(torch.float32) * meta["mul"] + meta["add"])[:, None]
    return x.cuda().contiguous(), idx


@pytest.mark.parametrize("B", [1, 3, 17])
def test_forward_against_the_reference(gold, B):
    d, meta, net = gold
    x, idx = _inputs(d, meta, B)
    tol = 4 * float(d["fp32_dev"])
    with torch.no_grad():
        out = net(x)
        att = net.attentionmap
        again = net(x)
        assert torch.equal(out, again) and torch.equal(att, net.attentionmap)  # two runs: bitwise
    e_out = float(np.abs(out.cpu().double().numpy() - d["out64"][idx]).max())
    e_att = float(np.abs(att.cpu().double().numpy() - d["attention64"][idx]).max())
    print(f"forward B={B}: out {e_out:.3e} attention {e_att:.3e} (bound {tol:.3e})")
    assert out.shape == (B, 5) and att.shape == (B, 7, 9)
    assert e_out <= tol and e_att <= tol


def test_packed_parameters_follow_the_restatement_and_the_versions(gold):
    d, meta, net = gold
    packed = net.packed_parameters("cuda")
    assert packed.numel() == H.lib().cdll.ttk_localizer_param_floats()
    ref = R.packed_parameters({k: d["sd/" + k] for k in meta["keys"]})
    assert torch.equal(packed.cpu(), ref)
    assert net.packed_parameters("cuda") is packed  # nothing changed: not packed again
    with torch.no_grad():
        net.convnet[14].bias.add_(0.0)  # an in-place write raises the tensor's version
    assert net.packed_parameters("cuda") is not packed


def test_forward_launches_and_graph_replay(gold):
    d, meta, net = gold
    assert 1 <= H.lib().cdll.ttk_localizer_launches() <= 16
    x, _ = _inputs(d, meta, 3)
    with torch.no_grad():
        eager = net(x).clone()
        eager_att = net.attentionmap.clone()
        torch.cuda.synchronize()
        with H.CAPTURE_LOCK:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = net(x)
                att = net.attentionmap
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(att, eager_att)


def test_training_on_the_device_is_refused(gold):
    _, _, net = gold
    net.train()
    try:
        with pytest.raises(NotImplementedError, match="training"):
            net(torch.zeros((1, 1, 224, 288), device="cuda"))
    finally:
        net.eval()


@pytest.mark.parametrize("Hs,Ws", [(60, 80), (224, 288), (100, 300)])
def test_localize_maps_the_boxes_to_frame_pixels(gold, Hs, Ws):
    from trackertraincode import eval as E

    _, _, net = gold
    rng = np.random.default_rng(Ws)
    frames = torch.from_numpy(rng.integers(0, 256, (4, Hs, Ws), dtype=np.uint8))
    loc = E.Localizer(net)
    got = loc.localize(frames)
    as_float = loc.localize(frames.to(torch.float32))
    for k in ("logit", "hasface", "roi", "roi_normalized"):
        assert torch.equal(got[k], as_float[k]), k
    lb = np.tile(np.asarray(R.letterbox_geometry(Hs, Ws), dtype=np.float32), (4, 1))
    np.testing.assert_array_equal(got["letterbox"].cpu().numpy(), lb)
    want = R.box_to_frame(got["roi_normalized"].cpu().numpy(), lb)
    np.testing.assert_array_equal(got["roi"].cpu().numpy(), want)
    np.testing.assert_allclose(got["hasface"].cpu().numpy(), R.sigmoid32(got["logit"].cpu().numpy()), rtol=1e-6)
    assert got["logit"].shape == (4,) and got["roi"].shape == (4, 4)
    # the network's own outputs: the forward on the restatement's letterbox
    x = torch.stack([torch.from_numpy(R.letterbox(f.numpy(), R.MUL, R.ADD)[0]) for f in frames])[:, None].to(torch.float32).cuda()
    with torch.no_grad():
        direct = net(x)
    # (the kernel's input differs from the float64 letterbox by float32 rounding only: the outputs agree to a few 1e-5)
    assert float((direct[:, 1:] - got["roi_normalized"]).abs().max()) < 1e-3
