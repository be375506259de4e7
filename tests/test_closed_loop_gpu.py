"""eval.ClosedLoopTracker against `Predictor`: every frame of a closed-loop track is what `Predictor.predict_batch` computes from the box
the tracker cropped that frame with (teacher forcing on the tracker's own roi_in: a free-running second implementation would diverge
chaotically with random weights and show nothing), and the boxes flow from frame to frame by the clamp and the `lost` rule.

Tolerances: the bounds of tests/track_cases.py evaluated on the network's raw outputs.  Against float64 (tests/track_ref.py) one bound;
against `Predictor` - whose back-transformation is apply_affine2d in float32 torch: the same sums of products with the same operand
magnitudes, a general matrix inverse instead of the closed form, atan2 / sin / cos of the same accuracy class - both sides lie within one
bound of the exact value, so they are held to TWICE the bound (the argument of tests/test_ensemble_predictor_gpu.py).

What "the same" forward means.  The eval forward of a row is bitwise repeatable for the same BATCH, but it is not independent of the other
rows of the batch: with the garbage magnitudes of network 1 (random weights, state seed 1; outputs of 10^2 .. 10^3 in the crop's [-1, 1]
coordinates) rows 0 and 2 of a batch move by 1.2 u in roi, 2.2 u in coord, 1.2 u in pose and 463 u in pt3d_68 (u = 2^-24, measured on an
MI355X) when rows 1 and 3 are cropped with another factor; network 0 is bitwise independent of them.  That is a property of the existing
forward, not of the tracker.  `Predictor(net, f).predict_batch` on the frames of all lanes crops EVERY row with f, so on a track that mixes
factors its batch is not the tracker's.  Hence: a mixed track is held to Predictor's arithmetic on the tracker's own batch - each lane's crop
and transform from `Predictor(net, factor of the lane).crop_batch`, one forward, `Predictor.to_image_coordinates` - which is what
predict_batch does with a batch; and tracks whose lanes share one factor (both videos, per factor) are held to `predict_batch` itself,
whose batch then is the tracker's row for row.  Every lane, frame and factor is compared both ways."""
import numpy as np
import pytest
import torch

import track_ref as TR
from track_cases import update_bounds, within
from util import build_net, gpu_section, load_golden

pytestmark = pytest.mark.gpu

T, HS, WS = 6, 96, 128
FIRST = [[40.0, 22.0, 92.0, 74.0], [34.5, 18.25, 88.0, 70.5]]  # one box per video, around the centre of the frame


@pytest.fixture(scope="module")
def nets():
    """Two half-width networks with the landmark head (state seeds 0, 1) and a full-width one without it."""
    g, meta = load_golden("model_w050.npz")
    cal = {k[len("calib/"):]: g[k] for k in g.files if k.startswith("calib/")}
    small = [build_net(dict(meta, state_seed=s), "cuda", cal).eval() for s in (0, 1)]
    g, meta = load_golden("model_posonly.npz")
    cal = {k[len("calib/"):]: g[k] for k in g.files if k.startswith("calib/")}
    return small, build_net(meta, "cuda", cal).eval()


@pytest.fixture(scope="module")
def video():
    rng = np.random.default_rng(123)
    return torch.from_numpy(rng.integers(0, 256, size=(2, T, HS, WS), dtype=np.uint8)), torch.tensor(FIRST, dtype=torch.float32)


@pytest.fixture(scope="module")
def tracks(nets, video):
    """One eager and one graphed track per half-width network: two videos x factors (1.0, 1.2) = four lanes; and one track per factor
    with the two videos as its lanes."""
    from trackertraincode import eval as E

    frames, first = video
    out = {}
    with gpu_section():
        for i, net in enumerate(nets[0]):
            out[i, "eager"] = E.ClosedLoopTracker(net).track(frames, first)
            out[i, "graphed"] = E.ClosedLoopTracker(net, graphed=True).track(frames, first)
            for f in (1.0, 1.2):
                out[i, f] = E.ClosedLoopTracker(net, factors=(f,)).track(frames, first)
    return out


def _np(t):
    return t.detach().cpu().numpy()


def _frame_against_predictor(net, frames, trk, t):
    """Frame t of a track against float64 and against Predictor's arithmetic, every lane; a track whose lanes share one factor also against
    `Predictor.predict_batch` itself."""
    from trackertraincode import eval as E

    lane_seq, lane_factor = _np(trk["lane_seq"]), _np(trk["lane_factor"])
    images = frames[torch.from_numpy(lane_seq.astype(np.int64)), t][:, None].cuda().contiguous()  # the frames of ALL lanes: batch size and row positions of the tracker
    rois = trk["roi_in"][t]
    factors = sorted(set(float(f) for f in lane_factor))
    with gpu_section(), torch.no_grad():
        preds = {f: E.Predictor(net, focus_roi_expansion_factor=f) for f in factors}
        crops = {f: p.crop_batch(images, rois) for f, p in preds.items()}
        # the tracker's batch row by row: every lane's crop and transform from the Predictor of its factor
        x = torch.stack([crops[float(f)]["image"][l] for l, f in enumerate(lane_factor)])
        tr = torch.stack([crops[float(f)]["image_transform"][l] for l, f in enumerate(lane_factor)])
        raw = net(x)
        N = preds[factors[0]].input_resolution
        want = {"to_image_coordinates on the tracker's batch": E.Predictor.to_image_coordinates(raw, tr, N)}
        if len(factors) == 1:
            want["predict_batch"] = preds[factors[0]].predict_batch(images, rois)
    case = {"tr": _np(tr), "N": N, "roi": _np(raw["roi"]), "coord": _np(raw["coord"]), "pose": _np(raw["pose"]),
            "pts": _np(raw["pt3d_68"]) if "pt3d_68" in raw else None, "lane_factor": lane_factor}
    r = TR.update(case["roi"], case["coord"], case["pose"], case["pts"], case["tr"], N, WS, HS, lane_factor, _np(rois))
    bd = update_bounds(case, r)
    print(f"frame {t}, factors {factors}")
    for key, rk in (("roi", "roi"), ("coord", "coord"), ("pose", "pose"), ("pt3d_68", "pts")):
        if r[rk] is None:
            assert key not in trk and all(key not in w for w in want.values())
            continue
        got = _np(trk[key][t]).astype(np.float64)
        within(f"{key} against float64", got, r[rk], bd[rk])
        for name, w in want.items():
            within(f"{key} against {name}", got, _np(w[key]).astype(np.float64), 2 * bd[rk])


def test_every_frame_is_what_predictor_computes_from_the_same_box(nets, video, tracks):
    frames, _ = video
    for i, net in enumerate(nets[0]):
        trk = tracks[i, "eager"]
        if i == 0:
            assert not bool(trk["lost"][0].any()), "the first boxes are chosen so that no lane of network 0 is lost on frame 0"
        # (network 1 - random weights, state seed 1 - predicts a box whose half size underflows against its centre, x0 == x1 in float32,
        # on every input: no first box keeps its lanes, and its frames exercise the lost path - each is still held to Predictor below)
        assert trk["roi_in"].shape == (T, 4, 4) and trk["lost"].shape == (T, 4) and trk["lost"].dtype == torch.bool
        assert trk["pt3d_68"].shape == (T, 4, 68, 3) and trk["coord"].shape == (T, 4, 3) and trk["pose"].shape == (T, 4, 4)
        assert _np(trk["lane_seq"]).tolist() == [0, 0, 1, 1] and np.allclose(_np(trk["lane_factor"]), [1.0, 1.2, 1.0, 1.2])
        print(f"network {i}: lost\n{_np(trk['lost']).astype(int)}")
        for t in range(T):
            _frame_against_predictor(net, frames, trk, t)
        for f in (1.0, 1.2):  # both videos with one factor: the batch of `Predictor(net, f).predict_batch` IS the tracker's
            assert _np(tracks[i, f]["lane_factor"]).tolist() == [np.float32(f)] * 2
            for t in range(T):
                _frame_against_predictor(net, frames, tracks[i, f], t)


def test_boxes_flow_by_the_clamp_and_the_lost_rule(tracks, video):
    _, first = video
    for i in (0, 1):
        trk = tracks[i, "eager"]
        roi_in, roi, lost = _np(trk["roi_in"]), _np(trk["roi"]), _np(trk["lost"])
        assert np.array_equal(roi_in[0], _np(first)[[0, 0, 1, 1]])
        for t in range(T - 1):
            clamped = TR.clamp(roi[t], WS, HS)  # float32 in, float32 out: the kernel's clamp exactly
            assert clamped.dtype == np.float32
            assert np.array_equal(roi_in[t + 1][~lost[t]], clamped[~lost[t]]), f"frame {t}: the next box is the clamp of the predicted one"
            assert np.array_equal(roi_in[t + 1][lost[t]], roi_in[t][lost[t]]), f"frame {t}: a lost lane keeps its box"
        assert np.isfinite(roi_in).all()


def test_single_frame_equals_predict_batch(nets, video):
    from trackertraincode import eval as E

    frames, first = video
    net = nets[0][0]
    with gpu_section():
        trk = E.ClosedLoopTracker(net).track(frames[:, :1], first)
    assert trk["roi"].shape == (1, 4, 4) and np.array_equal(_np(trk["roi_in"][0]), _np(first)[[0, 0, 1, 1]])
    _frame_against_predictor(net, frames, trk, 0)
    for f in (1.0, 1.2):
        with gpu_section():
            one = E.ClosedLoopTracker(net, factors=(f,)).track(frames[:, :1], first)
        _frame_against_predictor(net, frames, one, 0)  # against Predictor.predict_batch on the first boxes


def test_graphed_equals_eager_bitwise(tracks):
    for i in (0, 1):
        a, b = tracks[i, "eager"], tracks[i, "graphed"]
        assert sorted(a.keys()) == sorted(b.keys())
        for k in a.keys():
            assert torch.equal(a[k], b[k]), f"network {i}: {k} differs between the eager and the graphed track"


def test_position_only_network_returns_no_landmarks(nets, video):
    from trackertraincode import eval as E

    frames, first = video
    with gpu_section():
        trk = E.ClosedLoopTracker(nets[1], factors=(1.1,)).track(frames[0, :2], first[:1])  # [T,H,W]: one video
    assert "pt3d_68" not in trk and trk["pose"].shape == (2, 1, 4) and trk["lost"].shape == (2, 1)
    assert np.isfinite(_np(trk["coord"])).all()


def test_refusals(nets, video):
    from trackertraincode import eval as E

    frames, first = video
    net = nets[0][0]
    trk = E.ClosedLoopTracker(net)
    with pytest.raises(ValueError, match="1 to 16 lanes"):
        trk.track(frames, first, lanes=[(0, 1.0 + 0.01 * i) for i in range(17)])
    with pytest.raises(ValueError, match="1 to 16 lanes"):
        trk.track(frames, first, lanes=[])
    for bad in ([50.0, 20.0, 40.0, 60.0], [130.0, 20.0, 170.0, 60.0], [float("nan"), 20.0, 90.0, 60.0], [40.0, 20.0, 40.5, 20.5]):
        with pytest.raises(ValueError, match="first box"):
            trk.track(frames, torch.tensor([bad, FIRST[1]]))
    with pytest.raises(ValueError, match="area"):
        E.ClosedLoopTracker(net, resample="area")

    class NoBox(torch.nn.Module):
        input_resolution = net.input_resolution

        def forward(self, x):
            return {k: v for k, v in net(x).items() if k != "roi"}

    with gpu_section():
        with pytest.raises(ValueError, match="box head"):
            E.ClosedLoopTracker(NoBox()).track(frames, first)
