"""Re-acquisition of lost lanes in closed loop: ttk_track_reacquire against its numpy rule (tests/localizer_ref.py), and
eval.ClosedLoopTracker with a localizer against a host loop."""
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

NAN, INF = float("nan"), float("inf")


def _reacquire(loc, lb, t_dev, lane_seq, lane_factor, lost, after, thr, roi_state, lost_run, T, Hs, Ws):
    """One launch on copies; returns the device state and output rows as numpy."""
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()
    S, L = len(loc), len(lane_seq)
    st, run = dev(roi_state, np.float32), dev(lost_run, np.int32)
    re = torch.full((T, L), 9, dtype=torch.uint8, device="cuda")
    hf, roi = torch.full((T, S), -7.0, device="cuda"), torch.full((T, S, 4), -7.0, device="cuda")
    keep = [dev(loc, np.float32), dev(lb, np.float32), dev(t_dev, np.int32), dev(lane_seq, np.int32), dev(lane_factor, np.float32), dev(lost, np.uint8)]
    H.lib().call("ttk_track_reacquire", H.ptr(keep[0]), H.ptr(keep[1]), H.ptr(keep[2]), L, S, T, Hs, Ws, H.ptr(keep[3]), H.ptr(keep[4]), H.ptr(keep[5]),
                 after, thr, H.ptr(st), H.ptr(run), H.ptr(re), H.ptr(hf), H.ptr(roi))
    torch.cuda.synchronize()
    return st.cpu().numpy(), run.cpu().numpy(), re.cpu().numpy(), hf.cpu().numpy(), roi.cpu().numpy()


@pytest.mark.parametrize("L", [1, 16])
def test_kernel_against_the_numpy_rule(L):
    """Runs of lost frames below, at and above reacquire_after; logits on both sides of the threshold and NaN; boxes that are inverted,
    non-finite, outside the image or too small for the lane's factor."""
    T, Hs, Ws, S, after, thr = 5, 120, 160, 4, 3, 0.6
    good, big = (-0.5, -0.5, 0.5, 0.5), (-1.4, -1.2, 1.3, 1.4)
    # sequences: a face in a good box; the same below the threshold / NaN; bad boxes of every kind (by frame, below)
    boxes = {0: [good] * 5, 1: [big] * 5, 2: [good] * 5,
             3: [(0.5, -0.5, -0.5, 0.5), (NAN, 0.0, 0.5, 0.5), (-0.5, -0.5, INF, 0.5), (1.2, -0.3, 1.6, 0.3), (0.0, 0.0, 0.004, 0.004)]}
    logits = {0: [2.0] * 5, 1: [0.41, 0.40, 0.42, 3.0, -4.0], 2: [NAN, 0.3, NAN, 0.2, NAN], 3: [5.0] * 5}  # sigmoid(0.405) = 0.6
    rng = np.random.default_rng(L)
    lane_seq = [l % S for l in range(L)]
    lane_factor = [1.0 + 0.1 * (l % 3) for l in range(L)]
    lb = np.tile(np.asarray(R.letterbox_geometry(Hs, Ws), dtype=np.float32), (S, 1))
    state0 = np.tile(np.array([30, 20, 90, 80], dtype=np.float32), (L, 1))
    for t in range(T):
        loc = np.array([[logits[q][t], *boxes[q][t]] for q in range(S)], dtype=np.float32)
        lost = np.zeros((T, L), dtype=np.uint8)
        lost[t] = rng.integers(0, 4, L) > 0  # mostly lost
        run0 = rng.integers(0, 5, L)         # below, at and above reacquire_after - 1
        got = _reacquire(loc, lb, t + 1, lane_seq, lane_factor, lost, after, thr, state0, run0, T, Hs, Ws)
        st, run, re, hf, roi = R.reacquire_rule(loc, lb, lost[t], lane_seq, lane_factor, state0, run0, Hs, Ws, after, thr)
        np.testing.assert_array_equal(got[0], st)
        np.testing.assert_array_equal(got[1], run)
        np.testing.assert_array_equal(got[2][t], re.astype(np.uint8))
        np.testing.assert_allclose(got[3][t], hf, rtol=1e-6, equal_nan=True)
        np.testing.assert_array_equal(got[4][t], roi)
        other = [u for u in range(T) if u != t]
        assert np.all(got[2][other] == 9) and np.all(got[3][other] == -7.0) and np.all(got[4][other] == -7.0)  # the other rows stay
    # every branch of the rule was taken by some lane and frame
    loc = np.array([[logits[q][0], *boxes[q][0]] for q in range(S)], dtype=np.float32)
    lost = np.ones((T, L), dtype=np.uint8)
    got = _reacquire(loc, lb, 1, lane_seq, lane_factor, lost, after, thr, state0, np.full(L, 2), T, Hs, Ws)
    assert got[2][0][0] == 1 and np.all(got[0][0] == R.candidate(R.box_to_frame(loc[0, 1:], lb[0]), 1.0, Ws, Hs)[0])


def test_counter_out_of_range_writes_nothing():
    T, Hs, Ws = 3, 120, 160
    loc = np.array([[3.0, -0.5, -0.5, 0.5, 0.5]], dtype=np.float32)
    lb = np.asarray([R.letterbox_geometry(Hs, Ws)], dtype=np.float32)
    for t_dev in (0, T + 1, -5):  # t = t_dev - 1 outside [0, T)
        st, run, re, hf, roi = _reacquire(loc, lb, t_dev, [0], [1.0], np.ones((T, 1)), 1, 0.5, [[1, 2, 3, 4]], [4], T, Hs, Ws)
        assert np.all(st == [[1, 2, 3, 4]]) and run[0] == 4 and np.all(re == 9) and np.all(hf == -7.0) and np.all(roi == -7.0)


def test_refusals():
    z = torch.zeros(64, device="cuda")
    zi = torch.zeros(64, dtype=torch.int32, device="cuda")
    zb = torch.zeros(64, dtype=torch.uint8, device="cuda")
    P = H.ptr
    ok = lambda **kw: dict(dict(loc=P(z), L=1, after=3), **kw)
    for a in (ok(L=0), ok(L=17), ok(loc=None), ok(after=0)):
        with pytest.raises(RuntimeError, match="track_reacquire"):
            H.lib().call("ttk_track_reacquire", a["loc"], P(z), P(zi), a["L"], 1, 2, 10, 10, P(zi), P(z), P(zb), a["after"], 0.5, P(z), P(zi), P(zb), P(z), P(z))


# ---- the tracker ------------------------------------------------------------------------------------
T, HS, WS, LANES = 12, 60, 80, 4
THRESHOLD = 0.05


class ScriptedPoseNet(torch.nn.Module):
    """A stand-in for the pose network: frame t of the test video has grey levels in [8 t + 1, 8 t + 6], so the crop's centre pixel
    tells the frame on the device (graph capturable), and the module returns the planned box of that frame and lane."""

    input_resolution = 129
    enable_point_head = False

    def __init__(self, plan):
        super().__init__()
        L = len(plan[0])
        self.register_buffer("plan", torch.as_tensor(plan, dtype=torch.float32))
        self.register_buffer("lanes", torch.arange(L))
        self.register_buffer("coord", torch.tensor([0.0, 0.0, 0.5]).expand(L, 3).contiguous())
        self.register_buffer("pose", torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(L, 4).contiguous())

    def forward(self, crop):
        N = crop.shape[-1]  # (device tensors only: nothing here may copy from the host while a graph is captured)
        t = torch.clamp(torch.floor((crop[:, 0, N // 2, N // 2] + 0.5) * 32.0).long(), 0, self.plan.shape[0] - 1)
        return {"roi": self.plan[t, self.lanes], "coord": self.coord, "pose": self.pose}


@pytest.fixture(scope="module")
def setup():
    d = np.load(os.path.join(GOLDEN, "localizer.npz"))
    meta = json.loads(str(d["meta"]))
    loc = LocalizerNet()
    loc.load_state_dict({k: torch.from_numpy(d["sd/" + k]) for k in meta["keys"]}, strict=True)
    rng = np.random.default_rng(77)
    frames = rng.integers(1, 7, (2, T, HS, WS)).astype(np.uint8) + (8 * np.arange(T, dtype=np.uint8))[None, :, None, None]
    good = [-0.9, -0.85, 0.85, 0.9]  # nearly the crop itself: the boxes neither collapse nor run away within T frames
    plan = np.tile(np.array(good, dtype=np.float32), (T, LANES, 1))
    plan[2:7, 0] = NAN                      # lane 0: lost on frames 2..6: re-acquired on frame 4, lost again on 5, 6
    plan[1:3, 1] = [0.5, -0.5, -0.6, 0.6]   # lane 1: inverted on frames 1, 2: the run stays below reacquire_after
    plan[3:, 2] = [0.1, 0.1, INF, 0.5]      # lane 2: lost from frame 3 on: re-acquired on frames 5, 8, 11
    first = torch.tensor([[20.0, 10.0, 60.0, 50.0], [25.0, 12.0, 66.0, 52.0]])
    return loc, torch.from_numpy(frames), plan, first


def _np(v):
    return v.detach().cpu().numpy()


def test_tracker_with_a_localizer_against_a_host_loop(setup):
    from trackertraincode import eval as E

    loc, frames, plan, first = setup
    kw = dict(localizer=loc, reacquire_after=3, face_threshold=THRESHOLD)
    trk = E.ClosedLoopTracker(ScriptedPoseNet(plan), **kw).track(frames, first)
    graphed = E.ClosedLoopTracker(ScriptedPoseNet(plan), graphed=True, **kw).track(frames, first)
    for k in ("roi_in", "roi", "coord", "pose", "lost", "reacquired", "hasface", "loc_roi"):
        assert torch.equal(trk[k], graphed[k]) or (k in ("roi",) and np.array_equal(_np(trk[k]), _np(graphed[k]), equal_nan=True)), k
    # the host loop: the localizer on every frame (one batch), the box rule on the tracker's own recorded predictions, the numpy rule
    found = E.Localizer(loc).localize(frames.reshape(2 * T, HS, WS))
    loc_out = np.concatenate([_np(found["logit"])[:, None], _np(found["roi_normalized"])], axis=1).reshape(2, T, 5)
    lb = _np(found["letterbox"]).reshape(2, T, 3)
    np.testing.assert_array_equal(_np(trk["loc_roi"]), _np(found["roi"]).reshape(2, T, 4).transpose(1, 0, 2))
    np.testing.assert_allclose(_np(trk["hasface"]), _np(found["hasface"]).reshape(2, T).T, rtol=1e-6)
    lane_seq, lane_factor = _np(trk["lane_seq"]), _np(trk["lane_factor"])
    assert list(lane_seq) == [0, 0, 1, 1] and np.allclose(lane_factor, [1.0, 1.2, 1.0, 1.2])
    state, run = _np(first)[lane_seq].copy(), np.zeros(LANES, dtype=np.int32)
    for t in range(T):
        np.testing.assert_array_equal(_np(trk["roi_in"][t]), state, err_msg=f"frame {t}")
        lost = np.zeros(LANES, dtype=bool)
        for l in range(LANES):
            c, valid = R.candidate(_np(trk["roi"][t, l]), lane_factor[l], WS, HS)
            ordered = plan[t, l, 2] > plan[t, l, 0] and plan[t, l, 3] > plan[t, l, 1]
            lost[l] = not (valid and ordered)
            if not lost[l]:
                state[l] = c
        np.testing.assert_array_equal(_np(trk["lost"][t]), lost, err_msg=f"frame {t}")
        state, run, re, _, _ = R.reacquire_rule(loc_out[:, t], lb[:, t], lost, lane_seq, lane_factor, state, run, HS, WS, 3, THRESHOLD)
        np.testing.assert_array_equal(_np(trk["reacquired"][t]), re, err_msg=f"frame {t}")
    # the plan did what it was written for
    lost, re = _np(trk["lost"]), _np(trk["reacquired"])
    assert list(np.flatnonzero(lost[:, 0])) == [2, 3, 4, 5, 6] and list(np.flatnonzero(re[:, 0])) == [4]
    assert list(np.flatnonzero(lost[:, 1])) == [1, 2] and not re[:, 1].any()
    assert list(np.flatnonzero(re[:, 2])) == [5, 8, 11] and not lost[:, 3].any() and not re[:, 3].any()
    good = R.candidate(_np(found["roi"]).reshape(2, T, 4)[0, 4], 1.0, WS, HS)[0]
    np.testing.assert_array_equal(_np(trk["roi_in"][5, 0]), good)  # frame 5 of lane 0 is cropped with the localizer's box of frame 4


def test_tracker_without_a_localizer_has_no_new_outputs(setup):
    from trackertraincode import eval as E

    _, frames, plan, first = setup
    trk = E.ClosedLoopTracker(ScriptedPoseNet(plan)).track(frames, first)
    assert "reacquired" not in trk and "hasface" not in trk and "loc_roi" not in trk
    assert list(np.flatnonzero(_np(trk["lost"][:, 2]))) == list(range(3, T))  # lost for the rest of the video
    with pytest.raises(ValueError, match="first_rois"):
        E.ClosedLoopTracker(ScriptedPoseNet(plan)).track(frames)


def test_first_boxes_from_the_localizer(setup):
    from trackertraincode import eval as E

    loc, frames, plan, _ = setup
    trk = E.ClosedLoopTracker(ScriptedPoseNet(plan), localizer=loc, face_threshold=THRESHOLD).track(frames)
    found = _np(E.Localizer(loc).localize(frames[:, 0])["roi"])
    for l, q in enumerate(_np(trk["lane_seq"])):
        np.testing.assert_array_equal(_np(trk["roi_in"][0, l]), R.candidate(found[q], 1.0, WS, HS)[0])
    with pytest.raises(ValueError, match="sequence 0"):
        E.ClosedLoopTracker(ScriptedPoseNet(plan), localizer=loc, face_threshold=1.0).track(frames)
