"""ttk_track_crop / ttk_track_update (csrc/track.hip) through the C-ABI on guarded buffers.  The crop is compared bitwise with the three
launches it replaces; the update with tests/track_ref.py in float64 on the same float32 inputs, inside the bounds derived in
tests/track_cases.py; validity decisions exactly."""
import numpy as np
import pytest
import torch

import track_ref as TR
from head_loss_cases import Guarded
from track_cases import (FILL_I32, FILL_U8, IntGuarded, _f32, crop_case, decisions_are_safe, run_crop, run_update, three_launches, update_bounds,
                         update_case, within)
from util import gpu_section

pytestmark = pytest.mark.gpu


def _nan_outside(out, name, rows, width, keep):
    """Row `keep` of a [rows][width] trajectory buffer aside, everything - the guard words included - still holds its NaN fill."""
    full, numel = out.bufs[name]
    mask = torch.ones(full.numel(), dtype=torch.bool)
    if keep is not None:
        mask[keep * width:(keep + 1) * width] = False
    assert bool(full.cpu()[mask].isnan().all()), f"{name}: written outside row {keep}"


# ---------------------------------------------------------------------------------------------
# ttk_track_crop
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("N", [17, 129])
@pytest.mark.parametrize("L", [1, 3, 16])
def test_crop_is_bitwise_the_three_launches(L, N, dtype):
    case = crop_case(L, dtype, seed=10 * L + N)
    for t in (0, case["T"] - 1):
        with gpu_section():
            out, ints = run_crop(case, N, t)
            view, tr, crop = three_launches(case, N, t)
        out.check(f"L={L} N={N} {dtype} t={t}")
        assert torch.equal(ints.get("view").view(L, 4), view), "view_roi"
        assert torch.equal(out.get("tr").view(L, 2, 3), tr), "tr"
        assert torch.equal(out.get("crop").view(L, 1, N, N), crop), "crop"
        assert ints.guard_intact("view") and ints.guard_intact("t")
        assert int(ints.get("t")[0]) == t, "the crop must not advance the counter"
        assert torch.equal(out.get("roi_state").cpu(), torch.from_numpy(case["roi_state"]).reshape(-1)), "the crop must not touch roi_state"
        # the cases do what they are meant to: zero padding somewhere, image content somewhere
        assert bool((crop == -0.5).any()) or L == 1
        assert bool((crop != -0.5).any())


@pytest.mark.parametrize("t", [3, -1])
def test_crop_outside_the_video_writes_nothing(t):
    case = crop_case(3, "u8", seed=7)
    with gpu_section():
        out, ints = run_crop(case, 17, t)
    for name in ("tr", "crop"):
        assert bool(out.bufs[name][0].isnan().all()), name
    assert bool((ints.bufs["view"][0] == FILL_I32).all()) and int(ints.get("t")[0]) == t


@pytest.mark.parametrize("L", [0, 17])
def test_crop_refuses_lane_counts_out_of_range(L):
    case = crop_case(16, "u8", seed=8)
    with gpu_section():
        with pytest.raises(RuntimeError, match="lanes"):
            run_crop(case, 17, 0, L=L)
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# ttk_track_update
# ---------------------------------------------------------------------------------------------
def _check_update(case, t, what):
    L, T = case["L"], case["T"]
    r = TR.update(case["roi"], case["coord"], case["pose"], case["pts"], case["tr"], case["N"], case["Ws"], case["Hs"], case["lane_factor"],
                  case["roi_state"])
    bd = update_bounds(case, r)
    decisions_are_safe(case, r, bd)
    with gpu_section():
        out, ints = run_update(case, t)
    print(what)
    f64 = lambda name, *shape: out.get(name).cpu().numpy().reshape(*shape).astype(np.float64)
    within("roi", f64("traj_roi", T, L, 4)[t], r["roi"], bd["roi"])
    within("coord", f64("traj_coord", T, L, 3)[t], r["coord"], bd["coord"])
    within("pose", f64("traj_pose", T, L, 4)[t], r["pose"], bd["pose"])
    if case["pts"] is not None:
        within("pts", f64("traj_pts", T, L, 68, 3)[t], r["pts"], bd["pts"])
    assert np.array_equal(out.get("roi_in").cpu().numpy().reshape(T, L, 4)[t], case["roi_state"]), "roi_in is the state before the update"
    lost = ints.get("lost").cpu().numpy().reshape(T, L)
    assert np.array_equal(lost[t], r["lost"].astype(np.uint8)), (lost[t], r["lost"])
    state = f64("roi_state", L, 4)
    assert np.array_equal(state[r["lost"]], case["roi_state"][r["lost"]].astype(np.float64)), "a lost lane keeps its box"
    within("next state", state[~r["lost"]], r["cand"][~r["lost"]], bd["roi"][~r["lost"]])
    # row t and nothing else
    for name, width in (("roi_in", 4), ("traj_roi", 4), ("traj_coord", 3), ("traj_pose", 4)) + ((("traj_pts", 204),) if case["pts"] is not None else ()):
        _nan_outside(out, name, T, L * width, t)
    assert np.all(np.delete(lost, t, axis=0) == FILL_U8) and ints.guard_intact("lost")
    assert int(ints.get("t")[0]) == t + 1 and ints.guard_intact("t")
    assert bool(out.bufs["roi_state"][0][L * 4:].isnan().all())
    return r, out, ints


@pytest.mark.parametrize("pts", [True, False])
@pytest.mark.parametrize("L", [1, 3, 16])
def test_update_matches_float64(L, pts):
    """Axis-aligned transforms as the tracker makes them; with L >= 3 lane 1 rotated by 0.4 rad and lane 2 mirrored (flip map)."""
    case = update_case(L, seed=200 + L, pts=pts)
    if L >= 3:
        assert np.linalg.det(case["tr"][2, :, :2].astype(np.float64)) < 0
    r, _, _ = _check_update(case, t=2, what=f"L={L} pts={pts}")
    assert not r["lost"].any()


def test_update_first_and_last_frame():
    case = update_case(3, seed=31)
    _check_update(case, t=0, what="t=0")
    _check_update(case, t=case["T"] - 1, what="t=T-1")


def test_update_lost_rows():
    """Lane 0 inverted, 1 NaN in the box, 2 Inf in the box, 3 wholly right of the image, 4 half a pixel wide and high, 5 NaN only in the
    pose (NOT lost), 6 ordinary.  All axis-aligned."""
    case = update_case(7, seed=41, special=False)
    roi = case["roi"]
    roi[0] = roi[0][[2, 1, 0, 3]]
    roi[1, 0] = np.nan
    roi[2, 2] = np.inf
    case["roi_state"][3] = _f32([100.0, 30.0, 126.0, 56.0])  # the view box reaches to x = 126; the prediction lies right of x = 128
    case["tr"][3] = TR.roi_transform(TR.view_roi_f32(case["roi_state"][3:4], case["lane_factor"][3:4])[0], case["N"], np.float32)[0]
    roi[3] = _f32([1.4, -0.3, 1.9, 0.3])
    roi[4] = _f32([0.1, 0.1, 0.1 + case["tr"][4, 0, 0] / case["N"], 0.1 + case["tr"][4, 1, 1] / case["N"]])  # 0.5 image pixels: dx_image = dx N / 2 / tr_00
    case["pose"][5, 1] = np.nan
    r, out, _ = _check_update(case, t=1, what="lost rows")
    assert r["lost"].tolist() == [True, True, True, True, True, False, False]
    assert np.all(r["cand"][3, 2] - r["cand"][3, 0] < 0) and abs((r["roi"][4, 2] - r["roi"][4, 0]) - 0.5) < 1e-3
    assert np.isnan(out.get("traj_pose").cpu().numpy().reshape(case["T"], 7, 4)[1, 5]).any()


@pytest.mark.parametrize("how", ["L=0", "L=17", "pts without traj_pts"])
def test_update_refusals_write_nothing(how):
    case = update_case(16, seed=51)
    with gpu_section():
        with pytest.raises(RuntimeError, match="together" if "pts" in how else "lanes"):
            run_update(case, 1, L={"L=0": 0, "L=17": 17}.get(how), with_traj_pts=False if "pts" in how else None)
        torch.cuda.synchronize()
    # (run_update raised before it returned its buffers: the refusal is shown on fresh ones)
    from trackertraincode._hip import lib, ptr

    dev = {k: torch.from_numpy(case[k]).cuda() for k in ("roi", "coord", "pose", "pts", "tr", "lane_factor")}
    out, ints = Guarded(), IntGuarded()
    T, L = case["T"], 16
    args = [ptr(dev["roi"]), ptr(dev["coord"]), ptr(dev["pose"]), ptr(dev["pts"]), ptr(dev["tr"]), ints("t", 1, torch.int32, FILL_I32, [1]),
            {"L=0": 0, "L=17": 17}.get(how, L), case["N"], T, case["Hs"], case["Ws"], ptr(dev["lane_factor"]), out("roi_state", L * 4),
            out("roi_in", T * L * 4), out("traj_roi", T * L * 4), out("traj_coord", T * L * 3), out("traj_pose", T * L * 4),
            None if "pts" in how else out("traj_pts", T * L * 204), ints("lost", T * L, torch.uint8, FILL_U8)]
    with gpu_section():
        with pytest.raises(RuntimeError):
            lib().call("ttk_track_update", *args)
        torch.cuda.synchronize()
    for name, (full, _) in out.bufs.items():
        assert bool(full.isnan().all()), f"{name} was written by a refused call"
    assert bool((ints.bufs["lost"][0] == FILL_U8).all()) and int(ints.get("t")[0]) == 1


@pytest.mark.parametrize("t", [5, -1])
def test_update_outside_the_video_writes_nothing(t):
    case = update_case(3, seed=61)
    with gpu_section():
        out, ints = run_update(case, t)
    for name in ("roi_in", "traj_roi", "traj_coord", "traj_pose", "traj_pts"):
        assert bool(out.bufs[name][0].isnan().all()), name
    assert int(ints.get("t")[0]) == t and bool((ints.bufs["lost"][0] == FILL_U8).all())
    assert torch.equal(out.get("roi_state").cpu(), torch.from_numpy(case["roi_state"]).reshape(-1))


# ---------------------------------------------------------------------------------------------
# chain: crop -> a fixed table of "predictions" -> update, four frames
# ---------------------------------------------------------------------------------------------
def _chain_table(L, frames, seed):
    rng = np.random.default_rng(seed)
    table = []
    for t in range(frames):
        ctr, sz = rng.uniform(-0.15, 0.15, (L, 2)), rng.uniform(0.85, 1.05, (L, 2))  # boxes about as large as the view box
        roi = _f32(np.concatenate([ctr - sz, ctr + sz], -1))
        if t == 1:
            roi[1] = roi[1][[2, 1, 0, 3]]  # lane 1 is lost on frame 1 and recovers on frame 2
        q = rng.standard_normal((L, 4))
        table.append((roi, _f32(np.concatenate([ctr, rng.uniform(0.3, 0.6, (L, 1))], -1)), _f32(q / np.linalg.norm(q, axis=-1, keepdims=True)),
                      _f32(rng.uniform(-1.0, 1.0, (L, 68, 3)))))
    return table


def _run_chain(case, table, N):
    from trackertraincode._hip import lib, ptr

    L, T, S = case["L"], len(table), case["S"]
    f32 = dict(dtype=torch.float32, device="cuda")
    dev = {k: torch.from_numpy(case[k]).cuda() for k in ("frames", "lane_seq", "lane_factor", "roi_state")}
    t_dev = torch.zeros((), dtype=torch.int32, device="cuda")
    view, tr, crop = torch.empty((L, 4), dtype=torch.int32, device="cuda"), torch.empty((L, 2, 3), **f32), torch.empty((L, 1, N, N), **f32)
    traj = {"roi_in": torch.zeros((T, L, 4), **f32), "roi": torch.zeros((T, L, 4), **f32), "coord": torch.zeros((T, L, 3), **f32),
            "pose": torch.zeros((T, L, 4), **f32), "pts": torch.zeros((T, L, 68, 3), **f32), "lost": torch.full((T, L), 9, dtype=torch.uint8, device="cuda")}
    preds = [[torch.from_numpy(a).cuda() for a in row] for row in table]
    trs = []
    for row in preds:  # no host read inside the loop
        lib().call("ttk_track_crop", ptr(dev["frames"]), 1, S, case["T"], case["Hs"], case["Ws"], ptr(dev["lane_seq"]), ptr(dev["lane_factor"]),
                   ptr(dev["roi_state"]), ptr(t_dev), L, N, 1.0 / 256.0, -0.5, ptr(view), ptr(tr), ptr(crop))
        trs.append(tr.clone())
        lib().call("ttk_track_update", ptr(row[0]), ptr(row[1]), ptr(row[2]), ptr(row[3]), ptr(tr), ptr(t_dev), L, N, case["T"], case["Hs"], case["Ws"],
                   ptr(dev["lane_factor"]), ptr(dev["roi_state"]), ptr(traj["roi_in"]), ptr(traj["roi"]), ptr(traj["coord"]), ptr(traj["pose"]),
                   ptr(traj["pts"]), ptr(traj["lost"]))
    torch.cuda.synchronize()
    traj.update(t=t_dev, state=dev["roi_state"], tr=torch.stack(trs))
    return traj


def test_chain_of_four_frames():
    N, L = 17, 3
    case = crop_case(L, "u8", seed=71, T=4)
    case["roi_state"] = _f32([[14.3, 9.6, 39.2, 31.1], [20.5, 8.0, 44.25, 30.5], [10.0, 6.5, 33.5, 33.0]])
    table = _chain_table(L, 4, seed=72)
    ref, t_ref = TR.track(case["roi_state"], case["lane_factor"], table, N, case["Ws"], case["Hs"])
    with gpu_section():
        a = _run_chain(case, table, N)
        b = _run_chain(case, table, N)
    assert int(a["t"]) == t_ref == 4
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: two runs differ"
    lost = a["lost"].cpu().numpy()
    assert [bool(o["lost"][1]) for o in ref] == [False, True, False, False] and not any(o["lost"][[0, 2]].any() for o in ref)
    for t, o in enumerate(ref):
        frac = np.abs(o["view_pre"] - np.floor(o["view_pre"]) - 0.5)
        # (frame 0 starts from the same float32 boxes on both sides - one of them on an exact tie, rounded half to even by both)
        assert t == 0 or frac.min() > 1e-3, "a view box sits on a rounding tie: choose other inputs"
        assert np.array_equal(a["tr"][t].cpu().numpy(), o["tr"]), f"frame {t}: the crop transform follows the state"
        step = dict(case, roi=table[t][0], coord=table[t][1], pose=table[t][2], pts=table[t][3], tr=o["tr"], N=N)
        bd = update_bounds(step, o)
        decisions_are_safe(step, o, bd)
        print(f"frame {t}")
        # the state entering frame t carries the bound of the box it came from (the clamp is 1-Lipschitz); first boxes are exact
        prev = np.zeros((L, 4)) if t == 0 else prev_bd
        within("roi_in", a["roi_in"][t].cpu().numpy().astype(np.float64), o["roi_in"], np.maximum(prev, 1e-300))
        within("roi", a["roi"][t].cpu().numpy().astype(np.float64), o["roi"], bd["roi"])
        within("coord", a["coord"][t].cpu().numpy().astype(np.float64), o["coord"], bd["coord"])
        within("pose", a["pose"][t].cpu().numpy().astype(np.float64), o["pose"], bd["pose"])
        within("pts", a["pts"][t].cpu().numpy().astype(np.float64), o["pts"], bd["pts"])
        assert np.array_equal(lost[t], o["lost"].astype(np.uint8))
        prev_bd = np.where(o["lost"][:, None], prev, bd["roi"])
    assert np.array_equal(a["roi_in"][2, 1].cpu().numpy(), a["roi_in"][1, 1].cpu().numpy()), "the lost lane crops frame 2 around its last good box"
    within("final state", a["state"].cpu().numpy().astype(np.float64), ref[-1]["state"], prev_bd)
