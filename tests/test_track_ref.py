"""tests/track_ref.py - the float64 yardstick of the closed-loop tracker's kernels - held to pinned code: its back-transformation to
`Predictor.to_image_coordinates` on CPU tensors (itself pinned to the reference by tests/golden/eval.npz), its clamp to the reference's
four-line rule, and `eval.blink_stability` to a direct numpy statement of scripts/evaluate_stability.py:229-245."""
import numpy as np
import pytest
import torch

import track_ref as TR
from track_cases import update_case


@pytest.mark.parametrize("L,pts", [(1, True), (3, True), (16, True), (3, False)])
def test_back_transformation_equals_to_image_coordinates(L, pts):
    """Axis-aligned, rotated (lane 1) and mirrored (lane 2) transforms: float64 track_ref against the float32 torch path, to float32 rounding
    (1e-5 relative to the magnitude of the coordinates, a few hundred units in the last place of float32 at most)."""
    from trackertraincode.eval import Predictor

    case = update_case(L, seed=100 + L, pts=pts)
    r = TR.update(case["roi"], case["coord"], case["pose"], case["pts"], case["tr"], case["N"], case["Ws"], case["Hs"], case["lane_factor"],
                  case["roi_state"])
    preds = {k: torch.from_numpy(case[k]) for k in ("roi", "coord", "pose")}
    if pts:
        preds["pt3d_68"] = torch.from_numpy(case["pts"])
    got = Predictor.to_image_coordinates(preds, torch.from_numpy(case["tr"]), case["N"])
    if L >= 3:
        assert np.linalg.det(case["tr"][2, :, :2].astype(np.float64)) < 0 and abs(case["tr"][1, 0, 1]) > 0.1
    for k, name in (("roi", "roi"), ("coord", "coord"), ("pose", "pose"), ("pts", "pt3d_68")):
        if r[k] is None:
            assert name not in got
            continue
        want, have = r[k], got[name].numpy().astype(np.float64)
        np.testing.assert_allclose(have, want, rtol=0, atol=1e-5 * max(1.0, np.abs(want).max()), err_msg=k)


def test_clamp_is_the_reference_rule():
    rng = np.random.default_rng(3)
    roi = rng.uniform(-60, 220, (200, 4))
    w, h = 128, 96
    got = TR.clamp(roi, w, h)
    for (x0, y0, x1, y1), g in zip(roi, got):
        assert list(g) == [max(0.0, x0), max(0.0, y0), min(x1, w), min(y1, h)]  # scripts/evaluate_stability.py:259


def test_validity_rule_and_the_host_check_agree():
    from trackertraincode.eval import track_box_is_valid

    rows = {"good": ([10, 10, 50, 40], True), "inverted": ([50, 10, 10, 40], False), "nan": ([np.nan, 10, 50, 40], False),
            "inf": ([10, 10, np.inf, 40], False), "outside": ([140, 10, 180, 40], False), "half a pixel": ([10, 10, 10.5, 10.5], False),
            "two pixels at 1.0": ([10, 10, 12, 11], True), "1.8 pixels at 1.2": ([10, 10, 11.8, 11], True)}
    for name, (roi, want) in rows.items():
        f = 1.2 if "1.2" in name else 1.0
        roi = np.asarray([roi], np.float64)
        with np.errstate(invalid="ignore"):
            assert bool(TR.valid(roi, TR.clamp(roi, 128, 96), np.array([f]))[0]) == want, name
        assert track_box_is_valid(roi[0], f, 128, 96) == want, name


def test_state_and_counter_flow():
    """A lane that is lost keeps its box and crops the next frame with it; a valid one moves on; the counter counts frames."""
    N, Ws, Hs = 129, 128, 96
    first, factor = np.array([[40.0, 30.0, 80.0, 70.0]]), np.array([1.0], np.float32)
    ok = (np.array([[-0.5, -0.5, 0.5, 0.5]], np.float32), np.zeros((1, 3), np.float32), np.array([[0, 0, 0, 1]], np.float32), None)
    bad = (np.array([[0.5, -0.5, -0.5, 0.5]], np.float32),) + ok[1:]
    out, t = TR.track(first, factor, [ok, bad, ok], N, Ws, Hs)
    assert t == 3 and [bool(o["lost"][0]) for o in out] == [False, True, False]
    assert np.allclose(out[0]["state"], [[50, 40, 70, 60]])  # the middle half of the 40-pixel view box
    assert np.array_equal(out[1]["state"], out[0]["state"]) and np.array_equal(out[2]["roi_in"], out[0]["state"])
    assert np.array_equal(out[1]["view"], out[2]["view"]) and not np.array_equal(out[0]["view"], out[1]["view"])


def test_blink_stability_equals_the_reference_statement():
    from trackertraincode.eval import blink_stability

    rng = np.random.default_rng(5)
    blinks = [(8, 12), (22, 30)]
    for shape in ((40,), (40, 3), (40, 2)):
        v = rng.standard_normal(shape).cumsum(0)
        assert np.array_equal(blink_stability(v, blinks), TR.blink_stability_direct(v, blinks))
    for bad in ([(2, 12)], [(8, 36)], [(8, 12), (30, 35)]):
        with pytest.raises(ValueError, match="within 5 frames"):
            blink_stability(rng.standard_normal(40), bad)
