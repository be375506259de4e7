"""tests/localizer_ref.py - the float64 yardstick of the localizer's GPU tests - held to the reference's own LocalizerNet
(tests/golden/localizer.npz, tools/gen_golden_localizer.py), and its letterbox and re-acquisition rule to their identities."""
import json
import os

import numpy as np
import pytest
import torch

import localizer_ref as R
from util import GOLDEN


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLDEN, "localizer.npz"))
    meta = json.loads(str(d["meta"]))
    return d, meta, {k: d["sd/" + k] for k in meta["keys"]}


def test_restatement_reproduces_the_reference(gold):
    d, meta, sd = gold
    x = (torch.from_numpy(d["frames"]).double() * meta["mul"] + meta["add"])[:, None]
    # (the fixture whitens in float32: 1 / 256 and -0.5 are exact, so the float64 product is the same value)
    out, att, taps = R.forward(sd, x)
    assert np.abs(out.numpy() - d["out64"]).max() < 1e-10
    assert np.abs(att.numpy() - d["attention64"]).max() < 1e-10
    for i in R.TAPS:
        t = taps[i][0].numpy()
        if i in (1, 2):
            t = t[np.ix_(np.arange(t.shape[0]), R.sample_grid(t.shape[1]), R.sample_grid(t.shape[2]))]
        assert t.shape == d[f"tap{i}"].shape
        assert np.abs(t - d[f"tap{i}"]).max() < 1e-10, i


def test_packed_parameter_count(gold):
    _, _, sd = gold
    n = 232 + sum(ci * e * ci + 2 * ci * e + ci * e * k * k + co * ci * e + co for ci, co, k, s, e in R.BLOCKS) + 2 * 56 + 2 + 2
    assert R.packed_parameters(sd).numel() == n


def test_letterbox_constant_frame():
    x, (s, ox, oy) = R.letterbox(np.full((100, 300), 77.0))
    assert ox == 0 and s == 288 / 300 and oy == pytest.approx((224 - 96) / 2)
    ys = np.arange(224)
    inside = (ys >= oy) & (ys + 1 <= oy + 100 * s)
    outside = (ys + 1 <= oy) | (ys >= oy + 100 * s)
    assert inside.sum() == 96 and outside.sum() == 128
    assert np.abs(x[inside] - 77.0).max() < 1e-11 and np.all(x[outside] == 0)


def test_letterbox_integer_ratio_is_the_block_mean():
    rng = np.random.default_rng(0)
    f = rng.integers(0, 256, (448, 576)).astype(np.float64)
    x, lb = R.letterbox(f)
    assert lb == (0.5, 0.0, 0.0)
    assert np.abs(x - f.reshape(224, 2, 288, 2).mean(axis=(1, 3))).max() < 1e-11


def test_letterbox_frames_that_fill_the_input():
    """A frame of the input's own 9:7 shape fills it (ox = oy = 0); a 4:3 frame fills its width, and the bars above and below are 0."""
    rng = np.random.default_rng(1)
    x, lb = R.letterbox(rng.integers(1, 256, (112, 144)).astype(np.float64))
    assert lb == (2.0, 0.0, 0.0) and x.min() >= 1
    x, (s, ox, oy) = R.letterbox(rng.integers(1, 256, (480, 640)).astype(np.float64))
    assert (s, ox, oy) == (0.45, 0.0, 4.0)
    assert np.all(x[:4] == 0) and np.all(x[220:] == 0) and x[4:220].min() >= 1


def test_letterbox_upscaling_keeps_the_mean():
    rng = np.random.default_rng(2)
    f = rng.integers(0, 256, (37, 41)).astype(np.float64)
    x, (s, ox, oy) = R.letterbox(f)
    assert x.sum() == pytest.approx(f.sum() * s * s, rel=1e-12)  # area-preserving


def test_box_map():
    lb = np.array([0.45, 0.0, 4.0], dtype=np.float32)
    r = R.box_to_frame(np.array([-1.0, -1.0, 1.0, 1.0]), lb)
    np.testing.assert_allclose(r, [0, -4 / 0.45, 640, 220 / 0.45], rtol=1e-6)


def _rule(lost_row, run, logit, box, after=3, thr=0.5, factor=1.0):
    loc = np.array([[logit, *box]], dtype=np.float32)
    lb = np.array([[1.0, 0.0, 0.0]], dtype=np.float32)  # a 224 x 288 frame: frame pixels are input pixels
    state = np.array([[10, 10, 50, 50]], dtype=np.float32)
    return R.reacquire_rule(loc, lb, [lost_row], [0], [factor], state, [run], 224, 288, after, thr)


def test_reacquire_rule_on_scripted_inputs():
    good = (-0.5, -0.5, 0.5, 0.5)  # (72, 56, 216, 168)
    st, run, re, hf, roi = _rule(True, 1, 3.0, good)      # run 2 < 3
    assert run[0] == 2 and not re[0] and np.all(st == [[10, 10, 50, 50]])
    st, run, re, hf, roi = _rule(True, 2, 3.0, good)      # run 3: taken
    assert run[0] == 0 and re[0] and np.all(st == [[72, 56, 216, 168]]) and np.all(roi == st) and hf[0] == pytest.approx(0.95257413)
    st, run, re, _, _ = _rule(True, 7, 3.0, good)
    assert run[0] == 0 and re[0]
    st, run, re, _, _ = _rule(False, 7, 3.0, good)        # not lost: the run ends, nothing taken
    assert run[0] == 0 and not re[0] and np.all(st == [[10, 10, 50, 50]])
    for logit in (-0.1, float("nan")):                     # below the threshold, NaN
        st, run, re, _, _ = _rule(True, 2, logit, good)
        assert run[0] == 3 and not re[0] and np.all(st == [[10, 10, 50, 50]])
    for box in ((0.5, -0.5, -0.5, 0.5), (float("nan"), -0.5, 0.5, 0.5), (float("inf"), -0.5, 0.5, 0.5), (1.5, -0.5, 2.5, 0.5),
                (0.0, 0.0, 0.005, 0.005)):                 # inverted, non-finite, outside the image, too small
        st, run, re, _, _ = _rule(True, 5, 3.0, box)
        assert run[0] == 6 and not re[0] and np.all(st == [[10, 10, 50, 50]]), box
    # a box that leaves the image is clamped
    st, run, re, _, _ = _rule(True, 5, 3.0, (-1.5, -0.5, 0.5, 1.5))
    assert re[0] and np.all(st == [[0, 56, 216, 224]])
    # 0.72 x 0.56 pixels: too small at factor 1, large enough at factor 3
    tiny = (0.0, 0.0, 0.005, 0.005)
    assert _rule(True, 5, 3.0, tiny, factor=3.0)[2][0] and not _rule(True, 5, 3.0, tiny, factor=2.5)[2][0]
