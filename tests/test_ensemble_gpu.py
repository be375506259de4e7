"""ttk_ensemble_reduce (csrc/ensemble.hip) through the C-ABI on guarded buffers, against tests/ensemble_ref.py in float64 on the same float32
inputs.  The cases, the launches and the derivation of every tolerance are in tests/ensemble_cases.py."""
import numpy as np
import pytest
import torch

import ensemble_ref as ER
from ensemble_cases import SEED_FAR, _f32, bounds, check, make_case, outputs, run, within
from head_loss_cases import Guarded
from util import gpu_section

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("E", [1, 2, 3, 16])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_reduce_matches_float64(B, E):
    """Random member signs, S = 50, rotation + scale + shift per row, the last row mirrored (flip map)."""
    inp = make_case(B, E, seed=1000 + 17 * B + E)
    got, r = check(inp, f"B={B} E={E}")
    assert np.linalg.det(inp["back"][B - 1, :, :2].astype(np.float64)) < 0
    assert np.all(got["pose"][np.arange(B), r["pivot"]] > 0)  # the pivot rule leaves the largest component positive


def test_antipodal_pair_gives_q_not_zero():
    inp = make_case(3, 2, seed=5, sigma=1e-9)
    inp["pose"][1] = -inp["pose"][0]
    got, r = check(inp, "antipodal pair")
    assert np.all(got["stats"][:, 1] > 0.999) and np.all(got["stats"][:, 0] < 1e-3)
    q = ER.back_transform(inp["back"], inp["pose"][:1], inp["coord"][:1])[0][0]
    assert np.all(np.abs(np.abs((got["pose"] * q).sum(-1)) - 1) < 1e-5)


@pytest.mark.parametrize("pts,shape", [(False, False), (True, False), (False, True)])
def test_null_landmark_and_shape_pointers(pts, shape):
    check(make_case(3, 3, seed=11, pts=pts, shape=shape), f"NULL pointers: pts={pts} shape={shape}")


def test_shape_width_limits():
    check(make_case(3, 2, seed=12, S=1), "S=1")
    check(make_case(3, 2, seed=13, S=64), "S=64")


def test_exact_pivot_tie_up_to_sign():
    """|components| all 0.5 and an identity transform: the four sums of |q| tie exactly and both sides take component 0; compared up to the
    global sign of the quaternion all the same."""
    inp = make_case(3, 3, seed=21, mirrored=())
    inp["back"][:] = _f32([[1, 0, 0], [0, 1, 0]])
    inp["pose"][:] = 0.5
    inp["pose"][1, :, 2:] = -0.5
    inp["pose"][2, :, 1] = -0.5
    inp["pose"][2] *= -1.0
    check(inp, "pivot tie", up_to_sign=True)


def test_members_far_apart_report_a_small_norm():
    inp = make_case(3, 16, seed=SEED_FAR, sigma=None)  # uniformly random rotations: E[|component|] = 0.42 is about all the mean keeps
    got, r = check(inp, "members far apart")
    assert r["stats"][:, 1].min() < 0.5 and got["stats"][:, 1].min() < 0.5
    assert all(np.isfinite(v).all() for v in got.values() if v is not None)


def test_zero_mean_stays_finite():
    """All members zero (exactly representable): |mean| = 0 is reported, the division by max(|mean|, FLT_MIN) gives zeros, and nothing else
    in the row is touched by it."""
    inp = make_case(3, 2, seed=41, mirrored=())
    inp["back"][:] = _f32([[2, 0, 8], [0, 2, 16]])
    inp["pose"][:, 1] = 0.0
    with gpu_section():
        out = run(inp)
    out.check("zero mean")
    got = outputs(out, inp)
    assert all(np.isfinite(v).all() for v in got.values())
    assert np.all(got["pose"][1] == 0) and got["stats"][1, 1] == 0 and got["stats"][1, 0] == 0
    r = ER.ensemble_reduce(inp["pose"], inp["coord"], inp["pts"], inp["shape"], inp["back"])
    bd = bounds(inp, r)
    within("coord", got["coord"], r["coord"], bd["coord"])
    within("pts", got["pts"], r["pts"], bd["pts"])
    within("shape", got["shape"], r["shape"], bd["shape"])
    within("pose of the other rows", got["pose"][[0, 2]], r["pose"][[0, 2]], bd["pose"][[0, 2]])


@pytest.mark.parametrize("E", [0, 17])
def test_member_count_out_of_range_is_refused(E):
    from trackertraincode._hip import lib, ptr

    inp = make_case(3, 16, seed=51)
    dev = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    out = Guarded()
    args = (ptr(dev["pose"]), ptr(dev["coord"]), ptr(dev["pts"]), ptr(dev["shape"]), ptr(dev["back"]), E, 3, 50,
            out("pose", 12), out("coord", 9), out("pts", 612), out("shape", 150), out("stats", 15))
    with gpu_section():
        with pytest.raises(RuntimeError, match="members"):
            lib().call("ttk_ensemble_reduce", *args)
        torch.cuda.synchronize()
    for name, (full, _) in out.bufs.items():
        assert bool(full.isnan().all()), f"{name} was written by a refused call"


def test_mismatched_optional_pointers_are_refused():
    from trackertraincode._hip import lib, ptr

    inp = make_case(3, 2, seed=52)
    dev = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    out = Guarded()
    with gpu_section():
        with pytest.raises(RuntimeError, match="together"):
            lib().call("ttk_ensemble_reduce", ptr(dev["pose"]), ptr(dev["coord"]), ptr(dev["pts"]), ptr(dev["shape"]), ptr(dev["back"]), 2, 3, 50,
                       out("pose", 12), out("coord", 9), None, out("shape", 150), out("stats", 15))
        with pytest.raises(RuntimeError, match="shape parameters"):
            lib().call("ttk_ensemble_reduce", ptr(dev["pose"]), ptr(dev["coord"]), ptr(dev["pts"]), ptr(dev["shape"]), ptr(dev["back"]), 2, 3, 65,
                       out("pose", 12), out("coord", 9), out("pts", 612), out("shape", 150), out("stats", 15))
        torch.cuda.synchronize()
    for name, (full, _) in out.bufs.items():
        assert bool(full.isnan().all()), f"{name} was written by a refused call"


def test_two_calls_are_bitwise_equal():
    inp = make_case(65, 16, seed=61)
    with gpu_section():
        a, b = run(inp), run(inp)
    for name in a.bufs:
        assert torch.equal(a.get(name), b.get(name)), name
