"""The float64 restatement of the face-model fit (tests/facefit_ref.py) against the reference's own objective and point weights
(tests/golden/facefit.npz, written by tools/gen_golden_facefit.py from the notebook's class), its gradient against autograd, and the
project's optimiser against scipy's BFGS on the planted cases of the GPU tests (tests/facefit_cases.py)."""
import os

import numpy as np
import pytest
import torch

import facefit_cases as C
import facefit_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = np.load(os.path.join(GOLDEN, "facefit.npz"))


def test_objective_equals_the_references():
    """Both sides are float64 on the same widened float32 inputs and sum the same terms in different orders: facefit_ref.objective_bound."""
    m = C.model()
    worst = 0.0
    for i in range(len(G["f"])):
        x, y, w = (G[k][i].astype(np.float64) for k in ("x", "target", "weight"))
        f = R.objective(m, x, y, w)[0]
        bound = R.objective_bound(m, x, y, w)[0]
        worst = max(worst, abs(f - G["f"][i]) / bound)
        assert abs(f - G["f"][i]) <= bound, (i, f, G["f"][i], bound)
        assert abs(R.terms(m, x, y, w).sum() - f) <= bound
    print(f"objective against the golden: worst err / bound {worst:.4f}")
    res = np.stack([R.points(m, G["x"][i])[:, :2] - G["target"][i] for i in range(64)])
    assert (np.abs(res) < R.BETA).any() and (np.abs(res) > R.BETA).any()  # both zones of the huber term
    assert G["x"][:8, 6].min() < R.SIZE_SCALE < G["x"][:8, 6].max()        # a size on both sides of the constraint's scale


def test_point_weights_equal_the_references_exactly():
    h = np.degrees([R.heading(p) for p in G["wpose"]])
    assert h.min() < -89 and h.max() > 89 and (np.abs(h) < 2e-3).sum() >= 3 and (h[np.abs(h) < 2e-3] < 0).any() and (h[np.abs(h) < 2e-3] > 0).any()
    w2d = np.stack([R.point_weights(p, False) for p in G["wpose"]])
    w3d = np.stack([R.point_weights(p, True) for p in G["wpose"]])
    assert np.array_equal(w2d, G["w2d"]) and np.array_equal(w3d, G["w3d"])
    assert (w2d == 0).any() and (w2d[:, 8] != 0.1).all()  # the hidden side is switched off; point 8 is in both chin lists


def _torch_objective(m, x, y, w):
    """The objective in torch, written from the notebook's formulas (smooth_l1_loss, logsumexp), for autograd."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    q = x[:4] / torch.linalg.norm(x[:4])
    i, j, k, r = q
    Rm = torch.stack([torch.stack([1 - 2 * (j * j + k * k), 2 * (i * j - k * r), 2 * (i * k + j * r)]),
                      torch.stack([2 * (i * j + k * r), 1 - 2 * (i * i + k * k), 2 * (j * k - i * r)]),
                      torch.stack([2 * (i * k - j * r), 2 * (j * k + i * r), 1 - 2 * (i * i + j * j)])])
    local = t(m.kp) + (t(m.eig) * x[7:, None, None]).sum(0)
    P = local @ Rm.T * x[6]
    xy = P[:, :2] + x[4:6]
    errs = (t(w)[:, None] * torch.nn.functional.smooth_l1_loss(xy, t(y), beta=0.1, reduction="none")).mean()
    lp = torch.logsumexp(t(m.ck) - 0.5 * (((x[7:] - t(m.mu)) * t(m.sinv)) ** 2).sum(-1), 0)
    return errs + 1e-6 * torch.square(1.0 - torch.linalg.norm(x[:4])) + 0.01 * -(1.0 / 150.0) * lp + 10.0 * torch.exp(-x[6] / 0.05)


def gradient_cases():
    """16 points: golden rows of every block (residuals outside / inside beta, mixed, one face side at weight 0), and row 40 with one
    residual made exactly 0."""
    m = C.model()
    rows = [0, 5, 8, 9, 12, 16, 17, 20, 24, 25, 26, 27, 33, 40, 50, 63]
    out = []
    for i in rows:
        x, y, w = (G[k][i].astype(np.float64) for k in ("x", "target", "weight"))
        if i == 40:
            y = y.copy()
            y[10] = R.points(m, x)[10, :2]
        out.append((i, x, y, w))
    return out


def test_gradient_equals_autograd():
    m = C.model()
    worst = 0.0
    for i, x, y, w in gradient_cases():
        f, g = R.objective(m, x, y, w)
        xt = torch.from_numpy(x).requires_grad_(True)
        ft = _torch_objective(m, xt, y, w)
        (ga,) = torch.autograd.grad(ft, xt)
        bf, bg = R.objective_bound(m, x, y, w)
        assert abs(float(ft) - f) <= bf, (i, float(ft), f)
        err = np.abs(ga.numpy() - g)
        worst = max(worst, float((err / bg).max()))
        assert np.all(err <= bg), (i, err.max(), int(np.argmax(err / bg)))
        g7 = R.objective(m, x, y, w, 7)[1]
        assert np.array_equal(g7[:7], g[:7]) and not g7[7:].any()
    print(f"gradient against autograd: worst err / bound {worst:.4f}")
    i, x, y, w = gradient_cases()[13]
    assert abs((R.points(m, x)[10, :2] - y[10])).max() == 0.0
    assert G["weight"][24][R.FACE_LEFT].max() == 0 and G["weight"][26][R.FACE_RIGHT].max() == 0


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("B", C.BATCHES)
def test_optimiser_converges_on_the_planted_cases(B, mode):
    """The condition that makes the GPU tests' "every status is 0" fair: the restated optimiser converges on every planted case, lowers the
    objective, and ends no further above scipy's BFGS than FIT_OBJ_MARGIN (by construction) - which is printed for profiles/facefit.txt."""
    x0, y, w, ours, sc = C.planted(B, mode)
    m = C.model()
    for b, (o, s) in enumerate(zip(ours, sc)):
        assert o["status"] == 0, (b, o["status"], o["iterations"])
        assert o["f"] < o["f_start"]
        g = R.objective(m, o["x"], y[b], w[b])[1]
        assert np.abs(g).max() <= R.GTOL[1]
        assert o["f"] <= s["f"] + C.fit_obj_margin()
    its = np.array([o["iterations"] for o in ours])
    evs = np.array([o["evaluations"] for o in ours])
    print(f"B={B} fit_3d_projections={mode}: iterations {its.min(0)}..{its.max(0)}, evaluations {evs.min(0)}..{evs.max(0)}; "
          f"FIT_OBJ_MARGIN {C.fit_obj_margin():.3e}")
    assert 0.0 <= C.fit_obj_margin() < 1e-2  # objective values are of order 1e-2: a larger gap would mean one optimiser is broken


def test_optimiser_statuses():
    m = C.model()
    x0, y, w, ours, _ = C.planted(3, False)
    r = R.fit(m, x0[0], y[0], w[0], iters=(2, 2))
    assert r["status"] == 1 and r["iterations"] == (2, 2) and r["f"] < r["f_start"]
    r = R.fit(m, x0[0], y[0], w[0], iters=(0, 0))
    assert r["status"] == 1 and np.array_equal(r["x"], x0[0].astype(np.float64)) and r["f"] == r["f_start"]
    r = R.fit(m, ours[0]["x"], y[0], w[0], iters=(0, 0))
    assert r["status"] == 0  # started at a converged point
    bad = y[0].copy()
    bad[3, 1] = np.nan
    assert R.fit(m, x0[0], bad, w[0])["status"] == 3
    xs = x0[0].copy()
    xs[6] = -100.0
    r = R.fit(m, xs, y[0], w[0])
    assert r["status"] == 3 and np.isinf(r["f_start"])
    # a line search that cannot succeed: an objective that is not finite anywhere but at the start
    fun = lambda x: (0.0, np.ones(7)) if not x[:7].any() else (np.inf, np.ones(7))
    _, _, status, it, evals = R.bfgs_stage(fun, np.zeros(57), 7, 50, 1e-5)
    assert (status, it, evals) == (2, 0, 32)
