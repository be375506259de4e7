"""The float64 reference of the BatchNorm finalisation tests (tests/bn_ref.py) on its own, without a GPU: the bound formulas do bound,
the fold construction is what it says, and the allowances cover a correct float32 implementation - so that a failure of
tests/test_bn_finalize_gpu.py indicts the kernel and not the construction."""
import numpy as np
import pytest
import torch

import bn_ref as R


@pytest.mark.parametrize("name", R.FAMILIES + ("mixed",))
def test_forward_formula_bounds_the_true_maximum(name):
    """|max(scale*(y-mean)+beta, 0)| <= |scale| sqrt(count var) + |beta| per channel (Cauchy-Schwarz), every family, in float64."""
    n, C = 4096, 72
    rng = np.random.default_rng(5)
    y, gamma, beta = R.mixed(n, C, rng) if name == "mixed" else R.family(name, n, C, rng)
    formula, scale, mean = R.act_formula(y, gamma, beta)
    a = np.maximum(scale * (y.astype(np.float64) - mean) + beta.astype(np.float64), 0.0).max(0)
    # float64 rounding of mean and var over n terms: n * 2^-53 relative is ample
    assert (a <= formula * (1 + n * 2.0 ** -53)).all(), (name, float((a / np.maximum(formula, 1e-300)).max()))
    if name == "all_negative":
        assert a.max() == 0.0
    if name == "spike":  # the adversarial case: the formula is tight to 1/(2n) + |beta| here
        assert (a >= 0.99 * formula)[gamma * y.sum(0) > 0].all()
    # frozen form: statistics several sigma / a factor away
    mean_b, var_b = y.astype(np.float64).mean(0), y.astype(np.float64).var(0)
    mean_run = (mean_b + 3.0 * np.sqrt(var_b)).astype(np.float32)
    scale_run = (gamma / np.sqrt(4.0 * var_b + R.EPS)).astype(np.float32)
    ff = R.frozen_formula(y, scale_run, beta, mean_run)
    af = np.maximum(scale_run.astype(np.float64) * (y.astype(np.float64) - mean_run) + beta, 0.0).max(0)
    assert (af <= ff * (1 + n * 2.0 ** -53)).all(), name


def test_dy_formula_bounds_the_true_maximum():
    n, C = 4096, 40
    rng = np.random.default_rng(6)
    for spike_g, spike_y in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 0)):
        y, g = rng.standard_normal((n, C)), rng.standard_normal((n, C))
        px = rng.integers(0, n, C)
        if spike_g:
            g[:] = 0 if spike_g == 1 else -3.0  # (2: -a everywhere, +a at one pixel - |g - gmean| reaches 2 max|g|)
            g[px, np.arange(C)] = 3.0
        if spike_y:
            y[:] = 0
            y[px, np.arange(C)] = -2.0
        y, g = y.astype(np.float32), g.astype(np.float32)
        gamma = (rng.random(C) + 0.5).astype(np.float32)
        y64, g64 = y.astype(np.float64), g.astype(np.float64)
        mean, var = y64.mean(0), y64.var(0)
        rstd = 1 / np.sqrt(var + R.EPS)
        ga = gamma * rstd
        gb = -ga * rstd ** 2 * (g64 * (y64 - mean)).mean(0)
        true = np.abs(ga * (g64 - g64.mean(0)) + gb * (y64 - mean)).max(0)
        assert (true <= R.dy_formula(g, y, gamma, np.abs(g64).max()) * (1 + 1e-12)).all(), (spike_g, spike_y)


@pytest.mark.parametrize("rows", [1280, 1281, 2049, 5000])
def test_fold_reference_and_allowance(rows):
    """Folded (r, r + 1024, ...) and unfolded rows give the same float64 statistics; the float32 Kahan fold stays inside the allowance."""
    C = 40
    rng = np.random.default_rng(rows)
    y = (rng.normal(0, 3, C) + rng.standard_normal((rows * 2, C))).astype(np.float32)
    part = R.fwd_partial_rows(y, None, rows)
    folded, _ = R.fold64(part)
    assert folded.shape[0] == (rows if rows <= R.FOLD_ABOVE else R.FOLD_ROWS)
    p64 = part.astype(np.float64)
    d1, d2 = R.fold_allowance(part)
    # the same numbers added in another order, in float64: rows * 2^-53 of the magnitude - far inside the allowance of a real fold
    for j, d in ((0, d1), (1, d2)):
        diff = np.abs(folded[:, j].sum(0) - p64[:, j].sum(0))
        assert (diff <= rows * 2.0 ** -53 * np.abs(p64[:, j]).sum(0)).all()
        if rows > R.FOLD_ABOVE:
            assert (diff <= d).all()
            k32 = R.fold32_kahan(part).astype(np.float64)
            assert (np.abs(k32[:, j].sum(0) - p64[:, j].sum(0)) <= d).all()
            # a fold that drops its ragged last block is far outside it
            short = p64[:(rows // R.FOLD_ROWS) * R.FOLD_ROWS]
            assert (np.abs(short[:, j].sum(0) - p64[:, j].sum(0)) > d).any()
    # the variance is a stated fraction of E[y^2] (|mean| <= ~3 sigma by construction would give 1/10; N(0,3) means: check)
    gamma, beta = np.ones(C, np.float32), np.zeros(C, np.float32)
    ref = R.fwd_reference(part, None, rows * 2, gamma, beta, np.zeros(C, np.float32), np.ones(C, np.float32))
    y64 = y.astype(np.float64)
    want_var = y64.var(0)
    got_rstd, tol = ref["rstd"]
    # against the statistics of y itself: the rows were rounded to float32 once (U each), amplified by E[y^2]/var in the variance
    amp = (y64 ** 2).mean(0) / want_var
    assert (np.abs(got_rstd - 1 / np.sqrt(want_var + R.EPS)) <= (R.U * (1 + 2 * amp) + 1e-12) * got_rstd + tol).all()


def test_bwd_reference_matches_float64_autograd():
    n, C, rows = 2048, 24, 16
    rng = np.random.default_rng(7)
    y = (rng.normal(0, 1, C) + rng.standard_normal((n, C))).astype(np.float32)
    g = rng.standard_normal((n, C)).astype(np.float32)
    gamma = (rng.random(C) + 0.5).astype(np.float32)
    y64 = y.astype(np.float64)
    mean, rstd = y64.mean(0).astype(np.float32), (1 / np.sqrt(y64.var(0) + R.EPS)).astype(np.float32)
    ref = R.bwd_reference(R.bwd_partial_rows(g, y, mean, rows), n, gamma, rstd)
    yt = torch.from_numpy(y64).requires_grad_()
    gt, bt = torch.from_numpy(gamma.astype(np.float64)).requires_grad_(), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    out = torch.nn.functional.batch_norm(yt, None, None, gt, bt, True, 0.1, R.EPS)
    out.backward(torch.from_numpy(g.astype(np.float64)))
    # float32 rows, MEAN and RSTD against exact ones: 1e-6 relative to the sums' magnitude is generous for this CPU-only sanity check
    np.testing.assert_allclose(ref["dgamma"][0], gt.grad.numpy(), rtol=0, atol=1e-6 * np.abs(g).sum(0).max())
    np.testing.assert_allclose(ref["dbeta"][0], bt.grad.numpy(), rtol=0, atol=1e-6 * np.abs(g).sum(0).max())
    dy = ref["ga"][0] * (g - ref["gmean"][0]) + ref["gb"][0] * (y64 - mean)
    np.testing.assert_allclose(dy, yt.grad.numpy(), rtol=0, atol=1e-5)
