"""The BatchNorm finalisation kernels of csrc/bn.hip against float64, and the operand bounds they leave in row TTK_BN_AUX.

Every GEMM on the fp16 matrix pipe scales its operands by a power of two taken from TTK_AUX_ACT_BOUND / TTK_AUX_DY_BOUND; the contract
(include/ttk.h) is one-sided - bound >= the true maximum of the tensor the consumer forms - and a bound far too large loses small
operands.  The consumers are tested under bounds the tests supply; here the PRODUCERS of the bounds are: ttk_bn_fwd_finalize,
ttk_bn_frozen_bound, ttk_bn_bwd_finalize, ttk_bn_bwd_frozen (and ttk_bn_eval_prepare, whose rows they read).

The entry points take the partial rows as an argument, so no producer kernel is needed: the tests build y[n, C] and g[n, C], sum them
per pixel block in float64, round the rows to float32 and pass them in; the reference (tests/bn_ref.py, pinned by tests/test_bn_ref.py)
is float64 arithmetic on exactly those float32 rows and on the float32 y and g.  Every tolerance is derived where it is formed - from
float32 rounding, never from what the kernels returned."""
import copy

import numpy as np
import pytest
import torch

import bn_ref as R
from bn_ref import AUX_ACT_BOUND, AUX_DY_BOUND, AUX_GMAX, BN_AUX, BN_BETA, BN_GA, BN_GB, BN_GMEAN, BN_MEAN, BN_RSTD, BN_SCALE, U

pytestmark = pytest.mark.gpu

CS = (8, 40, 64, 1000, 2048)                         # 8, 40, 1000: not multiples of the 32-channel workgroup
ROWS = (1, 31, 33, 1024, 1280, 1281, 2049, 5000)     # both sides of the 32 row lanes and of the fold threshold; ragged last fold block


def _lib():
    import trackertraincode._hip as H
    return H.lib(), H.ptr


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _sentinel_bn(C, rng, zero_slots=()):
    """A constant block full of recognisable junk (so that an untouched row can be told from a rewritten one); the AUX slots in
    `zero_slots` start at zero as the contract of the atomicMax asks."""
    bn = rng.normal(0, 1, (8, C)).astype(np.float32) + 10.0
    for s in zero_slots:
        bn[BN_AUX, s] = 0.0
    return bn


def _pixels_per_row(rows):
    return max(1, 2048 // rows)


def _assert_close(name, got, want_tol, ctx):
    want, tol = want_tol
    got = got.detach().double().cpu().numpy()
    err = np.abs(got - want)
    bad = err > tol
    assert not bad.any(), (ctx, name, int(bad.sum()), "worst err/tol", float((err / np.maximum(tol, 1e-300)).max()),
                           "at channel", int(np.argmax(err / np.maximum(tol, 1e-300))))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. rows and running statistics of ttk_bn_fwd_finalize
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("C", CS)
def test_fwd_finalize_rows_and_statistics(C, rows):
    """SCALE, BETA, MEAN, RSTD, running_mean, running_var against float64 on the same float32 rows (allowances: bn_ref.fwd_reference -
    2 U |want| for results that are the float32 cast of a double computation, plus above 1280 rows the float32 Kahan fold's
    2^-23 of the folded magnitude per element, propagated through the formulas); num_batches_tracked + 1 exactly; rows GA, GB, GMEAN and
    the other AUX slots bitwise untouched.

    Inputs: y = mu + s z with |mu| <= 3 s, so without a pivot var >= E[y^2] / 10 (asserted at 1/12 for the sample), with a pivot at
    mu + 0.3 s N(0,1) better still: the cancellation amplification of the variance is a known constant <= 12."""
    L, p = _lib()
    rng = np.random.default_rng(1000 * C + rows)
    n = rows * _pixels_per_row(rows)
    s = rng.random(C) + 0.5
    mu = rng.uniform(-3, 3, C) * s
    y = (mu + s * rng.standard_normal((n, C))).astype(np.float32)
    gamma, beta = (rng.random(C) + 0.5).astype(np.float32), rng.normal(0, 0.2, C).astype(np.float32)
    gamma[::3] *= -1
    rm0 = (mu + 0.3 * s * rng.standard_normal(C)).astype(np.float32)
    rv0 = (rng.random(C) + 0.5).astype(np.float32)
    sep = (mu + 0.3 * s * rng.standard_normal(C)).astype(np.float32)
    # (pivot, running statistics given, num_batches_tracked given, count)
    combos = [("none", True, True, n), ("separate", False, False, n), ("alias", True, False, n), ("separate", True, True, 1)]
    for pivot_mode, running, counter, count in combos:
        ctx = (C, rows, pivot_mode, running, counter, count)
        pivot = {"none": None, "separate": sep, "alias": rm0}[pivot_mode]
        if count == 1:  # ONE pixel; its sums sit in the LAST row (the others are zero): unbiased factor 1, variance 0 up to the rows' rounding
            part = np.zeros((rows, 2, C), np.float32)
            part[-1] = R.fwd_partial_rows(y[:1], pivot, 1)[0]
        else:
            part = R.fwd_partial_rows(y, pivot, rows)
            _, var, _, e2 = R.fwd_stats(part, pivot, count)
            assert (var >= e2 / 12).all(), ctx  # the stated fraction
        ref = R.fwd_reference(part, pivot, count, gamma, beta, rm0 if running else None, rv0 if running else None)
        bn0 = _sentinel_bn(C, rng, (AUX_ACT_BOUND,))
        d_part, d_bn, d_gamma, d_beta = _t(part), _t(bn0), _t(gamma), _t(beta)
        d_rm, d_rv = (_t(rm0), _t(rv0)) if running else (None, None)
        d_pivot = {"none": None, "separate": _t(sep), "alias": d_rm}[pivot_mode]
        nbt = torch.full((), 7, dtype=torch.int64, device="cuda") if counter else None
        L.call("ttk_bn_fwd_finalize", p(d_part), p(d_pivot), rows, C, count, p(d_gamma), p(d_beta), p(d_rm), p(d_rv), p(nbt), R.MOMENTUM, R.EPS,
               p(d_bn))
        torch.cuda.synchronize()
        for name, row in (("scale", BN_SCALE), ("beta", BN_BETA), ("mean", BN_MEAN), ("rstd", BN_RSTD)):
            _assert_close(name, d_bn[row], ref[name], ctx)
        if running:
            _assert_close("running_mean", d_rm, ref["running_mean"], ctx)
            _assert_close("running_var", d_rv, ref["running_var"], ctx)
        if counter:
            assert int(nbt) == 8, ctx
        got, was = _bits(d_bn), _bits(torch.from_numpy(bn0))
        assert torch.equal(got[BN_GA:BN_AUX], was[BN_GA:BN_AUX]), ("rows GA, GB, GMEAN were touched", ctx)
        assert torch.equal(got[BN_AUX, 1:], was[BN_AUX, 1:]), ("AUX slots other than ACT_BOUND were touched", ctx)
        bound = float(d_bn[BN_AUX, AUX_ACT_BOUND])
        assert np.isfinite(bound) and bound > 0, ctx


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the forward bound contract
# ------------------------------------------------------------------------------------------------------------------------------
_N, _C, _ROWS = 4096, 72, 8  # 72 channels: three workgroups, the last one ragged; 8 rows of 512 pixels (see bn_ref.family on "tiny")


def _family(name, rng):
    return R.mixed(_N, _C, rng) if name == "mixed" else R.family(name, _N, _C, rng)


@pytest.mark.parametrize("with_pivot", [False, True])
@pytest.mark.parametrize("name", R.FAMILIES + ("mixed",))
def test_fwd_finalize_bound_contract(name, with_pivot):
    """true_max <= ACT_BOUND <= 2 * formula64.  The lower side is the contract of include/ttk.h, with the true maximum formed in
    float64 from the stored y and the rows the kernel itself wrote (what the consumer will use); the upper side allows one
    power-of-two step of the consumer's scale over the documented |scale| sqrt(count var) + |beta| in float64 - a cap from how the
    bound is used, not a measurement."""
    L, p = _lib()
    rng = np.random.default_rng(11)
    y, gamma, beta = _family(name, rng)
    y64 = y.astype(np.float64)
    sig = y64.std(0)
    pivot = (y64.mean(0) + 0.3 * sig * rng.standard_normal(_C)).astype(np.float32) if with_pivot else None  # a running mean of such batches
    part = R.fwd_partial_rows(y, pivot, _ROWS)
    d_bn = torch.zeros(8, _C, device="cuda")
    d_part, d_pivot, d_gamma, d_beta = _t(part), (_t(pivot) if with_pivot else None), _t(gamma), _t(beta)  # (named: they must outlive the call)
    L.call("ttk_bn_fwd_finalize", p(d_part), p(d_pivot), _ROWS, _C, _N, p(d_gamma), p(d_beta), None, None, None, R.MOMENTUM, R.EPS, p(d_bn))
    torch.cuda.synchronize()
    bn = d_bn.cpu().numpy()
    assert np.isfinite(bn).all()
    true_max = R.act_true_max(y, bn[BN_SCALE], bn[BN_BETA], bn[BN_MEAN])
    formula = float(R.act_formula(y, gamma, beta)[0].max())
    bound = float(bn[BN_AUX, AUX_ACT_BOUND])
    print(f"fwd bound {name} pivot={with_pivot}: true_max {true_max:.6g}  bound {bound:.6g}  formula64 {formula:.6g}")
    assert true_max <= bound, (name, with_pivot, true_max, bound)
    assert bound <= 2.0 * formula, (name, with_pivot, bound, formula)
    if name == "all_negative":
        assert true_max == 0.0


@pytest.mark.parametrize("with_pivot", [False, True])
@pytest.mark.parametrize("name", R.FAMILIES + ("mixed",))
def test_frozen_bound_contract(name, with_pivot):
    """ttk_bn_eval_prepare + ttk_bn_frozen_bound with running statistics 3 sigma (at least 5 % of |mean|) from the batch mean and a
    factor 4 or 1/4 from the batch variance: true_max <= ACT_BOUND <= 2 * formula64 with the frozen form
    |scale| (sqrt(count var_b) + |mean_b - mean_run|) + |beta|; nothing else of bn is written."""
    L, p = _lib()
    rng = np.random.default_rng(12)
    y, gamma, beta = _family(name, rng)
    y64 = y.astype(np.float64)
    mean_b, var_b = y64.mean(0), y64.var(0)
    rm = (mean_b + rng.choice([-3.0, 3.0], _C) * np.maximum(np.sqrt(var_b), 0.05 * np.abs(mean_b))).astype(np.float32)
    rv = (var_b * rng.choice([0.25, 4.0], _C)).astype(np.float32)
    d_bn = _t(_sentinel_bn(_C, rng, (AUX_ACT_BOUND,)))
    d_gamma, d_beta, d_rm, d_rv = _t(gamma), _t(beta), _t(rm), _t(rv)  # (named: they must outlive the call)
    L.call("ttk_bn_eval_prepare", p(d_gamma), p(d_beta), p(d_rm), p(d_rv), R.EPS, _C, p(d_bn))
    torch.cuda.synchronize()
    before = _bits(d_bn)
    pivot = rm if with_pivot else None  # (the host passes the running mean)
    part = R.fwd_partial_rows(y, pivot, _ROWS)
    d_part = _t(part)
    L.call("ttk_bn_frozen_bound", p(d_part), p(d_rm) if with_pivot else None, _ROWS, _C, _N, p(d_bn))
    torch.cuda.synchronize()
    after = _bits(d_bn)
    keep = torch.ones(8, _C, dtype=torch.bool)
    keep[BN_AUX, AUX_ACT_BOUND] = False
    assert torch.equal(before[keep], after[keep]), "ttk_bn_frozen_bound wrote something besides ACT_BOUND"
    bn = d_bn.cpu().numpy()
    true_max = R.act_true_max(y, bn[BN_SCALE], bn[BN_BETA], bn[BN_MEAN])
    formula = float(R.frozen_formula(y, bn[BN_SCALE], bn[BN_BETA], bn[BN_MEAN]).max())
    bound = float(bn[BN_AUX, AUX_ACT_BOUND])
    print(f"frozen bound {name} pivot={with_pivot}: true_max {true_max:.6g}  bound {bound:.6g}  formula64 {formula:.6g}")
    assert np.isfinite(bound)
    assert true_max <= bound, (name, with_pivot, true_max, bound)
    assert bound <= 2.0 * formula, (name, with_pivot, bound, formula)


@pytest.mark.parametrize("entry", ["ttk_bn_fwd_finalize", "ttk_bn_frozen_bound"])
def test_act_bound_is_raised_never_lowered(entry):
    """The slot is raised with atomicMax: a larger preset stays bitwise, a smaller one ends at the value a zeroed slot ends at."""
    L, p = _lib()
    rng = np.random.default_rng(13)
    y, gamma, beta = _family("gaussian", rng)
    part = R.fwd_partial_rows(y, None, _ROWS)
    d_gamma, d_beta = _t(gamma), _t(beta)
    proto = np.zeros((8, _C), np.float32)
    proto[BN_SCALE], proto[BN_BETA], proto[BN_MEAN], proto[BN_RSTD] = gamma, beta, 0.25, 1.0

    def run(preset):
        d_bn = _t(proto)
        d_bn[BN_AUX, AUX_ACT_BOUND] = preset
        d_part = _t(part)  # (the entry points may fold it in place: a fresh copy per call)
        if entry == "ttk_bn_fwd_finalize":
            L.call(entry, p(d_part), None, _ROWS, _C, _N, p(d_gamma), p(d_beta), None, None, None, R.MOMENTUM, R.EPS, p(d_bn))
        else:
            L.call(entry, p(d_part), None, _ROWS, _C, _N, p(d_bn))
        torch.cuda.synchronize()
        return d_bn[BN_AUX, AUX_ACT_BOUND].cpu()

    fresh = run(0.0)
    assert float(fresh) > 0
    big = torch.tensor(float(fresh) * 3.0)
    assert torch.equal(_bits(run(float(big))), _bits(big))
    assert torch.equal(_bits(run(float(fresh) * 0.5)), _bits(fresh))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. ttk_bn_bwd_finalize
# ------------------------------------------------------------------------------------------------------------------------------
def _autograd_param_grads(y, g, gamma):
    yt = torch.from_numpy(y.astype(np.float64))
    gt = torch.from_numpy(gamma.astype(np.float64)).requires_grad_()
    bt = torch.zeros(y.shape[1], dtype=torch.float64, requires_grad=True)
    torch.nn.functional.batch_norm(yt, None, None, gt, bt, True, 0.1, R.EPS).backward(torch.from_numpy(g.astype(np.float64)))
    return gt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("C", CS)
def test_bwd_finalize_rows_and_parameter_gradients(C, rows):
    """GA, GB, GMEAN against their definitions on the float32 rows (bn_ref.bwd_reference); dgamma / dbeta against float64 autograd of
    F.batch_norm(training=True) on the same y and g - accumulate 0 and 1 onto non-zero contents, and NULL dgamma / dbeta."""
    L, p = _lib()
    rng = np.random.default_rng(2000 * C + rows)
    n = rows * _pixels_per_row(rows)
    y = (rng.normal(0, 1, C) + (rng.random(C) + 0.5) * rng.standard_normal((n, C))).astype(np.float32)
    g = (rng.normal(0, 0.3, C) + rng.standard_normal((n, C))).astype(np.float32)
    gamma = ((rng.random(C) + 0.5) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    y64 = y.astype(np.float64)
    mean64, rstd64 = y64.mean(0), 1.0 / np.sqrt(y64.var(0) + R.EPS)
    mean, rstd = mean64.astype(np.float32), rstd64.astype(np.float32)  # what a forward finalisation left in the block
    part = R.bwd_partial_rows(g, y, mean, rows)
    ref = R.bwd_reference(part, n, gamma, rstd)
    auto_dgamma, auto_dbeta = _autograd_param_grads(y, g, gamma)
    # Against autograd (exact mean, rstd and sums) the kernel's inputs are already rounded:
    #   rows:  each float32 row is within U of its float64 block sum -> the column sums within U * sum_r |row_r| (+ the fold's allowance);
    #   MEAN:  sum g (y - mean_f32) = sum g (y - mean) + (mean - mean_f32) sum g, |mean - mean_f32| <= U |mean|;
    #   RSTD:  within U relative;  the float32 result: U more, and bwd_reference's 2U covers the double arithmetic.
    d1, d2 = R.fold_allowance(part)
    rows_a, rows_b = U * np.abs(part[:, 0].astype(np.float64)).sum(0) + d1, U * np.abs(part[:, 1].astype(np.float64)).sum(0) + d2
    tol_dbeta = rows_a + 2 * U * np.abs(auto_dbeta)
    tol_dgamma = rstd64 * (rows_b + U * np.abs(mean64) * np.abs(g.astype(np.float64).sum(0))) + 3 * U * np.abs(auto_dgamma)
    old_g, old_b = rng.normal(0, 50, C).astype(np.float32), rng.normal(0, 50, C).astype(np.float32)
    d_gamma = _t(gamma)
    for accumulate, with_grads in ((0, True), (1, True), (0, False)):
        ctx = (C, rows, accumulate, with_grads)
        bn0 = _sentinel_bn(C, rng, (AUX_DY_BOUND, AUX_GMAX))
        bn0[BN_MEAN], bn0[BN_RSTD] = mean, rstd
        d_bn, d_dg, d_db, d_part = _t(bn0), _t(old_g), _t(old_b), _t(part)  # (a fresh copy of the rows per call: the fold is in place)
        L.call("ttk_bn_bwd_finalize", p(d_part), rows, C, n, p(d_gamma), p(d_bn), p(d_dg) if with_grads else None, p(d_db) if with_grads else None,
               accumulate)
        torch.cuda.synchronize()
        for name, row in (("ga", BN_GA), ("gb", BN_GB), ("gmean", BN_GMEAN)):
            _assert_close(name, d_bn[row], ref[name], ctx)
        got, was = _bits(d_bn), _bits(torch.from_numpy(bn0))
        assert torch.equal(got[:BN_GA], was[:BN_GA]), ("forward rows were touched", ctx)
        assert torch.equal(got[BN_AUX], was[BN_AUX]), ("GMAX == 0: the AUX row must stay as it was", ctx)
        if not with_grads:
            assert torch.equal(_bits(d_dg), _bits(torch.from_numpy(old_g))) and torch.equal(_bits(d_db), _bits(torch.from_numpy(old_b)))
            continue
        # accumulate: float32(old + float32(sum)) - one more rounding of the result, U |old + sum|
        base_g, base_b = (old_g.astype(np.float64), old_b.astype(np.float64)) if accumulate else (0.0, 0.0)
        _assert_close("dgamma", d_dg, (base_g + auto_dgamma, tol_dgamma + accumulate * U * np.abs(base_g + auto_dgamma)), ctx)
        _assert_close("dbeta", d_db, (base_b + auto_dbeta, tol_dbeta + accumulate * U * np.abs(base_b + auto_dbeta)), ctx)
        # ... and against the same float32 rows (sharper: no input rounding)
        _assert_close("dgamma/rows", d_dg, (base_g + ref["dgamma"][0], ref["dgamma"][1] + accumulate * U * np.abs(base_g + ref["dgamma"][0])), ctx)
        _assert_close("dbeta/rows", d_db, (base_b + ref["dbeta"][0], ref["dbeta"][1] + accumulate * U * np.abs(base_b + ref["dbeta"][0])), ctx)


@pytest.mark.parametrize("case", ["gaussian", "spike_g", "spike_y", "spike_both", "offset_g"])
def test_bwd_finalize_dy_bound_contract(case):
    """GMAX preset to max |g|:  max |ga (g - gmean) + gb (y - mean)| <= DY_BOUND <= 2 * formula64 (the comment of
    bn_bwd_finalize_body: |ga| (gmax + |gmean|) + |gb| sqrt(count) / rstd), with the kernel's own rows on the left.  A one-hot
    spike is where |g - gmean| and |y - mean| reach their bounds."""
    L, p = _lib()
    rng = np.random.default_rng(31)
    y, g = rng.normal(0, 1, _C) + rng.standard_normal((_N, _C)), rng.standard_normal((_N, _C))
    px = rng.integers(0, _N, _C)
    if case in ("spike_g", "spike_both"):
        g[:] = 0
        g[px, np.arange(_C)] = rng.choice([-1.0, 1.0], _C) * (1 + rng.random(_C))
    if case in ("spike_y", "spike_both"):
        y[:] = 0
        y[px, np.arange(_C)] = rng.choice([-1.0, 1.0], _C) * (1 + 4 * rng.random(_C))
    if case == "offset_g":  # -a everywhere, +a at one pixel: max |g| = a but |g - gmean| reaches 2a - the |gmean| term of the bound carries it
        a = 1 + rng.random(_C)
        g[:] = -a
        g[px, np.arange(_C)] = a
    y, g = y.astype(np.float32), g.astype(np.float32)
    gamma = ((rng.random(_C) + 0.5) * rng.choice([-1.0, 1.0], _C)).astype(np.float32)
    y64 = y.astype(np.float64)
    mean, rstd = y64.mean(0).astype(np.float32), (1.0 / np.sqrt(y64.var(0) + R.EPS)).astype(np.float32)
    gmax = float(np.abs(g).max())
    part = R.bwd_partial_rows(g, y, mean, _ROWS)
    bn0 = _sentinel_bn(_C, rng, (AUX_DY_BOUND,))
    bn0[BN_MEAN], bn0[BN_RSTD], bn0[BN_AUX, AUX_GMAX] = mean, rstd, gmax
    d_bn, d_part, d_gamma = _t(bn0), _t(part), _t(gamma)
    L.call("ttk_bn_bwd_finalize", p(d_part), _ROWS, _C, _N, p(d_gamma), p(d_bn), None, None, 0)
    torch.cuda.synchronize()
    bn = d_bn.cpu().numpy()
    true_max = R.dy_true_max(g, y, bn[BN_GA], bn[BN_GB], bn[BN_GMEAN], bn[BN_MEAN])
    formula = float(R.dy_formula(g, y, gamma, gmax).max())
    bound = float(bn[BN_AUX, AUX_DY_BOUND])
    print(f"dy bound {case}: true_max {true_max:.6g}  bound {bound:.6g}  formula64 {formula:.6g}")
    assert true_max <= bound, (case, true_max, bound)
    assert bound <= 2.0 * formula, (case, bound, formula)
    keep = torch.ones(_C, dtype=torch.bool)
    keep[AUX_DY_BOUND] = False
    assert torch.equal(_bits(d_bn)[BN_AUX][keep], _bits(torch.from_numpy(bn0))[BN_AUX][keep])
    # GMAX == 0 (no producer left a maximum): DY_BOUND stays bitwise as it was, whatever it was
    bn1 = bn0.copy()
    bn1[BN_AUX, AUX_GMAX], bn1[BN_AUX, AUX_DY_BOUND] = 0.0, 3.25e-7
    d_bn1 = _t(bn1)
    L.call("ttk_bn_bwd_finalize", p(d_part), _ROWS, _C, _N, p(d_gamma), p(d_bn1), None, None, 0)
    torch.cuda.synchronize()
    assert torch.equal(_bits(d_bn1)[BN_AUX], _bits(torch.from_numpy(bn1))[BN_AUX])


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the frozen pair
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 40, 264, 1000, 2048])
def test_eval_prepare_against_float64(C):
    """bn_eval_prepare_k works in float32: t = fl(rvar + eps), s = fl(sqrt(t)), rstd = fl(1 / s), scale = fl(gamma * rstd), each
    correctly rounded (the library is built without fast-math; division and square root are IEEE then).  Relative errors: t: U;
    s: U/2 inherited + U; rstd: 3U/2 inherited + U = 5U/2; scale: 7U/2.  Allowed: 3U and 4U (second-order terms).  BETA and MEAN
    are copies.  Rows 4 to 7 untouched."""
    L, p = _lib()
    rng = np.random.default_rng(C)
    gamma, beta = ((rng.random(C) + 0.5) * rng.choice([-1.0, 1.0], C)).astype(np.float32), rng.normal(0, 1, C).astype(np.float32)
    rm = rng.normal(0, 3, C).astype(np.float32)
    rv = np.exp(rng.uniform(np.log(1e-8), np.log(1e6), C)).astype(np.float32)
    rv[0] = 0.0
    bn0 = _sentinel_bn(C, rng)
    d_bn = _t(bn0)
    d_gamma, d_beta, d_rm, d_rv = _t(gamma), _t(beta), _t(rm), _t(rv)  # (named: they must outlive the call)
    L.call("ttk_bn_eval_prepare", p(d_gamma), p(d_beta), p(d_rm), p(d_rv), R.EPS, C, p(d_bn))
    torch.cuda.synchronize()
    rstd = 1.0 / np.sqrt(rv.astype(np.float64) + R.EPS)
    _assert_close("rstd", d_bn[BN_RSTD], (rstd, 3 * U * rstd), C)
    _assert_close("scale", d_bn[BN_SCALE], (gamma * rstd, 4 * U * np.abs(gamma * rstd)), C)
    got, was = _bits(d_bn), _bits(torch.from_numpy(bn0))
    assert torch.equal(got[BN_BETA], _bits(torch.from_numpy(beta))) and torch.equal(got[BN_MEAN], _bits(torch.from_numpy(rm)))
    assert torch.equal(got[BN_GA:], was[BN_GA:]), "rows 4 to 7 were touched"


@pytest.mark.parametrize("where", ["last_channel", "last_wave"])
@pytest.mark.parametrize("C", [8, 264, 1000, 2048])
def test_bwd_frozen(C, where):
    """One workgroup of 256 threads strides over the channels and reduces over four waves: GA = SCALE bitwise, GB = GMEAN = 0,
    max |scale g| <= DY_BOUND <= 2 max|scale| gmax, with the largest |scale| in the last channel (the ragged tail of the strided
    loop: C mod 256 = 8, 8, 232, 0) or in a channel that thread 192..255 - the last wave - owns."""
    L, p = _lib()
    rng = np.random.default_rng(C)
    scale = ((rng.random(C) + 0.5) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    in_last_wave = [c for c in range(C) if c % 256 >= 192]
    top = C - 1 if (where == "last_channel" or not in_last_wave) else in_last_wave[len(in_last_wave) // 2]
    scale[top] = -37.5
    g = rng.standard_normal((512, C)).astype(np.float32)
    g[5, top] = 6.0  # the largest gradient meets the largest scale
    gmax = float(np.abs(g).max())
    bn0 = _sentinel_bn(C, rng, (AUX_DY_BOUND,))
    bn0[BN_SCALE], bn0[BN_AUX, AUX_GMAX] = scale, gmax
    d_bn = _t(bn0)
    L.call("ttk_bn_bwd_frozen", p(d_bn), C)
    torch.cuda.synchronize()
    got, was = _bits(d_bn), _bits(torch.from_numpy(bn0))
    assert torch.equal(got[BN_GA], was[BN_SCALE])
    assert torch.equal(got[BN_GB], torch.zeros(C, dtype=torch.int32)) and torch.equal(got[BN_GMEAN], torch.zeros(C, dtype=torch.int32))
    assert torch.equal(got[:BN_GA], was[:BN_GA])
    keep = torch.ones(C, dtype=torch.bool)
    keep[AUX_DY_BOUND] = False
    assert torch.equal(got[BN_AUX][keep], was[BN_AUX][keep])
    bound = float(d_bn[BN_AUX, AUX_DY_BOUND])
    true_max = float(np.abs(scale.astype(np.float64) * g.astype(np.float64)).max())
    assert true_max <= bound <= 2.0 * float(np.abs(scale).max()) * gmax, (C, where, true_max, bound)
    bn1 = bn0.copy()
    bn1[BN_AUX, AUX_GMAX], bn1[BN_AUX, AUX_DY_BOUND] = 0.0, 3.25e-7
    d_bn1 = _t(bn1)
    L.call("ttk_bn_bwd_frozen", p(d_bn1), C)
    torch.cuda.synchronize()
    assert torch.equal(_bits(d_bn1)[BN_AUX], _bits(torch.from_numpy(bn1))[BN_AUX]), "GMAX == 0 must leave DY_BOUND alone"


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the contract inside a real step (MobileNet, fp32 path)
# ------------------------------------------------------------------------------------------------------------------------------
_B, _HW = 32, 129


def _make_net(width, blurpool, seed=0):
    from trackertraincode.backbones.mobilenet_v1 import MobileNet

    torch.manual_seed(seed)
    net = MobileNet(num_classes=None, widen_factor=width, use_blurpool=blurpool).cuda()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():  # BatchNorm parameters and statistics off their initial 1 / 0: both signs of beta, channels off zero
        for bn in net._bns():
            bn.weight.copy_((torch.rand(bn.weight.shape, generator=g) + 0.5).cuda())
            bn.bias.copy_((torch.randn(bn.bias.shape, generator=g) * 0.3).cuda())
    return net.train()


def _step(net, x, gfeat, frozen):
    """One forward + backward through the launch sequences themselves -> (ctx of the forward with AUX rows as the backward left them,
    [(label, ACT_BOUND, true_max)] of the forward, taken BEFORE the backward)."""
    import trackertraincode._hip as H
    from trackertraincode.backbones import mobilenet_v1 as M

    momentum, eps = net._check(x)
    params = [q.detach() for q in net._flat_params()]
    feat, ctx = M._forward_impl(x, params, net._flat_buffers(), momentum, eps, training=not frozen, frozen=frozen, blur=net._blur_weights(),
                                blocks=net._blocks)
    torch.cuda.synchronize()
    names = ["conv1"] + [f"{name}.{part}" for name, *_ in net._blocks for part in ("conv_dw", "conv_sep")]
    fwd = []
    for label, st in zip(names, ctx.stages):
        assert bool(torch.isfinite(st.bn).all()), label
        if st.skip is not None:
            continue  # (relu(bn(y) + skip): the depthwise kernels read it; no GEMM scales by this block's ACT_BOUND)
        C = st.y.shape[-1]
        y = H.from_blocks_any(st.y).reshape(-1, C).double()
        bn = st.bn.double()
        true_max = float(torch.clamp_min(bn[BN_SCALE] * (y - bn[BN_MEAN]) + bn[BN_BETA], 0).max())
        fwd.append((label, float(st.bn[BN_AUX, AUX_ACT_BOUND]), true_max))
    M._backward_impl(ctx, gfeat, params)
    torch.cuda.synchronize()
    return ctx, fwd


@pytest.mark.parametrize("width,blurpool,frozen", [(1.0, False, False), (0.75, False, False), (1.0, True, False), (1.0, False, True),
                                                   (0.75, True, True)])
def test_bounds_hold_inside_a_training_step(width, blurpool, frozen):
    """Every stage whose block has no residual input: true_max (float64, from the stored y and the written rows) <= ACT_BOUND, all of
    bn finite; after the backward GMAX and DY_BOUND finite and positive where a GEMM consumes them (the pointwise stages of the tuned
    layers).  The looseness ACT_BOUND / true_max stays within 2^12 - up to which tests/test_range_stress_gpu.py proves the consumers
    accurate - on the stages a GEMM reads (the depthwise stages; printed for all)."""
    net = _make_net(width, blurpool)
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(_B, 1, _HW, _HW, generator=g) * 0.5 + 0.2).cuda()
    if frozen:  # running statistics that a few training steps left, then frozen (prepare_finetune() + train(): BatchNorm in eval mode)
        with torch.no_grad():
            for _ in range(3):
                net.forward_features((torch.randn(_B, 1, _HW, _HW, generator=g) * 0.5 + 0.2).cuda())
        net.prepare_finetune()
        net.train()
        for bn in net._bns():
            bn.eval()
    gfeat = (torch.randn(_B, net.num_features, generator=g) / _B).cuda()
    ctx, fwd = _step(net, x, gfeat, frozen)
    worst = 0.0
    for label, bound, true_max in fwd:
        loose = bound / true_max if true_max > 0 else float("nan")
        print(f"width {width} blur {blurpool} frozen {frozen}  {label:18s} ACT_BOUND {bound:.5g}  true_max {true_max:.5g}  looseness {loose:.1f}")
        assert np.isfinite(bound) and true_max <= bound, (label, true_max, bound)
        if label.endswith("conv_dw") and true_max > 0:
            worst = max(worst, loose)
            assert loose <= 2.0 ** 12, (label, loose)
    print(f"width {width} blur {blurpool} frozen {frozen}: worst looseness of a GEMM-read bound {worst:.1f} at B = {_B}")
    for k in range(len(net._blocks)):
        for st in (ctx.stages[2 * k + 1], ctx.stages[2 * k + 2]):
            assert bool(torch.isfinite(st.bn).all())
        if ctx.prep[k] is not None:  # a tuned pointwise layer: its backward GEMMs scale by bn_sep's GMAX / DY_BOUND
            aux = ctx.stages[2 * k + 2].bn[BN_AUX]
            assert float(aux[AUX_GMAX]) > 0 and float(aux[AUX_DY_BOUND]) > 0, (k, aux[:3])


@pytest.mark.parametrize("frozen", [False, True])
def test_no_stale_maxima_carry_over_between_steps(frozen):
    """AUX is raised with a monotone atomicMax, so it must start every step at zero: a step on a batch, then (running statistics
    restored) a step on the same batch scaled by 1/100 - the second step's AUX rows equal, bitwise, those of a fresh identical network
    that only ever saw the small batch."""
    net = _make_net(1.0, False)
    if frozen:
        for bn in net._bns():
            bn.eval()
    fresh = copy.deepcopy(net)
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(8, 1, _HW, _HW, generator=g) * 0.5 + 0.2).cuda()
    gfeat = (torch.randn(8, net.num_features, generator=g) / 8).cuda()
    saved = [b.clone() for b in net._flat_buffers()]
    _step(net, x, gfeat, frozen)
    with torch.no_grad():
        for b, s in zip(net._flat_buffers(), saved):
            b.copy_(s)
    aux = lambda ctx: [_bits(st.bn[BN_AUX]) for st in ctx.stages]
    second = aux(_step(net, x / 100, gfeat / 100, frozen)[0])
    alone = aux(_step(fresh, x / 100, gfeat / 100, frozen)[0])
    for k, (a, b) in enumerate(zip(second, alone)):
        assert torch.equal(a, b), ("stage", k, a[:3], b[:3])


# ------------------------------------------------------------------------------------------------------------------------------
# 6. bad arguments
# ------------------------------------------------------------------------------------------------------------------------------
def test_bn_entry_points_reject_null_pointers_and_bad_sizes():
    """Negative return code -> RuntimeError carrying ttk_last_error_string(); nothing is launched (the block stays as it was)."""
    L, p = _lib()
    C = 32
    t = torch.ones(64, device="cuda")
    part = torch.ones(2, 2, C, device="cuda")
    bn = torch.full((8, C), 2.0, device="cuda")
    cases = [
        ("null pointer", "ttk_bn_fwd_finalize", (None, None, 2, C, 10, p(t), p(t), None, None, None, 0.1, 1e-5, p(bn))),
        ("null pointer", "ttk_bn_fwd_finalize", (p(part), None, 2, C, 10, None, p(t), None, None, None, 0.1, 1e-5, p(bn))),
        ("null pointer", "ttk_bn_fwd_finalize", (p(part), None, 2, C, 10, p(t), None, None, None, None, 0.1, 1e-5, p(bn))),
        ("null pointer", "ttk_bn_fwd_finalize", (p(part), None, 2, C, 10, p(t), p(t), None, None, None, 0.1, 1e-5, None)),
        ("running_mean/var", "ttk_bn_fwd_finalize", (p(part), None, 2, C, 10, p(t), p(t), p(t), None, None, 0.1, 1e-5, p(bn))),
        ("bad sizes", "ttk_bn_fwd_finalize", (p(part), None, 2, C, 0, p(t), p(t), None, None, None, 0.1, 1e-5, p(bn))),
        ("null pointer", "ttk_bn_eval_prepare", (None, p(t), p(t), p(t), 1e-5, C, p(bn))),
        ("null pointer", "ttk_bn_eval_prepare", (p(t), None, p(t), p(t), 1e-5, C, p(bn))),
        ("null pointer", "ttk_bn_eval_prepare", (p(t), p(t), None, p(t), 1e-5, C, p(bn))),
        ("null pointer", "ttk_bn_eval_prepare", (p(t), p(t), p(t), None, 1e-5, C, p(bn))),
        ("null pointer", "ttk_bn_eval_prepare", (p(t), p(t), p(t), p(t), 1e-5, C, None)),
        ("bn_eval_prepare", "ttk_bn_eval_prepare", (p(t), p(t), p(t), p(t), 1e-5, 0, p(bn))),
        ("null pointer", "ttk_bn_bwd_finalize", (None, 2, C, 10, p(t), p(bn), None, None, 0)),
        ("null pointer", "ttk_bn_bwd_finalize", (p(part), 2, C, 10, None, p(bn), None, None, 0)),
        ("null pointer", "ttk_bn_bwd_finalize", (p(part), 2, C, 10, p(t), None, None, None, 0)),
        ("dgamma/dbeta", "ttk_bn_bwd_finalize", (p(part), 2, C, 10, p(t), p(bn), p(t), None, 0)),
        ("dgamma/dbeta", "ttk_bn_bwd_finalize", (p(part), 2, C, 10, p(t), p(bn), None, p(t), 0)),
        ("bad sizes", "ttk_bn_bwd_finalize", (p(part), 0, C, 10, p(t), p(bn), None, None, 0)),
        ("bn_frozen_bound", "ttk_bn_frozen_bound", (None, None, 2, C, 10, p(bn))),
        ("bn_frozen_bound", "ttk_bn_frozen_bound", (p(part), None, 2, C, 10, None)),
        ("bn_frozen_bound", "ttk_bn_frozen_bound", (p(part), None, 0, C, 10, p(bn))),
        ("bn_frozen_bound", "ttk_bn_frozen_bound", (p(part), None, 2, C, 0, p(bn))),
        ("bn_bwd_frozen", "ttk_bn_bwd_frozen", (None, C)),
        ("bn_bwd_frozen", "ttk_bn_bwd_frozen", (p(bn), 0)),
    ]
    for match, name, args in cases:
        with pytest.raises(RuntimeError, match=match):
            L.call(name, *args)
    torch.cuda.synchronize()
    assert bool((bn == 2.0).all()) and bool((part == 1.0).all()) and bool((t == 1.0).all())
