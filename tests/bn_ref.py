"""Float64 reference of the BatchNorm finalisation kernels (csrc/bn.hip) and of the operand bounds they leave in row TTK_BN_AUX
(include/ttk.h).  Plain numpy, no GPU: tests/test_bn_finalize_gpu.py compares the kernels with it, tests/test_bn_ref.py pins it on
its own.  Everything here works on what the kernels are GIVEN - float32 partial rows `part[rows][2][C]`, float32 y / g - in float64."""
import numpy as np

BN_SCALE, BN_BETA, BN_MEAN, BN_RSTD, BN_GA, BN_GB, BN_GMEAN, BN_AUX = range(8)
AUX_ACT_BOUND, AUX_DY_BOUND, AUX_GMAX = 0, 1, 2
FOLD_ROWS = 1024           # kFoldRows of csrc/bn.hip: rows r, r + 1024, ... are folded into row r ...
FOLD_ABOVE = 1280          # ... when there are more than this many
U = 2.0 ** -24             # unit roundoff of float32 (round to nearest): |fl(x) - x| <= U |x|
MOMENTUM = float(np.float32(0.1))  # the entry point takes float arguments: the kernel sees float32(0.1) widened, not 0.1
EPS = float(np.float32(1e-5))


def partial_rows(v1, v2, rows):
    """`rows` float32 partial rows [rows][2][C] of the per-pixel float64 terms v1, v2 [n][C]: pixel blocks of n/rows, each summed
    in float64 and rounded to float32 once (n must be a multiple of rows)."""
    n, C = v1.shape
    assert n % rows == 0, (n, rows)
    part = np.empty((rows, 2, C), np.float32)
    part[:, 0] = v1.reshape(rows, n // rows, C).sum(1)
    part[:, 1] = v2.reshape(rows, n // rows, C).sum(1)
    return part


def fwd_partial_rows(y, pivot, rows):
    """What a forward producer leaves: sums of (y - pivot) and (y - pivot)^2 (pivot None: of y, y^2)."""
    d = y.astype(np.float64) - (0.0 if pivot is None else pivot.astype(np.float64))
    return partial_rows(d, d * d, rows)


def fold64(part):
    """The in-place fold of the finalisations, in float64: (folded rows [<=1024][2][C], sum of |terms| per folded element)."""
    p = part.astype(np.float64)
    if p.shape[0] <= FOLD_ABOVE:
        return p, np.abs(p)
    out, mag = p[:FOLD_ROWS].copy(), np.abs(p[:FOLD_ROWS])
    for lo in range(FOLD_ROWS, p.shape[0], FOLD_ROWS):
        blk = p[lo:lo + FOLD_ROWS]          # (the last one is ragged)
        out[:blk.shape[0]] += blk
        mag[:blk.shape[0]] += np.abs(blk)
    return out, mag


def fold32_kahan(part):
    """The fold as csrc/bn.hip does it: float32 with Kahan compensation, row r <- r, r + 1024, ...  (emulation for the CPU tests)."""
    p = part.astype(np.float32)
    if p.shape[0] <= FOLD_ABOVE:
        return p
    acc, comp = p[:FOLD_ROWS].copy(), np.zeros_like(p[:FOLD_ROWS])
    for lo in range(FOLD_ROWS, p.shape[0], FOLD_ROWS):
        k = min(FOLD_ROWS, p.shape[0] - lo)
        v = p[lo:lo + k] - comp[:k]
        t = acc[:k] + v
        comp[:k] = (t - acc[:k]) - v
        acc[:k] = t
    return acc


def fold_allowance(part):
    """(D1, D2)[C]: how far the column sums S1, S2 of the float32-Kahan-folded rows may lie from those of the exact rows.
    Kahan summation of m terms errs by at most (2U + O(m U^2)) * sum|x_i| (Higham, Accuracy and Stability, eq. 4.8); m <= 5 here,
    the second-order term is 1e-14 relative: 2^-23 (1 + 2^-20) of the folded magnitude per element, summed over the 1024 elements
    of a column.  Zero without a fold."""
    if part.shape[0] <= FOLD_ABOVE:
        z = np.zeros(part.shape[2])
        return z, z
    _, mag = fold64(part)
    d = 2.0 * U * (1.0 + 2.0 ** -20) * mag.sum(0)
    return d[0], d[1]


def fwd_stats(part, pivot, count, s1_shift=0.0, s2_shift=0.0):
    """mean, biased variance (clamped at 0), shifted mean, E[(y - pivot)^2] from float32 partial rows, in float64.
    s1_shift / s2_shift move the column sums (error propagation)."""
    p, _ = fold64(part)
    s1, s2 = p[:, 0].sum(0) + s1_shift, p[:, 1].sum(0) + s2_shift
    shifted = s1 / count
    mean = shifted + (0.0 if pivot is None else pivot.astype(np.float64))
    var = np.maximum(s2 / count - shifted * shifted, 0.0)
    return mean, var, shifted, s2 / count


def fwd_reference(part, pivot, count, gamma, beta, rmean, rvar, momentum=MOMENTUM, eps=EPS):
    """Rows and running statistics of ttk_bn_fwd_finalize with their allowances.  Returns {name: (want, tol)}, float64 [C].

    The kernel accumulates the rows, forms mean / var / rstd / scale and the running updates in double and rounds each RESULT to
    float32 once.  So against the same computation in float64:
      * rounding of the result: <= U |want| (round to nearest);  allowed 2U |want| - a factor 2 for the double arithmetic below;
      * the double arithmetic itself (another summation order over <= 1280 rows, fused multiply-adds): <= rows * 2^-53 relative to the
        sums, amplified in the variance by E[(y-pivot)^2] / (var + eps) - the callers keep var >= E[(y-pivot)^2] / 12 (stated
        where the inputs are made), so < 1280 * 12 * 2^-53 = 2e-12 relative: far inside the factor 2 above.  The mean adds
        pivot + shifted, which may cancel: 2^-50 (|pivot| + |shifted|) absolute covers its double rounding;
      * above 1280 rows the fold is float32 (Kahan): the column sums move by at most fold_allowance(), propagated EXACTLY by evaluating
        the same formulas at the four corners S1 +- D1, S2 +- D2 (each output is monotone in S1 at fixed S2 and in S2 at fixed S1 between
        the corners for the inputs used here: |shifted| well above D1/count or the term is second order; the corner spread is then
        the largest change)."""
    gamma64, beta64 = gamma.astype(np.float64), beta.astype(np.float64)
    unbias = count / (count - 1.0) if count > 1 else 1.0

    def outputs(s1_shift, s2_shift):
        mean, var, shifted, _ = fwd_stats(part, pivot, count, s1_shift, s2_shift)
        rstd = 1.0 / np.sqrt(var + eps)
        o = {"scale": gamma64 * rstd, "beta": beta64, "mean": mean, "rstd": rstd}
        if rmean is not None:
            o["running_mean"] = (1.0 - momentum) * rmean.astype(np.float64) + momentum * mean
            o["running_var"] = (1.0 - momentum) * rvar.astype(np.float64) + momentum * var * unbias
        return o

    want = outputs(0.0, 0.0)
    d1, d2 = fold_allowance(part)
    spread = {k: np.zeros_like(v) for k, v in want.items()}
    if part.shape[0] > FOLD_ABOVE:
        for a in (-1.0, 1.0):
            for b in (-1.0, 1.0):
                for k, v in outputs(a * d1, b * d2).items():
                    spread[k] = np.maximum(spread[k], np.abs(v - want[k]))
    _, _, shifted, _ = fwd_stats(part, pivot, count)
    piv = 0.0 if pivot is None else np.abs(pivot.astype(np.float64))
    out = {}
    for k, v in want.items():
        tol = 2.0 * U * np.abs(v) + spread[k]
        if k in ("mean", "running_mean"):
            tol = tol + 2.0 ** -50 * (piv + np.abs(shifted))
        if k == "beta":
            tol = np.zeros_like(v)  # a copy
        out[k] = (v, tol)
    return out


def act_true_max(y, scale, beta, mean):
    """max |max(scale*(y-mean)+beta, 0)| over pixels and channels: the tensor the consumers form from y and the written rows."""
    a = scale.astype(np.float64) * (y.astype(np.float64) - mean.astype(np.float64)) + beta.astype(np.float64)
    return float(np.maximum(a, 0.0).max())


def act_formula(y, gamma, beta, eps=EPS):
    """The documented bound of ttk_bn_fwd_finalize per channel, |scale| sqrt(count var) + |beta|, from the float64 statistics of y."""
    y64 = y.astype(np.float64)
    n = y64.shape[0]
    mean, var = y64.mean(0), y64.var(0)
    scale = gamma.astype(np.float64) / np.sqrt(var + eps)
    return np.abs(scale) * np.sqrt(n * var) + np.abs(beta.astype(np.float64)), scale, mean


def frozen_formula(y, scale, beta, mean_run):
    """The documented bound of ttk_bn_frozen_bound per channel: |scale| (sqrt(count var_b) + |mean_b - mean_run|) + |beta|, with the
    batch statistics of y in float64 and the rows ttk_bn_eval_prepare wrote."""
    y64 = y.astype(np.float64)
    n = y64.shape[0]
    mean_b, var_b = y64.mean(0), y64.var(0)
    return (np.abs(scale.astype(np.float64)) * (np.sqrt(n * var_b) + np.abs(mean_b - mean_run.astype(np.float64)))
            + np.abs(beta.astype(np.float64)))


FAMILIES = ("gaussian", "spike", "constant", "far13", "neg_gamma", "big_beta", "all_negative", "tiny", "huge")


def family(name, n, C, rng):
    """(y [n][C] float32, gamma [C], beta [C]) of one input family of the forward bound contract.

    fp32 range of the sums of squares (the partial rows are float32): "huge" has |y| ~ 1e15 N(0,1), squares ~ 1e30 and a whole
    column sums to n * 1e30 <= 1e34 for n <= 1e4, under FLT_MAX = 3.4e38.  "tiny" has |y| ~ 1e-20 N(0,1): a square is 1e-40, a float32
    SUBNORMAL, so the callers use at most n / 512 partial rows for it - a row then sums >= 512 squares to ~5e-38, above FLT_MIN =
    1.18e-38, a normal number with full precision (the float64 block sum is rounded once)."""
    gamma = (rng.random(C) + 0.5).astype(np.float32)
    beta = (rng.normal(0, 0.2, C)).astype(np.float32)
    z = rng.standard_normal((n, C))
    if name == "gaussian":
        y = rng.normal(0, 1, C) + (rng.random(C) + 0.5) * z
    elif name == "spike":  # ONE pixel non-zero per channel: |y - mean| = sqrt(count var) up to 1 - 1/n, Cauchy-Schwarz is tight
        y = np.zeros((n, C))
        y[rng.integers(0, n, C), np.arange(C)] = rng.choice([-1.0, 1.0], C) * (rng.random(C) * 4 + 1)
        beta = np.abs(beta)  # the positive side survives the ReLU where gamma * spike > 0
    elif name == "constant":
        # variance exactly 0 (the clamp var < 0 -> 0 decides).  From float32 sums no finalisation can know the variance of such a channel
        # closer than ~2^-23 E[y^2] (the rounding of S2 alone), so SOME slack of |scale| sqrt(n 2^-23 E[y^2]) is in every sound bound;
        # the value c is chosen so that this resolution term, with |gamma| <= 1.5 and rstd = 1/sqrt(eps), stays an order of
        # magnitude below |beta| = 1: 1.5 * 316 * sqrt(n * 2^-23) * |c| <= 1/8  <=>  |c| <= 0.76 / sqrt(n)
        c = rng.choice([-1.0, 1.0], C) * (0.25 + 0.5 * rng.random(C)) / np.sqrt(n)
        c[::4] = 0.0  # (dead channels: exactly zero)
        y = np.broadcast_to(c, (n, C)).copy()
        beta = rng.choice([-1.0, 1.0], C).astype(np.float32)
    elif name == "far13":
        s = rng.random(C) + 0.5
        y = rng.choice([-13.0, 13.0], C) * s + s * z
    elif name == "neg_gamma":
        gamma = -gamma
        y = rng.normal(0, 1, C) + z
    elif name == "big_beta":  # |beta| 1e3 times the scaled spread of ~sqrt(n)
        y = z
        beta = (rng.choice([-1.0, 1.0], C) * 1e3 * np.sqrt(n)).astype(np.float32)
    elif name == "all_negative":  # beta below -|scale| max|y - mean|: relu(...) = 0 everywhere, the true maximum is 0
        y = rng.normal(0, 1, C) + z
        beta = (-2.0 * np.abs(gamma) * np.sqrt(n)).astype(np.float32)
    elif name == "tiny":
        y = 1e-20 * z
    elif name == "huge":
        y = 1e15 * (rng.normal(0, 1, C) + z)
    else:
        raise KeyError(name)
    return y.astype(np.float32), gamma, beta


def mixed(n, C, rng):
    """Channel c takes family c mod 9 - every family in one call (and in one 32-channel workgroup)."""
    y, gamma, beta = np.empty((n, C), np.float32), np.empty(C, np.float32), np.empty(C, np.float32)
    for i, f in enumerate(FAMILIES):
        yf, gf, bf = family(f, n, C, rng)
        sel = np.arange(C) % len(FAMILIES) == i
        y[:, sel], gamma[sel], beta[sel] = yf[:, sel], gf[sel], bf[sel]
    return y, gamma, beta


def bwd_partial_rows(g, y, mean, rows):
    """What a backward producer leaves: sums of g and g * (y - mean) with the float32 MEAN row of the block."""
    g64 = g.astype(np.float64)
    return partial_rows(g64, g64 * (y.astype(np.float64) - mean.astype(np.float64)), rows)


def bwd_reference(part, count, gamma, rstd):
    """Rows GA, GB, GMEAN and the parameter gradients of ttk_bn_bwd_finalize by their definitions (include/ttk.h) from the float32
    partial rows and the float32 RSTD row, in float64: {name: (want, tol)}.

    As in fwd_reference the kernel works in double and rounds each result once: 2U |want|.  Every output is LINEAR in one column sum
    (sum g: gmean, dbeta;  sum g (y-mean): gb, dgamma), so above 1280 rows the fold's allowance D propagates as |d out / d S| * D."""
    p, _ = fold64(part)
    s_g, s_gx = p[:, 0].sum(0), p[:, 1].sum(0)
    d1, d2 = fold_allowance(part)
    rs, ga64 = rstd.astype(np.float64), gamma.astype(np.float64)
    A = ga64 * rs
    want = {"ga": (A, 0.0), "gb": (-A * rs * rs * s_gx / count, np.abs(A) * rs * rs * d2 / count), "gmean": (s_g / count, d1 / count),
            "dgamma": (rs * s_gx, rs * d2), "dbeta": (s_g, d1)}
    return {k: (v, 2.0 * U * np.abs(v) + lin) for k, (v, lin) in want.items()}


def dy_true_max(g, y, ga, gb, gmean, mean):
    f = lambda t: t.astype(np.float64)
    return float(np.abs(f(ga) * (f(g) - f(gmean)) + f(gb) * (f(y) - f(mean))).max())


def dy_formula(g, y, gamma, gmax, eps=EPS):
    """The bound in the comment of bn_bwd_finalize_body per channel, in float64 from y and g themselves:
    |ga| (gmax + |gmean|) + |gb| sqrt(count) / rstd."""
    y64, g64 = y.astype(np.float64), g.astype(np.float64)
    n = y64.shape[0]
    mean, var = y64.mean(0), y64.var(0)
    rstd = 1.0 / np.sqrt(var + eps)
    A = gamma.astype(np.float64) * rstd
    gb = -A * rstd * rstd * (g64 * (y64 - mean)).mean(0)
    return np.abs(A) * (gmax + np.abs(g64.mean(0))) + np.abs(gb) * np.sqrt(n) / rstd
