"""Float64 reference of one call of the fused global-norm clip + Adam step (ttk_clip_adam / ttk_clip_adam_guarded, csrc/adam.hip), the
per-element bounds a float32 run of it must meet, and the table of cases.  Plain numpy.  tests/test_adam_ref.py pins all of it without a
GPU (a float32 emulation meets every bound, fifteen planted errors do not, float64 torch agrees with the reference);
tests/test_adam_rows_gpu.py holds the kernels to it through the C ABI and tests/test_optimizer_gpu.py through train.ClipAdam.

What is computed, from the float32 values the kernel is GIVEN (parameters p, gradients g, moments m and v, steps[], and the float32
lr / wd / beta1 / beta2 / eps / max_norm / grad_scale of the ABI), all widened to float64:
    S = sum g^2 over the tensors with a gradient        total = grad_scale * sqrt(S)
    coef = grad_scale * (max_norm > 0 ? min(max_norm / (total + 1e-6), 1) : 1)
    t = steps + 1 where there is a gradient
    g' = coef*g + wd*p        m' = b1*m + (1 - b1)*g'        v' = b2*v + (1 - b2)*g'^2
    p' = p - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
A tensor without a gradient keeps p, m, v bitwise and its step count.

Every bound is derived from u = 2^-24, the unit roundoff of float32, by counting the kernel's float32 roundings.  Division and square
root are correctly rounded in this build (csrc/Makefile passes no fast-math flag, and hipcc's default for float32 `/` and sqrtf is the
correctly rounded form), so each counts one rounding; an explicit fmaf counts one; every other operation counts one whether or not the
compiler contracts it with a neighbour (a contraction only removes a rounding).  fp64 operations are not counted: their 2^-53 is
inside the "+ 1" that each count carries for second-order terms.

  * norm.  A chunk's partial sum: every thread runs an fma chain over its elements - at most 4*ceil(chunk_size/1024) in the 16-byte
    body plus one of the scalar tail, L = 4*ceil(chunk_size/1024) + 1 (the scalar path's ceil(chunk_size/256) is no longer) - then 6
    shuffle levels and the 4 wave adds.  All terms are non-negative, so the partial, and with it S, is off by at most (L + 10)u
    relative; the bound holds for ANY order in which no square passes through more than L + 10 float32 additions.  The partials are
    added in fp64.  The square root halves the error; the cast to float32 and the product with grad_scale add one rounding each:
        e_norm = ((L + 11)/2 + 2) u        |out_norm - total| <= e_norm * total.
  * coef.  total + 1e-6f (one rounding; the float32 constant is 1e-6 to 2.8e-9, which moves the sum by less than u/20), the division,
    the product with grad_scale: e_coef = e_norm + 5u (3 roundings, the constant, second order).  min(., 1) is 1-Lipschitz and exact,
    so the step has no discontinuity and no element is left out; where the float64 ratio max_norm/(total + 1e-6) exceeds 1 by more
    than 2*(e_norm + 3u) the float32 ratio exceeds 1 too and coef is grad_scale exactly: e_coef = 0, as with max_norm = 0.
  * g'.  With cg = coef*g and the yardstick Y_g = |cg| + wd*|p| (the sum can cancel): the scaling and the fma give
        E_g = (e_coef + u)|cg| + u*Y_g.
  * m'.  Yardstick Y_m = b1*|m| + (1 - b1)*Y_g (it can cancel too).  1 - b1, the product, the fma:
        E_m = (1 - b1)(E_g + 2u*Y_g) + 2u*Y_m        (the fma's rounding and one for second order).
  * v'.  A sum of non-negative terms.  1 - b2, two products, the fma:
        E_v = (1 - b2)(2|g'|E_g + E_g^2 + 3u*g'^2) + 2u*v',
    which is relative, (2 e_coef + 9u)v' at most, wherever g' does not cancel (wd = 0).
  * p'.  bc1 and bc2 are casts of fp64 values (u each); step_size = lr/bc1 (2u in all); 1/sqrtf(bc2) (u/2 + u + u = 2.5u);
    denom = sqrtf(v')*inv + eps: E_sqrt = min(sqrt(E_v), E_v/sqrt(v')) bounds what v' hands to its square root (half-relative where v'
    is not tiny), sqrtf and the product add 2u, so
        E_den = (E_sqrt + 4.5u*sqrt(v'))/sqrt(bc2) + u*denom,        e_den = E_den/denom;
    the division m'/denom, the product with step_size and the subtraction add u each:
        T_p = u|p'| + step_size/denom * E_m/(1 - e_den) + |update| * (4u + e_den/(1 - e_den) + 2u)        (2u: second order).
  * subnormals.  FLT_MIN is added to E_g, E_m and E_v and 4*FLT_MIN to T_p and the norm's bound, so a build that flushes subnormal
    intermediates is no failure.  No input is subnormal.
  * exact values.  Where g = m = v = 0 and wd = 0 every operation is exact: p' is p bitwise and m' = v' = 0 (bound 0).  With
    coef == grad_scale == 1 and wd = 0, m' from m = 0 is the ONE product (1 - b1)*g: bound u|m'| (2u where 1 - b1 is not a float32).
  * steps[] is exact.
The assertion is: worst error/bound <= 1, per output, over every element.

torch semantics.  The kernel forms 1 - beta^t in fp64 from the FLOAT32 betas; torch.optim.Adam's default path uses the Python doubles.
float32(0.999) - 0.999 = 1.29e-8, so with the same m' and v' the update differs from double-beta Adam by the relative
    |b32 - b| * t * b^(t-1) / (1 - b^t)        (beta1; half of it for beta2, which sits under the square root):
6.4e-6 at t = 1 for beta2 = 0.999, decaying as t grows.  The moments see the other beta as well: |dm'| <= |b32 - b|(|m| + |g'|),
|dv'| <= |b32 - b|(v + g'^2) (at t = 1 from zero moments these cancel against the bias corrections).  reference().dbeta is the sum of
the four, to first order (the second order, 1e-10 relative, is below u/100); it is added to T_p ONLY when a result is judged against
double-beta semantics (tests/test_optimizer_gpu.py).  torch's own capturable path is coarser; the kernel is not changed for it."""
import math
import types
import zlib

import numpy as np

U = 2.0 ** -24        # unit roundoff of float32
FLT_MIN = 2.0 ** -126
F = np.float32
MAX_GROUPS = 128      # TTK_ADAM_MAX_GROUPS (include/ttk.h)
BAND = 64             # floats of sentinel between and around the tensors of a case
SENTINEL = F(-7251.375)
ROLES = ("p", "g", "m", "v")   # the four addresses of a tensor, in the order of the ABI's pointer table


def hyper(lr, wd, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.0, grad_scale=1.0):
    """The float32 hyper-parameters of one call as the ABI receives them; lr / wd: one value per group, padded to MAX_GROUPS."""
    pad = lambda a: np.concatenate([np.asarray(a, F).reshape(-1), np.zeros(MAX_GROUPS, F)])[:MAX_GROUPS]
    return types.SimpleNamespace(lr=pad(lr), wd=pad(wd), beta1=F(beta1), beta2=F(beta2), eps=F(eps), max_norm=F(max_norm),
                                 grad_scale=F(grad_scale))


def chain_length(chunk):
    return 4 * math.ceil(chunk / 1024) + 1


def norm_rel(chunk):
    """e_norm (module docstring)."""
    return ((chain_length(chunk) + 11) / 2 + 2) * U


def total_norm(g, grad_scale):
    d = [np.asarray(x, np.float64) for x in g if x is not None]
    return float(grad_scale) * math.sqrt(sum(float(np.sum(x * x)) for x in d))


def reference(p, g, m, v, steps, group, h, chunk, betas64=None):
    """One call in float64.  p, g, m, v: per-tensor float32 arrays (g[i] None: no gradient); steps: float32 counts BEFORE the call;
    group[i]: index into h.lr / h.wd.  betas64: the betas as Python doubles instead of the widened float32 ones (double-beta semantics;
    the bounds are still those of the float32 betas).  -> p, m, v (lists, float64), tp, tm, tv (their bounds), dbeta (the double-beta
    term per tensor, zero unless betas64 is given), steps (float32, after), norm, tnorm, coef."""
    d = lambda a: np.asarray(a, np.float64)
    b1, b2 = float(h.beta1), float(h.beta2)
    c1, c2 = betas64 if betas64 is not None else (b1, b2)
    gs, mx, eps = float(h.grad_scale), float(h.max_norm), float(h.eps)
    total = total_norm(g, gs)
    e_n = norm_rel(chunk)
    ratio = mx / (total + 1e-6) if mx > 0 else math.inf
    coef = gs * min(ratio, 1.0)
    e_c = e_n + 5 * U if ratio < 1 + 2 * (e_n + 3 * U) else 0.0
    one_product = coef == 1.0 and gs == 1.0 and e_c == 0.0
    r = types.SimpleNamespace(p=[], m=[], v=[], tp=[], tm=[], tv=[], dbeta=[], steps=np.array(steps, F), norm=total,
                              tnorm=e_n * total + 4 * FLT_MIN, coef=coef)
    for i in range(len(p)):
        P, M, V = d(p[i]), d(m[i]), d(v[i])
        if g[i] is None:
            z = np.zeros_like(P)
            for lst, val in ((r.p, P), (r.m, M), (r.v, V), (r.tp, z), (r.tm, z), (r.tv, z), (r.dbeta, z)):
                lst.append(val)
            continue
        G = d(g[i])
        r.steps[i] = steps[i] + F(1)
        t = float(r.steps[i])
        lr, wd = float(h.lr[group[i]]), float(h.wd[group[i]])
        cg = coef * G
        yg = np.abs(cg) + wd * np.abs(P)
        gp = cg + wd * P
        eg = (e_c + U) * np.abs(cg) + U * yg + FLT_MIN
        m1 = c1 * M + (1 - c1) * gp
        ym = b1 * np.abs(M) + (1 - b1) * yg
        em = (1 - b1) * (eg + 2 * U * yg) + 2 * U * ym + FLT_MIN
        v1 = c2 * V + (1 - c2) * gp * gp
        ev = (1 - b2) * (2 * np.abs(gp) * eg + eg * eg + 3 * U * gp * gp) + 2 * U * v1 + FLT_MIN
        bc1, bc2 = 1 - c1 ** t, 1 - c2 ** t
        step = lr / bc1
        sq = np.sqrt(v1)
        den = sq / math.sqrt(bc2) + eps
        upd = step * m1 / den
        p1 = P - upd
        esq = np.minimum(np.sqrt(ev), ev / np.maximum(sq, 1e-300))
        e_den = ((esq + 4.5 * U * sq) / math.sqrt(bc2) + U * den) / den
        assert float(e_den.max()) < 0.5, "the denominator is not resolved in float32: not a case for this criterion"
        tp = U * np.abs(p1) + step / den * em / (1 - e_den) + np.abs(upd) * (6 * U + e_den / (1 - e_den)) + 4 * FLT_MIN
        tm, tv = em, ev
        if one_product and wd == 0.0:
            exact_1mb1 = float(F(1) - h.beta1) == 1 - b1
            tm = np.where(M == 0, (U if exact_1mb1 else 2 * U) * np.abs(m1) + FLT_MIN, tm)
        if wd == 0.0:
            zero = (G == 0) & (M == 0) & (V == 0)
            tp, tm, tv = np.where(zero, 0.0, tp), np.where(zero, 0.0, tm), np.where(zero, 0.0, tv)
        # against double-beta semantics (module docstring, "torch semantics"), first order
        db1, db2 = abs(b1 - c1), abs(b2 - c2)
        k1 = db1 * t * b1 ** (t - 1) / (1 - b1 ** t)
        k2 = 0.5 * db2 * t * b2 ** (t - 1) / (1 - b2 ** t)
        dbeta = np.abs(upd) * (k1 + k2) + step / den * db1 * (np.abs(M) + np.abs(gp)) \
            + np.abs(upd) * 0.5 * db2 * (V + gp * gp) / np.maximum(v1, 1e-300)
        for lst, val in ((r.p, p1), (r.m, m1), (r.v, v1), (r.tp, tp), (r.tm, tm), (r.tv, tv), (r.dbeta, dbeta)):
            lst.append(val)
    return r


def _worst(err, tol):
    """max err/tol; an error at bound 0 is infinitely far out, none is 0.  NaN propagates (and fails every `<= 1`)."""
    err, tol = np.asarray(err, np.float64), np.asarray(tol, np.float64)
    if err.size == 0:
        return 0.0
    if np.isnan(err).any():
        return float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / np.maximum(tol, 1e-300), np.where(err == 0, 0.0, np.inf))
    return float(ratio.max())


def _nanmax(vals):
    vals = list(vals)
    return float("nan") if any(x != x for x in vals) else max(vals, default=0.0)


def ratios(r, p, m, v, steps, norm=None, extra_p=None):
    """Worst error/bound of one call's float32 results (per-tensor arrays) against `r`: {"p", "exp_avg", "exp_avg_sq", "norm", "steps"}
    ("steps": 0 if exact, inf otherwise; "norm" only when given).  extra_p: per-tensor terms added to the bound of p (where it is not 0)."""
    d = lambda a: np.asarray(a, np.float64)
    n = range(len(r.p))
    tp = r.tp if extra_p is None else [np.where(r.tp[i] > 0, r.tp[i] + extra_p[i], 0.0) for i in n]
    out = {"p": _nanmax(_worst(np.abs(d(p[i]) - r.p[i]), tp[i]) for i in n),
           "exp_avg": _nanmax(_worst(np.abs(d(m[i]) - r.m[i]), r.tm[i]) for i in n),
           "exp_avg_sq": _nanmax(_worst(np.abs(d(v[i]) - r.v[i]), r.tv[i]) for i in n),
           "steps": 0.0 if np.array_equal(np.asarray(steps, F), r.steps) else math.inf}
    if norm is not None:
        out["norm"] = _worst(abs(float(norm) - r.norm), r.tnorm)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
def T(numel, off=0, grad=True, group=0, step0=0, gmag=1.0, zero_grad=False):
    """One tensor of a case.  off: start in floats past a 16-byte boundary - one value for all four addresses or (p, g, m, v)."""
    off = (off,) * 4 if isinstance(off, int) else tuple(off)
    return types.SimpleNamespace(numel=numel, off=off, grad=grad, group=group, step0=step0, gmag=gmag, zero_grad=zero_grad)


STEPS0 = (0, 1, 9, 999, 100000)   # initial steps[] cycled over the tensors of the mixed cases: per-tensor bias corrections
GMAGS = (1e-8, 1e-3, 1.0, 1e3, 1e-5, 30.0)


def _mixed(numels, **kw):
    """Tensors of the given sizes with start offsets 0, 4, 8, 12 bytes, initial step counts and gradient magnitudes cycled."""
    return [T(n, off=i % 4, step0=STEPS0[i % 5], gmag=GMAGS[i % 6], **kw) for i, n in enumerate(numels)]


def _sizes(c):
    return [1, 3, 4, 5, c - 1, c, c + 1, 2 * c, 3 * c + 7]


def _regroup(ts, groups):
    for t, gi in zip(ts, groups):
        t.group = gi
    return ts


# name -> (reason, dict of: chunk, tensors, lr, wd, betas, eps, clip, grad_scale, hyper_dev, calls)
# clip: ("off",) | ("value", max_norm) | ("boundary", k): max_norm = float32((total + 1e-6)(1 + k*u)) |
#       ("rescale", total, max_norm): the gradients are rescaled so that the norm is `total`
def _table():
    c = {}
    c["product_mix"] = ("chunk 4096 (the product value), every size around the vector width and the chunk, four start offsets, three "
                        "groups with lr 1e-5 and wd 0.05 / 1 (the multi-chunk tensors carry wd), per-tensor steps, magnitudes 1e-8..1e3, heavy clipping",
                        dict(chunk=4096, tensors=_regroup(_mixed(_sizes(4096)), [0, 0, 1, 0, 2, 0, 1, 2, 1]), lr=[1e-3, 1e-5, 1e-3],
                             wd=[0.0, 0.05, 1.0], clip=("value", 1.0)))
    c["chunk64_unclipped_third"] = ("chunk 64: fewer than one element per thread; norm far below max_norm, so coef is grad_scale = 1/3 exactly",
                                    dict(chunk=64, tensors=_mixed(_sizes(64)), lr=[1e-3], wd=[0.0], clip=("value", 1e9), grad_scale=1 / 3))
    c["chunk66_off_boundary"] = ("chunk 66: every odd chunk of an aligned tensor starts 8 bytes off a 16-byte boundary; norm three u below the clip boundary, grad_scale 1/8",
                                 dict(chunk=66, tensors=_regroup([T(n, step0=s, gmag=0.5) for n, s in zip(_sizes(66), STEPS0 + STEPS0)], [0, 1] * 5), lr=[1e-3, 1e-3],
                                      wd=[0.0, 0.05], clip=("boundary", 3), grad_scale=1 / 8))
    c["boundary_above"] = ("norm three u above the clip boundary: the other side of min(., 1)",
                           dict(chunk=4096, tensors=_mixed([5, 4097, 700]), lr=[1e-3], wd=[0.0], clip=("boundary", -3)))
    c["chunk16384_passes"] = ("chunk 16384: 16 vector iterations per thread, with tails; wd on multi-chunk tensors; grad_scale 1/3 under heavy clipping",
                              dict(chunk=16384, tensors=_regroup(_mixed([16383, 16384, 16385, 2 * 16384, 3 * 16384 + 7]), [0, 1, 0, 1, 1]),
                                   lr=[1e-3, 1e-3], wd=[0.0, 0.05], clip=("value", 1.0), grad_scale=1 / 3))
    c["one_address_misaligned"] = ("each of the four addresses alone forces the scalar path: only p, only the gradient, only exp_avg, only exp_avg_sq off a 16-byte boundary",
                                   dict(chunk=4096, tensors=[T(1000, off=(1, 0, 0, 0), step0=1), T(4096 + 500, off=(0, 2, 0, 0), step0=9), T(1000, off=(0, 0, 3, 0)),
                                                             T(4096 + 500, off=(0, 0, 0, 1), step0=999), T(1000, off=0, step0=1)], lr=[1e-3], wd=[0.0], clip=("value", 1.0)))
    c["one_chunk"] = ("nchunks = 1: a single workgroup; clipping off (max_norm = 0), so m' from m = 0 is one product",
                      dict(chunk=4096, tensors=[T(100)], lr=[1e-3], wd=[0.0], clip=("off",)))
    c["zeros"] = ("clipping off: an all-zero gradient on zero moments (bitwise no-op) and one on live moments (pure decay), planted zeros elsewhere",
                  dict(chunk=64, tensors=[T(70, zero_grad=True), T(130, zero_grad=True, step0=9), T(65, step0=1), T(5)], lr=[1e-3], wd=[0.0], clip=("off",)))
    c["chunks_256"] = ("exactly 256 chunks: one full pass of the strided fp64 sum", dict(chunk=64, tensors=[T(256 * 64, step0=1)], lr=[1e-3], wd=[0.0], clip=("value", 1.0)))
    c["chunks_257"] = ("257 chunks: one partial into the second pass, and a one-element last chunk",
                       dict(chunk=64, tensors=[T(256 * 64 + 1, step0=1)], lr=[1e-3], wd=[0.0], clip=("value", 1.0)))
    c["chunks_600"] = ("600 chunks over two tensors: the strided sum and the tree at a non-power-of-two",
                       dict(chunk=64, tensors=[T(38000, step0=9, off=1), T(391, off=2)], lr=[1e-3], wd=[0.05], clip=("value", 1.0)))
    c["no_gradient"] = ("first, middle and last tensor without a gradient, the middle one multi-chunk: untouched bitwise, step counts unchanged",
                        dict(chunk=64, tensors=[T(7, grad=False, step0=9), T(100, step0=1), T(64 * 3 + 5, grad=False, step0=999), T(66), T(64, grad=False, step0=1)],
                             lr=[1e-3], wd=[0.05], clip=("value", 1.0)))
    c["groups_128"] = ("the maximum of 128 groups, index 127 in use", dict(chunk=4096, tensors=[T(50, group=0), T(4100, group=127, step0=9), T(9, group=64, step0=1)],
                                                                          lr=[1e-3] + [7e-4] * 63 + [2e-3] + [7e-4] * 62 + [1e-5],
                                                                          wd=[0.0] * 64 + [1.0] + [0.0] * 62 + [0.05], clip=("value", 1.0)))
    c["hyper_dev"] = ("lr and wd read from device memory; the host arrays hold NaN, which proves they are not read",
                      dict(chunk=4096, tensors=_regroup(_mixed([33, 4097, 600]), [0, 1, 2]), lr=[1e-3, 1e-5, 2e-3], wd=[0.0, 0.05, 1.0], clip=("value", 1.0),
                           hyper_dev=True))
    c["eps_1e-3"] = ("eps = 1e-3 at small step counts: its place after the square root and after the bias correction is visible",
                     dict(chunk=64, tensors=[T(100, step0=s, gmag=g) for s, g in ((0, 1e-2), (1, 1e-3), (9, 1.0), (999, 1e-2))], lr=[1e-3], wd=[0.0], eps=1e-3,
                          clip=("off",)))
    c["betas_distant"] = ("betas (0.5, 0.9): nothing is tied to the product pair", dict(chunk=64, tensors=_mixed([5, 65, 200]), lr=[1e-3], wd=[0.05], betas=(0.5, 0.9),
                                                                                      clip=("value", 1.0)))
    c["clip_just_above_1e-3"] = ("norm 1.0005e-3 just above max_norm = 1e-3: the 1e-6 of the denominator is a relative 1e-3 of it",
                                 dict(chunk=64, tensors=[T(100, step0=1), T(300)], lr=[1e-3], wd=[0.0], clip=("rescale", 1.0005e-3, 1e-3)))
    c["tiny_gradients"] = ("clipping off, gradients of 1e-8: sqrt(v') after the bias correction is comparable with eps = 1e-8",
                           dict(chunk=64, tensors=[T(100, gmag=1e-8), T(70, gmag=3e-9, step0=999), T(65, gmag=1e-7, step0=9)], lr=[1e-3], wd=[0.0], clip=("off",)))
    c["three_steps"] = ("three consecutive calls, norm above / below / above max_norm; each call's reference starts from the kernel's own float32 state",
                        dict(chunk=64, tensors=_regroup(_mixed([5, 64, 65, 200]), [0, 1, 0, 1]), lr=[1e-3, 1e-5], wd=[0.0, 0.05], clip=("value", 1.0), calls=3))
    return c


TABLE = _table()
CASES = list(TABLE)


def make_case(name):
    """The inputs of a case: c.buf[role] float32 buffers with the tensors between sentinel bands (c.pos[role][i]: first float of tensor i;
    the gradient buffer of call k is c.grads[k]), c.numel, c.group, c.has_grad, c.steps0, c.h (hyper()), c.hyper_dev, c.chunk,
    c.chunk_tensor / c.chunk_offset, c.calls.  Element numel//2 of every tensor of at least 2 elements has g = m = v = 0 planted."""
    reason, s = TABLE[name]
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)
    ts = s["tensors"]
    c = types.SimpleNamespace(name=name, reason=reason, chunk=s["chunk"], calls=s.get("calls", 1), hyper_dev=s.get("hyper_dev", False),
                              numel=[t.numel for t in ts], group=[t.group for t in ts], has_grad=[t.grad for t in ts],
                              steps0=np.array([t.step0 for t in ts], F), pos={}, buf={})
    for k, role in enumerate(ROLES):
        cur, pos = BAND, []
        for t in ts:
            start = (cur + 3) // 4 * 4 + t.off[k]
            pos.append(start)
            cur = start + t.numel + BAND
        c.pos[role] = pos
        c.buf[role] = np.full(cur, SENTINEL, F)
    c.grads = [np.array(c.buf["g"]) for _ in range(c.calls)]
    for i, t in enumerate(ts):
        sl = lambda role: slice(c.pos[role][i], c.pos[role][i] + t.numel)
        c.buf["p"][sl("p")] = rng.randn(t.numel)
        live = t.step0 > 0
        c.buf["m"][sl("m")] = rng.randn(t.numel) * t.gmag * 0.3 if live else 0.0
        c.buf["v"][sl("v")] = (rng.randn(t.numel) * t.gmag) ** 2 * 0.5 + (0.01 * t.gmag) ** 2 if live else 0.0
        for k in range(c.calls):
            g = rng.randn(t.numel) * t.gmag * (1.0 if k % 2 == 0 else 1e-5)
            c.grads[k][sl("g")] = 0.0 if t.zero_grad else g
        if t.numel >= 2:
            z = t.numel // 2
            c.buf["m"][c.pos["m"][i] + z] = c.buf["v"][c.pos["v"][i] + z] = 0.0
            for k in range(c.calls):
                c.grads[k][c.pos["g"][i] + z] = 0.0
    b1, b2 = s.get("betas", (0.9, 0.999))
    gs = F(s.get("grad_scale", 1.0))
    clip = s["clip"]
    if clip[0] == "rescale":
        for k in range(c.calls):
            f = clip[1] / total_norm(tensors_of(c, {"g": c.grads[k]}, "g"), gs)
            for i, t in enumerate(ts):
                c.grads[k][c.pos["g"][i]:c.pos["g"][i] + t.numel] *= F(f)
    total = total_norm(tensors_of(c, {"g": c.grads[0]}, "g"), gs)
    mx = {"off": lambda: 0.0, "value": lambda: clip[1], "rescale": lambda: clip[2],
          "boundary": lambda: float(F((total + 1e-6) * (1 + clip[1] * U)))}[clip[0]]()
    c.h = hyper(s["lr"], s["wd"], b1, b2, s.get("eps", 1e-8), mx, gs)
    c.buf["g"] = c.grads[0]
    c.chunk_tensor = [i for i, n in enumerate(c.numel) for _ in range(0, n, c.chunk)]
    c.chunk_offset = [o for n in c.numel for o in range(0, n, c.chunk)]
    for role in ROLES:  # nothing subnormal is planted
        a = np.abs(c.buf[role])
        assert not ((a > 0) & (a < FLT_MIN)).any()
    return c


def tensors_of(c, bufs, role, grad_mask=False):
    """Per-tensor views of a role's buffer (with grad_mask: None for the tensors without a gradient)."""
    return [None if (grad_mask and not c.has_grad[i]) else bufs[role][c.pos[role][i]:c.pos[role][i] + n] for i, n in enumerate(c.numel)]


def case_reference(c, bufs, steps, **kw):
    """reference() of one call of case `c` from the float32 state `bufs` (role -> buffer) and `steps`."""
    return reference(tensors_of(c, bufs, "p"), tensors_of(c, bufs, "g", True), tensors_of(c, bufs, "m"), tensors_of(c, bufs, "v"),
                     steps, c.group, c.h, c.chunk, **kw)


def case_ratios(c, r, bufs, steps, norm=None):
    return ratios(r, tensors_of(c, bufs, "p"), tensors_of(c, bufs, "m"), tensors_of(c, bufs, "v"), steps, norm)


def bands_untouched(c, bufs):
    """True when every float outside the tensors still holds the sentinel, bit for bit, in all four buffers."""
    for role in ROLES:
        band = np.ones(bufs[role].shape, bool)
        for i, n in enumerate(c.numel):
            band[c.pos[role][i]:c.pos[role][i] + n] = False
        if not (bufs[role][band].view(np.uint32) == SENTINEL.view(np.uint32)).all():
            return False
    return True
