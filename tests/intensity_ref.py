"""Float64 reference, per-pixel error bound and case tables of the fused intensity augmentation (csrc/intensity.hip,
ttk_intensity_augment): equalize -> posterize -> gamma -> contrast -> brightness -> 5x5 Gaussian blur -> + noise -> clip -> + out_shift.
CPU only; tests/test_intensity_ref.py pins it without a GPU, tests/test_intensity_rows_gpu.py judges the kernel by it.

REFERENCE.  kornia's published formulas (enhance.equalize / _scale_channel, posterize, adjust_gamma, adjust_contrast, adjust_brightness,
filters.gaussian_blur2d with border_type="reflect", RandomGaussianNoise) restated in torch float64, in the order of the reference's
container.  The float32 inputs (image, parameters, noise) are exact in float64; everything after them is float64.  Three steps quantise,
and they are integer decisions, not arithmetic:
  * the histogram bin: 256 bins over [0, 255], bin = floor(q 256 / 255), the maximum in the last bin, values outside ignored;
  * the LUT index trunc(q) (`im.long()`) and posterize's trunc(q);
  * `step`, `lut` and the shift by one bin: integer arithmetic.
q = fl32(x 255) is the ONE float32 product kornia and the kernel both form (an IEEE multiplication: every float32 implementation holds
the same q); the decisions are taken on it in real arithmetic.  A decision is UNDECIDED where its argument lies within 4 ulp (float32) of
an integer / a bin edge without lying on it: there another rounding of the same expression could decide otherwise.  An argument ON the
integer or edge is decided by real arithmetic: the loader's lattice k/256 has q 256/255 = k exactly (torch.histc forms (q 256) / 255,
exact; the kernel's q fl32(256/255) lands in the same bin since fl32(256/255) > 256/255), and a level L/255 has fl32(fl32(L/255) 255) = L
for every L.  tests/test_intensity_ref.py asserts both facts for all 256 values, and that NO pixel of any case is undecided: a condition
on the inputs, not a tolerance.

BOUND.  Beside the float64 value v runs e, a bound on |kernel - v| counted from the kernel's float32 roundings, u = 2^-24:
  LUT or posterize level L/255      u v                                   one rounding (the level itself is an integer decision)
  equalize with step == 0           |fl32(fl32(x 255) / 255) - x|         kornia's round trip against the kernel's untouched x: 0 on the lattices
  gamma                             max |(v +- e)^g - v^g| (v - e clamped at 0) + P u v^g, P = P_POWF
  contrast                          c e + u c v
  brightness                        e + u (|b - 1| + |v + b - 1|)         fl(b - 1), then the sum
  each blur pass                    blur(e) + (K_W + 5) u blur(|v|)       the weights' error and five fma roundings
  noise                             e + u (|s n| + |v|)
  clip                              e                                     1-Lipschitz
  shift                             e + u |v + shift|                     one rounding of the sum
CRITERION: |x - f64| <= 4 e + 2^-24 |f64| on every pixel of every case, none left out (where the right side is 0, x == 0 exactly).
Bitwise rules beside it: where the value is an exact level and nothing but clip and shift follows, x == fl32(fl32(L) / fl32(255) + shift);
where equalize finds step == 0 (or no operation fires) and nothing follows, x == fl32(clip(input) + shift).
"""
import functools
from collections import namedtuple

import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24
EQ, BITS, GAMMA, CONTRAST, BRIGHT, BLUR, NOISE, SLOT7, NPARAMS = 0, 1, 2, 3, 4, 5, 6, 7, 8
SIGMA = 1.5
# powf of the device library: the HIP math documentation installed with the toolchain states no ulp figure, so the OpenCL bound the
# library is written to meet: 16 ulp, in the table's units (the factor of u v^g).  The measured figure is in profiles/intensity_float64.txt.
P_POWF = 16.0
# Relative error of a normalised weight g_k / sum(g), in units of u (first order, 1 ulp = 2 u):
#   numerator   expf within 3 ulp = 6 u, its argument -(k^2) / 4.5 one division: |arg| u <= 8/9 u < 1 u            ->  7
#   denominator five such terms (7) summed by four additions of positive numbers (u each)                           -> 11
#   one division                                                                                                    ->  1
K_W = 19.0
MARGIN = 4.0
LDS_FLOATS = (160 * 1024 - 64) // 4  # the launcher admits 2 HW + 512 floats <= this: HW <= 20 216


def max_pixels():
    return (LDS_FLOATS - 512) // 2


# ---------------------------------------------------------------------------------------------------------------------------------
# the decisions
# ---------------------------------------------------------------------------------------------------------------------------------
def near(t, ulps=4.0):
    """within `ulps` ulp (float32, taken at the integer: >= the ulp of t) of an integer without lying on it"""
    r = torch.round(t)
    d = (t - r).abs()
    return (d > 0) & (d <= ulps * 2.0 ** -23 * r.abs().clamp(min=1.0))


def product255(x32):
    """q = fl32(x 255) as float64: the one rounding the reference and every float32 implementation share"""
    return (x32 * 255.0).double()


def decide_index(q, ulps=4.0):
    """trunc(q) clamped to 0..255 (im.long(), posterize) -> (index, undecided)"""
    return torch.trunc(q).clamp(0, 255).long(), near(q, ulps)


def decide_bin(q, ulps=4.0):
    """torch.histc(bins=256, min=0, max=255) -> (bin, inside, undecided)"""
    inside = (q >= 0) & (q <= 255)
    t = q * 256.0 / 255.0  # q 256 is exact, the quotient correctly rounded: an argument on an edge is on it here too
    b = torch.floor(t).clamp(0, 255).long()
    ends = ((q != 0) & (q.abs() <= ulps * 2.0 ** -23)) | ((q != 255) & ((q - 255.0).abs() <= ulps * 2.0 ** -23 * 255.0))  # in or out
    return b, inside, (inside & near(t, ulps)) | ends


def equalize_levels(x32, ulps=4.0):
    """the integer path of _scale_channel -> (levels or None where step == 0, undecided, info)"""
    q = product255(x32)
    b, inside, und_b = decide_bin(q, ulps)
    hist = torch.bincount(b[inside].flatten(), minlength=256)
    nz = hist[hist != 0]
    step = int((nz.sum() - nz[-1]) // 255) if nz.numel() else 0
    info = dict(step=step, rest=int(nz.sum() - nz[-1]) if nz.numel() else 0, lut_max=0)
    if step == 0:
        return None, und_b, info
    raw = (torch.cumsum(hist, 0) + step // 2) // step
    raw = torch.cat([torch.zeros(1, dtype=torch.long), raw[:-1]])  # shifted by one bin
    info["lut_max"] = int(raw.max())
    idx, und_i = decide_index(q, ulps)
    return raw.clamp(0, 255)[idx], und_b | und_i, info


# ---------------------------------------------------------------------------------------------------------------------------------
# the stages: (v, e) -> (v, e) in float64
# ---------------------------------------------------------------------------------------------------------------------------------
def level_stage(level):
    v = level.double() / 255.0
    return v, U * v


def gamma_stage(v, e, g):
    w = v ** g
    spread = torch.maximum(((v + e) ** g - w).abs(), ((v - e).clamp(min=0) ** g - w).abs())
    return w.clamp(0, 1), spread + P_POWF * U * w


def contrast_stage(v, e, c):
    return (v * c).clamp(0, 1), c * e + U * c * v.abs()


def brightness_stage(v, e, b):
    return (v + (b - 1.0)).clamp(0, 1), e + U * (abs(b - 1.0) + (v + (b - 1.0)).abs())


def weights64(sigma=SIGMA):
    k = torch.arange(-2, 3, dtype=torch.float64)
    g = torch.exp(-k * k / (2.0 * sigma * sigma))
    return g / g.sum()


def _reflect(i, n):
    i = i.abs()
    return torch.where(i >= n, 2 * n - 2 - i, i)


def blur_pass(v, axis):
    """one 5-tap pass along `axis` of an [H, W] float64 image, border "reflect" (-1 -> 1, n -> n - 2)"""
    g, n = weights64(), v.shape[axis]
    taps = _reflect(torch.arange(n)[None, :] + torch.arange(-2, 3)[:, None], n)
    return sum(g[k] * v.index_select(axis, taps[k]) for k in range(5))


def blur_stage(v, e):
    for axis in (1, 0):  # along the rows first, as the kernel; the float64 value does not depend on the order
        e = blur_pass(e, axis) + (K_W + 5.0) * U * blur_pass(v.abs(), axis)
        v = blur_pass(v, axis)
    return v, e


def noise_stage(v, e, s, n):
    return v + s * n, e + U * ((s * n).abs() + v.abs())


def shift_stage(v, e, shift):
    v = v.clamp(0, 1)
    return v + shift, e + (U * (v + shift).abs() if shift != 0.0 else 0.0)


Ref = namedtuple("Ref", "v e undecided exact info")  # v, e float64 [H, W] before clip + shift; exact: float32 before clip + shift or None


def reference_image(x, p, noise, ulps=4.0):
    """x [H, W] float32, p the eight float32 parameters, noise [H, W] float32 or None -> Ref (before clip and shift)"""
    x32 = torch.from_numpy(np.array(x, dtype=F32))
    p = [float(F32(a)) if np.isfinite(a) else a for a in p]
    v, e = x32.double(), torch.zeros(x32.shape, dtype=torch.float64)
    und = torch.zeros(x32.shape, dtype=torch.bool)
    level, info = None, dict(step=None)
    exact = x32.clone()  # nothing fired yet: the input itself
    bits = int(p[BITS])
    quantising = p[EQ] > 0 or 0 < bits < 8
    if quantising:
        assert float(x32.min()) >= 0.0 and float(x32.max()) <= 1.0, "the quantising steps are defined for images in [0, 1]"
    if p[EQ] > 0:
        level, u, info = equalize_levels(x32, ulps)
        und |= u
        if level is None:
            e = (((x32 * 255.0) / 255.0).double() - v).abs()
            if float(e.max()) > 0:
                exact = None
    if 0 < bits < 8:
        if level is None:
            level, u = decide_index(product255(x32), ulps)
            und |= u
        level = (level >> (8 - bits)) << (8 - bits)
    if level is not None:
        v, e = level_stage(level)
        exact = level.float() / torch.tensor(255.0, dtype=torch.float32)
    if p[GAMMA] > 0:
        assert float(v.min()) >= 0.0
        v, e = gamma_stage(v, e, p[GAMMA])
    if p[CONTRAST] > 0:
        v, e = contrast_stage(v, e, p[CONTRAST])
    if p[BRIGHT] > 0:
        v, e = brightness_stage(v, e, p[BRIGHT])
    if p[BLUR] > 0:
        v, e = blur_stage(v, e)
    noisy = noise is not None and p[NOISE] > 0
    if noisy:
        v, e = noise_stage(v, e, p[NOISE], torch.from_numpy(np.array(noise, dtype=F32)).double())
    if p[GAMMA] > 0 or p[CONTRAST] > 0 or p[BRIGHT] > 0 or p[BLUR] > 0 or noisy:
        exact = None
    return Ref(v, e, und, exact, info)


def finish(ref, shift):
    """clip and shift -> (f64, e, exact float32 output or None)"""
    v, e = shift_stage(ref.v, ref.e, float(shift))
    exact = None if ref.exact is None else (ref.exact.clamp(0, 1) + torch.tensor(shift, dtype=torch.float32)).numpy()
    return v.numpy(), e.numpy(), exact


def ratios(got, f64, e):
    """|x - f64| / (4 e + 2^-24 |f64|) per pixel; where the allowance is 0 the value must be exactly f64"""
    got = np.asarray(got, np.float64)
    allow = MARGIN * e + U * np.abs(f64)
    err = np.abs(got - f64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(allow > 0, err / allow, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(got), r, np.inf)


# ---------------------------------------------------------------------------------------------------------------------------------
# images: every one chosen so that no decision is undecided
# ---------------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def arbitrary(rng, H, W):
    """floats off both lattices, 8 ulp and more clear of every integer and every bin edge of q = x 255 by construction: q inside
    (j, e_j) or (e_j, j + 1), e_j = (j + 1) 255 / 256 the one bin edge between j and j + 1, a fifth of the interval away from its ends
    (the narrowest, (254, 254.0039), leaves 7.8e-4 = 51 ulp)"""
    j = rng.integers(0, 255, (H, W)).astype(np.float64)
    f = rng.uniform(0.2, 0.8, (H, W))
    edge = (j + 1.0) * 255.0 / 256.0
    upper = (j >= 64) & (rng.random((H, W)) < 0.5)
    q = np.where(upper, edge + f * (j + 1.0 - edge), j + f * (edge - j))
    return (q / 255.0).astype(F32)


def planted(rng, H, W, rest, denom=256.0, top=250):
    """`rest` pixels on levels below `top`, all others on `top`, the last non-empty bin: HW - last == rest"""
    k = np.full(H * W, top, np.int64)
    pos = rng.permutation(H * W)[:rest]
    k[pos] = (np.arange(rest) * 7) % 200
    return (k.astype(F32) / F32(denom)).reshape(H, W)


def image(kind, H, W, seed):
    rng = _rng(_seed(kind), H, W, seed)
    u8 = rng.integers(0, 256, (H, W))
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if kind == "u256":  # what the loader hands over: u8 / 256
        return u8.astype(F32) / F32(256.0)
    if kind == "u255":
        return u8.astype(F32) / F32(255.0)
    if kind == "arb":
        return arbitrary(rng, H, W)
    if kind == "smooth":  # a textured gradient on the loader's lattice: rows and columns differ
        k = (96 + 60 * np.sin(0.31 * cc + 0.13 * rr) + 50 * np.cos(0.07 * cc - 0.23 * rr) + rng.integers(0, 24, (H, W))).astype(np.int64)
        return np.clip(k, 0, 255).astype(F32) / F32(256.0)
    if kind == "zero":
        return np.zeros((H, W), F32)
    if kind == "one":
        return np.ones((H, W), F32)
    if kind == "flat":
        return np.full((H, W), 0.25, F32)
    if kind == "two":  # two levels, the split neither along rows nor along columns
        return np.where((rr * 3 + cc * 5) % 7 < 3, F32(192.0 / 256.0), F32(64.0 / 256.0)).astype(F32)
    if kind == "ramp":  # every level in turn
        return ((rr * W + cc) % 256).astype(F32) / F32(255.0)
    if kind == "block1":  # a 4 x 4 block (as much of it as fits) of exactly 1.0: the last bin
        im = u8.astype(F32) / F32(256.0)
        im[:4, :4] = 1.0
        return im
    if kind == "step0":
        return planted(rng, H, W, min(254, H * W - 1))
    if kind == "step1":
        return planted(rng, H, W, min(255, H * W - 1))
    if kind == "saturate":  # (HW - last) = 255 step + r with r + step // 2 >= step: the last LUT entry passes 255 and is clamped
        rest = H * W - max(1, H * W // 15)
        step = rest // 255
        while step and rest % 255 + step // 2 < step:
            rest -= 1
            step = rest // 255
        return planted(rng, H, W, rest, 255.0, top=255)
    if kind == "over":  # past 1.0, for the clamp after gamma: no quantising step may see it
        return rng.integers(0, 193, (H, W)).astype(F32) / F32(128.0)
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------------------------------------
# parameters and the tables of cases
# ---------------------------------------------------------------------------------------------------------------------------------
def prm(eq=0.0, bits=0.0, gamma=0.0, contrast=0.0, bright=0.0, blur=0.0, noise=0.0, slot7=0.0):
    return [eq, bits, gamma, contrast, bright, blur, noise, slot7]


CHAIN = ("eq", "post", "gamma", "contrast", "bright", "blur", "noise")
ALONE = dict(eq=prm(eq=1), post=prm(bits=4), gamma=prm(gamma=0.5), contrast=prm(contrast=1.5), bright=prm(bright=0.7), blur=prm(blur=1),
             noise=prm(noise=4 / 255))
PAIRS = {"eq+post": prm(eq=1, bits=1), "post+gamma": prm(bits=7, gamma=2.0), "gamma+contrast": prm(gamma=0.5, contrast=0.7),
         "contrast+bright": prm(contrast=1.5, bright=1.5), "bright+blur": prm(bright=0.7, blur=1), "blur+noise": prm(blur=1, noise=64 / 255)}
FULL = prm(eq=1, bits=4, gamma=2.0, contrast=0.7, bright=1.5, blur=1, noise=64 / 255)
FULL2 = prm(eq=1, bits=7, gamma=0.5, contrast=1.5, bright=0.7, blur=1, noise=4 / 255)
NONE = prm()
KINDS = ("u256", "u255", "arb", "smooth")

Row = namedtuple("Row", "name kind prm")
Case = namedtuple("Case", "name H W rows")
SHIFTS = (0.0, -0.5)


def standard_rows(offset=0):
    """each operation alone, each adjacent pair in chain order, the full chain twice, nothing: 16 images, the image families in turn"""
    table = [(k, ALONE[k]) for k in CHAIN] + list(PAIRS.items()) + [("full", FULL), ("full2", FULL2), ("none", NONE)]
    return [Row(n, KINDS[(i + offset) % len(KINDS)], p) for i, (n, p) in enumerate(table)]


SHAPES = [(3, 3), (3, 64), (64, 3), (5, 51), (16, 16), (3, 86), (31, 47), (47, 31), (129, 129), (142, 142), (141, 143)]
SPECIAL = ("zero", "one", "flat", "two", "ramp", "block1", "step0", "step1", "saturate")


def _special_rows():
    rows = []
    for k in SPECIAL:
        rows += [Row("eq", k, ALONE["eq"]), Row("eq+post+blur", k, prm(eq=1, bits=4, blur=1)), Row("full", k, FULL)]
    return rows


def _edge_rows():
    rows = [Row(f"bits{b}", "u255" if b % 2 else "u256", prm(bits=b)) for b in (0, 1, 4, 7, 8, 9)]
    rows += [Row(f"bits{b}arb", "arb", prm(bits=b)) for b in (1, 7)]
    rows += [Row(f"gamma{g}", k, prm(gamma=g)) for g, k in ((0.5, "u256"), (1.0, "u255"), (2.0, "arb"), (0.5, "zero"), (2.0, "one"))]
    rows += [Row(f"contrast{c}", "u256", prm(contrast=c)) for c in (0.7, 1.5)]
    rows += [Row(f"bright{b}", "u255", prm(bright=b)) for b in (0.7, 1.5)]
    rows += [Row(f"noise{s}", "smooth", prm(noise=s / 255)) for s in (4, 64)]
    rows += [Row("blur", k, prm(blur=1)) for k in ("zero", "one", "flat", "arb")]
    rows += [Row("gamma+contrast over 1", "over", prm(gamma=2.0, contrast=0.7)), Row("eq arb", "arb", ALONE["eq"]),
             Row("eq+post arb", "arb", prm(eq=1, bits=4))]
    return rows


def _batch_rows(n):
    base = standard_rows() + _special_rows()
    return [base[(i * 7) % len(base)] for i in range(n)]


CASES = {f"{h}x{w}": Case(f"{h}x{w}", h, w, standard_rows(i)) for i, (h, w) in enumerate(SHAPES)}
CASES.update({
    "special16x16": Case("special16x16", 16, 16, _special_rows()),
    "special31x47": Case("special31x47", 31, 47, _special_rows()),
    "edges31x47": Case("edges31x47", 31, 47, _edge_rows()),
    "edges47x31": Case("edges47x31", 47, 31, _edge_rows()),
    "b1": Case("b1", 31, 47, [Row("full", "u256", FULL)]),
    "b2": Case("b2", 47, 31, [Row("full2", "smooth", FULL2), Row("eq", "u255", ALONE["eq"])]),
    "b300": Case("b300", 16, 16, _batch_rows(300)),  # more workgroups than the device has compute units
})
CASE_NAMES = list(CASES)
REFUSED = [(143, 142), (2, 5), (5, 2)]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(x [B, H, W], params [B, 8], noise [B, H, W]) float32 of a case; read-only"""
    c = CASES[name]
    x = np.stack([image(r.kind, c.H, c.W, i) for i, r in enumerate(c.rows)]).astype(F32)
    p = np.array([r.prm for r in c.rows], F32)
    n = _rng(_seed(name), 77).standard_normal(x.shape).astype(F32)
    for a in (x, p, n):
        a.setflags(write=False)
    return x, p, n


@functools.lru_cache(maxsize=None)
def reference(name):
    """the Ref of every image of a case (before clip and shift); computed once and shared"""
    x, p, n = inputs(name)
    return tuple(reference_image(x[i], p[i], n[i]) for i in range(x.shape[0]))


def judge(name, got, shift):
    """worst ratio per image of `got` [B, H, W] (the criterion asks <= 1) and the images that break a bitwise rule"""
    worst, broken = [], []
    for i, ref in enumerate(reference(name)):
        f64, e, exact = finish(ref, shift)
        worst.append(float(ratios(got[i], f64, e).max()))
        if exact is not None and not np.array_equal(np.asarray(got[i], F32).view(np.int32), exact.view(np.int32)):
            broken.append(i)
    return np.array(worst), broken


def active_ops(p, noise=True):
    bits = int(p[BITS])
    on = [p[EQ] > 0, 0 < bits < 8, p[GAMMA] > 0, p[CONTRAST] > 0, p[BRIGHT] > 0, p[BLUR] > 0, noise and p[NOISE] > 0]
    return tuple(n for n, f in zip(CHAIN, on) if f)


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 emulation of the kernel's arithmetic, with the planted errors of tests/test_intensity_ref.py
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("edge_repeat", "symmetric", "corners", "swap_hw", "bin_floor", "lut_unshifted", "step_total", "post_round", "post_low",
             "bright_mul", "contrast_mean", "no_clamp", "noise_first", "shift_first", "sigma1", "unnormalised", "neighbour")


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _emu_equalize(v, mut):
    s = v * F32(255.0)
    inside = (s >= 0) & (s <= 255)
    t = s[inside] if mut == "bin_floor" else s[inside] * F32(F32(256.0) / F32(255.0))
    hist = np.bincount(np.minimum(t.astype(np.int64), 255).ravel(), minlength=256)
    nz = hist[hist != 0]
    step = (int(nz.sum()) - (0 if mut == "step_total" else int(nz[-1]))) // 255 if nz.size else 0
    if step == 0:
        return v
    lut = (np.cumsum(hist) + step // 2) // step
    if mut != "lut_unshifted":
        lut = np.concatenate([[0], lut[:-1]])
    lut = np.clip(lut, 0, 255)
    return lut[np.clip(s.astype(np.int64), 0, 255)].astype(F32) / F32(255.0)


def _emu_blur(v, mut):
    H, W = v.shape
    if mut == "swap_hw":  # r = i / H, c = i - r H: the buffer walked as a W x H image
        return _emu_blur(v.reshape(W, H), None).reshape(H, W)
    k = np.arange(5) - 2
    g = np.exp(-(k * k).astype(F32) / F32(2.0 * (1.0 if mut == "sigma1" else SIGMA) ** 2)).astype(F32)
    if mut != "unnormalised":
        g = g / g.sum(dtype=F32)

    def idx(i, n):
        if mut in ("edge_repeat", "corner_source"):
            return np.clip(i, 0, n - 1)
        if mut == "symmetric":  # -1 -> 0, n -> n - 1
            i = np.where(i < 0, -1 - i, i)
            return np.where(i >= n, 2 * n - 1 - i, i)
        i = np.abs(i)
        return np.where(i >= n, 2 * n - 2 - i, i)

    cols, rows = idx(np.arange(W)[None, :] + k[:, None], W), idx(np.arange(H)[None, :] + k[:, None], H)
    tmp = np.zeros_like(v)
    for t in range(5):
        tmp = _fma(np.broadcast_to(g[t], v.shape), v[:, cols[t]], tmp)
    out = np.zeros_like(v)
    for t in range(5):
        out = _fma(np.broadcast_to(g[t], v.shape), tmp[rows[t], :], out)
    if mut == "corners":  # the four corners only: what an edge-repeating border gives there
        wrong = _emu_blur(v, "corner_source")
        for r in (0, -1):
            for c in (0, -1):
                out[r, c] = wrong[r, c]
    return out


def emulate(x, params, noise, shift=0.0, mut=None):
    """the kernel's chain in numpy float32, operation by operation in its order; `mut` plants one of MUTATIONS"""
    assert mut is None or mut in MUTATIONS
    shift = F32(shift)
    out = np.empty(x.shape, F32)
    clip = lambda a: np.clip(a, F32(0), F32(1)).astype(F32)
    for n in range(x.shape[0]):
        p, v = params[n], x[n].astype(F32)
        bits = int(p[BITS])
        if p[EQ] > 0:
            v = _emu_equalize(v, mut)
        if 0 < bits < 8:
            s = v * F32(255.0)
            u = np.clip(np.rint(s).astype(np.int64) if mut == "post_round" else s.astype(np.int64), 0, 255)
            u = (u & ((1 << (8 - bits)) - 1)) if mut == "post_low" else (u >> (8 - bits)) << (8 - bits)
            v = u.astype(F32) / F32(255.0)
        if p[GAMMA] > 0:
            v = np.power(v, F32(p[GAMMA]), dtype=F32)
            v = v if mut == "no_clamp" else clip(v)
        if p[CONTRAST] > 0:
            m = v.mean(dtype=np.float64).astype(F32)
            v = clip((v - m) * F32(p[CONTRAST]) + m) if mut == "contrast_mean" else clip(v * F32(p[CONTRAST]))
        if p[BRIGHT] > 0:
            v = clip(v * F32(p[BRIGHT])) if mut == "bright_mul" else clip(v + (F32(p[BRIGHT]) - F32(1.0)))
        noisy = noise is not None and p[NOISE] > 0
        add = lambda a: _fma(np.broadcast_to(F32(p[NOISE]), a.shape), noise[n].astype(F32), a)
        if noisy and mut == "noise_first":
            v = add(v)
        if p[BLUR] > 0:
            v = _emu_blur(v, mut)
        if noisy and mut != "noise_first":
            v = add(v)
        out[n] = clip(v + shift) if mut == "shift_first" else clip(v) + shift
    if mut == "neighbour":  # one pixel of every 256 read from the next image of the batch
        flat = out.reshape(out.shape[0], -1)
        flat[:, 255::256] = np.roll(flat, -1, axis=0)[:, 255::256]
    return out
