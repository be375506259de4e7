"""Float64 reference, yardstick, cases and restated launch arithmetic of the 5x5 / stride 2 / pad 2 stem, 1 -> 32 channels (csrc/stem.hip:
stem_fwd_band_k, stem_fwd_mfma_k, stem_wgrad_mfma_k, each in fp32 and bf16 storage).  Plain numpy on the CPU, built on tests/conv_ref.py
(im2col, the fp32 fma chain, Product); tests/test_stem_rows_gpu.py compares the kernels with it through the C ABI, tests/test_stem_ref.py
pins it on its own without a GPU.

Reference.  X = im2col(x)[M][25] (padded taps are zeros), in float64 of the float32 inputs:
    y  = X @ w^T                 [M][32], M = B * Ho * Wo, Ho = (H + 1) // 2
    dw = dy^T @ X                [32][25], contraction over the M output pixels;  dy = ga*(g - gmean) + gb*(y - mean)
with the per-element scale s = sum |a| |b| over the contraction; for dy the term bound D of conv_ref.dy_terms stands in for |dy| (the
device rounds every term of dy, their cancellation is not the kernels' error).

Yardstick.  The kernels are true fp32 MFMAs (v_mfma_f32_32x32x2_f32): conv_ref.chain32 - one float32 fma per contraction step - on the
case's own matrices is the whole yardstick, Y = max |chain32 - f64| / s; there is no split and no range floor.  For the weight gradient
the chain is the sequential sum over all M pixels, the pessimistic order: the kernel sums per workgroup and then atomically (or folds).

Criterion, for every element:      |x - f64| <= (MARGIN * Y + 2^-24) * s,      x == 0 exactly where s == 0
(MARGIN = 4 and its derivation: conv_ref.py).  With accumulate = 1 onto dw0 the reference is dw0 + dw and the scale gains |dw0|.

bf16 storage (act_bf16 = 3).  The weight gradient is GIVEN y and g already rounded to bf16 and exactly widened: its reference, scale and
yardstick are computed from those values, the criterion is unchanged.  The forward output is judged by a bracket, not a tolerance: with
allowed = (MARGIN * Y + 2^-24) * s the stored value v must satisfy
    rne_bf16(f64 - allowed) <= v <= rne_bf16(f64 + allowed),      v == +0 where s == 0.
The device stores rne_bf16(acc) of an fp32 accumulator acc within `allowed` of f64; rounding to nearest even is monotone, so is the
rounding of the float64 end points to float32 that rne_bf16 does first (acc is a float32: f32(lo) <= acc <= f32(hi)), hence the bracket
is exact and needs no fitted number.  The BatchNorm sums of this form are those of the values AS STORED (include/ttk.h).

Sums (`part`).  As tests/test_conv_rows_gpu.py::_check_forward_sums: column 0 against float64 of (y - pivot), absolute 3e-5 of the largest
channel's sum |y - pivot|; column 1 against float64 of (y - pivot)^2 and against the squares of the values the kernel stored, relative
3e-5.  y is the float64 reference in fp32 storage and the stored (bracketed) value in bf16 storage.  sums_outside() returns the worst
error / tolerance.

Launch arithmetic, restated from ttk_stem_fwd / ttk_stem_bwd_weight / stem_band_rows (facts()): which forward kernel a width takes, grids,
band heights and who gets a second band or tile.  Every CASE names the facts it is there for and tests/test_stem_ref.py asserts them.

Search (heights_search()): over B <= 1600, Ho <= 26 the weight-gradient band height takes every value 6..13 (and Ho below 6); the shapes
(B, 2 Ho - 1, 5) with the fewest input pixels that reach 11 and 13 are (385, 21, 5) and (513, 25, 5) - recorded in HEIGHT_CASES and
re-derived by the CPU test."""
import functools
import types

import numpy as np

from conv_ref import (BN_GA, BN_GB, BN_GMEAN, BN_MEAN, MARGIN, U, Product, bn_block, chain32, dy32_of, dy_terms,  # noqa: F401
                      gather_index, im2col)

C = 32
TAPS = 25
SUM_TOL = 3e-5            # tests/test_conv_rows_gpu.py::_check_forward_sums

# ---------------------------------------------------------------------------------------------------------------------------------
# the host's launch arithmetic (csrc/stem.hip), restated
# ---------------------------------------------------------------------------------------------------------------------------------
LDS_LIMIT = 64 * 1024     # what both entry points hold their DYNAMIC size to
BAND_MAX = 13             # kFwBand = kWgBand: staged rows = 2 * 13 + 3
WAVES = 4                 # kBlock / kWave
FWD_STATIC_LDS = WAVES * 2 * C * 4   # `red` of the forward kernels: 1 KB beside the dynamic size
MAX_PARTIAL_ROWS = 1024   # TTK_MAX_PARTIAL_ROWS_ELEMENTWISE
WGRAD_RESIDENT = 768      # persistent workgroups of the weight gradient


def out_hw(H, W):
    return (H + 1) // 2, (W + 1) // 2


def fwd_dynamic_lds(W):
    """bytes: the band [29][W + 4] rounded up to 16 bytes + four wave tiles [32][36]"""
    return ((((2 * BAND_MAX + 3) * (W + 4) + 3) & ~3) + WAVES * 32 * 36) * 4


def fwd_form(W):
    """the device accepts static + dynamic LDS above 64 KB (W = 394..402 launch and are correct: tests/test_stem_rows_gpu.py), so the
    host's test of the dynamic size alone stands"""
    return "band" if fwd_dynamic_lds(W) <= LDS_LIMIT else "gather"


def fwd_grid(B, Ho, Wo):
    """elementwise_grid(B * Ho * Wo * 8): one workgroup per 32 pixels, at most 1024; = the rows of `part`"""
    return int(min(max(-(-(B * Ho * Wo * (C // 4)) // 256), 1), MAX_PARTIAL_ROWS))


def fwd_band_rows(Ho):
    return min(BAND_MAX, Ho)


def fwd_bands(B, Ho):
    return B * -(-Ho // fwd_band_rows(Ho))


def wgrad_band_rows(B, Ho, grid=WGRAD_RESIDENT, max_rows=BAND_MAX):
    """stem_band_rows: the height in 6..13 (Ho below 6: Ho) with the least ceil(tiles / grid) * rows, the larger height on a tie"""
    best, best_cost = min(max_rows, Ho), None
    for r in range(min(max_rows, Ho), 5, -1):
        cost = -(-(B * -(-Ho // r)) // grid) * r
        if best_cost is None or cost < best_cost:
            best, best_cost = r, cost
    return best


def wgrad_tiles(B, Ho):
    return B * -(-Ho // wgrad_band_rows(B, Ho))


def wgrad_grid(B, Ho):
    return min(wgrad_tiles(B, Ho), WGRAD_RESIDENT)


def wgrad_lds(W):
    """bytes: the band [29][W] + per wave a dy chunk [32][32] and a fold tile [32][25]"""
    return ((2 * BAND_MAX + 3) * W + WAVES * (32 * C + C * TAPS)) * 4


def wgrad_fits(W):
    return wgrad_lds(W) <= LDS_LIMIT


def facts(B, H, W):
    """everything the host derives from a shape, by name"""
    Ho, Wo = out_hw(H, W)
    P = B * Ho * Wo
    f = dict(Ho=Ho, Wo=Wo, P=P, fwd_form=fwd_form(W), fwd_grid=fwd_grid(B, Ho, Wo), fwd_lds=fwd_dynamic_lds(W) + FWD_STATIC_LDS,
             wgrad_fits=wgrad_fits(W))
    if f["fwd_form"] == "band":
        rows, bands = fwd_band_rows(Ho), fwd_bands(B, Ho)
        f.update(fwd_bands=bands, fwd_band_heights=tuple([rows] * (Ho // rows) + ([Ho % rows] if Ho % rows else [])),
                 fwd_second_band=max(bands - f["fwd_grid"], 0),   # workgroups that stage a second band
                 fwd_idle=max(f["fwd_grid"] - bands, 0))          # workgroups without a band: their `part` row is zeros
    else:
        tiles = -(-P // 32)
        f.update(fwd_tiles=tiles, fwd_second_tile=max(tiles - WAVES * f["fwd_grid"], 0))  # waves that take a second tile
    if f["wgrad_fits"]:
        f.update(wgrad_rows=wgrad_band_rows(B, Ho), wgrad_tiles=wgrad_tiles(B, Ho), wgrad_grid=wgrad_grid(B, Ho),
                 wgrad_second_tile=max(wgrad_tiles(B, Ho) - wgrad_grid(B, Ho), 0))
    return f


def heights_search(max_B=1600, max_Ho=26):
    """{height: (B, H, 5) with the fewest input pixels B * H * 5, H = 2 Ho - 1, that the weight gradient runs at that height}"""
    best = {}
    for Ho in range(1, max_Ho + 1):
        for B in range(1, max_B + 1):
            r, px = wgrad_band_rows(B, Ho), B * (2 * Ho - 1) * 5
            if r not in best or px < best[r][0]:
                best[r] = (px, (B, 2 * Ho - 1, 5))
    return {r: shape for r, (px, shape) in best.items()}


HEIGHT_CASES = {11: (385, 21, 5), 13: (513, 25, 5)}  # heights_search()[11], [13]

# (shape, the facts the case is there for).  The smallest shape that reaches its path; figures from facts().
CASES = [
    # the training geometry: Ho = 65 = five forward bands of 13 per image, 255 idle forward workgroups; gradient height 6
    ((2, 129, 129), dict(fwd_form="band", fwd_band_heights=(13,) * 5, fwd_bands=10, fwd_idle=255, wgrad_rows=6, wgrad_tiles=22)),
    # odd / even sides, non-square
    ((3, 33, 33), dict(fwd_form="band", fwd_band_heights=(13, 4), wgrad_rows=6, wgrad_tiles=9)),
    ((2, 40, 50), dict(fwd_form="band", fwd_band_heights=(13, 7), wgrad_rows=6, wgrad_tiles=8)),
    ((5, 7, 9), dict(fwd_form="band", fwd_band_heights=(4,), wgrad_rows=4)),
    ((1, 5, 5), dict(Ho=3, Wo=3, fwd_band_heights=(3,), fwd_grid=1, wgrad_rows=3, wgrad_grid=1)),  # the smallest shape admitted
    # W even / odd against H: the last column and row of taps on or off the image; Wo = 3: the `wo += 2` wrap hits on every step
    ((2, 6, 5), dict(Ho=3, Wo=3, wgrad_rows=3)),
    ((2, 5, 6), dict(Ho=3, Wo=3, wgrad_rows=3)),
    # forward persistent loop: 40 bands on 32 workgroups, eight stage a second band
    ((40, 9, 9), dict(fwd_form="band", fwd_bands=40, fwd_grid=32, fwd_second_band=8)),
    # one image, bands of 13, 13 and 4 rows: the short last band behind a full one; two idle workgroups
    ((1, 60, 9), dict(fwd_form="band", fwd_band_heights=(13, 13, 4), fwd_bands=3, fwd_grid=5, fwd_idle=2)),
    # gradient persistent loop at a height above 6: 1538 tiles of 7 (and 6) rows on 768 workgroups
    ((769, 25, 5), dict(wgrad_rows=7, wgrad_tiles=1538, wgrad_grid=768, wgrad_second_tile=770)),
    # the further heights the search reaches (HEIGHT_CASES), each with one band per image
    ((385, 21, 5), dict(wgrad_rows=11, wgrad_tiles=385, wgrad_grid=385)),
    ((513, 25, 5), dict(wgrad_rows=13, wgrad_tiles=513, wgrad_grid=513)),
    # the widest gradient that fits
    ((1, 5, 313), dict(fwd_form="band", wgrad_fits=True, wgrad_rows=3)),
    # the edges of the forward LDS test: 393 the last width with static + dynamic <= 64 KB, 402 the last band width, 403 the first gather
    ((1, 5, 393), dict(fwd_form="band", fwd_lds=65520, wgrad_fits=False)),
    ((1, 5, 402), dict(fwd_form="band", fwd_lds=66560, wgrad_fits=False)),
    ((1, 5, 403), dict(fwd_form="gather", fwd_tiles=19, fwd_second_tile=0, wgrad_fits=False)),
    # gather kernel past 4096 tiles on the capped grid: waves take a second tile through the prefetch; forward only
    ((217, 5, 403), dict(fwd_form="gather", P=131502, fwd_grid=1024, fwd_tiles=4110, fwd_second_tile=14, wgrad_fits=False)),
]
SHAPES = [shape for shape, _ in CASES]
BF16_SHAPES = [(2, 129, 129), (5, 7, 9), (40, 9, 9), (769, 25, 5), (1, 5, 403)]
REFUSED_WIDTH = (1, 5, 314)  # one past the widest gradient


# ---------------------------------------------------------------------------------------------------------------------------------
# bfloat16 on the bit pattern
# ---------------------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """uint16 bits of x (finite) rounded to nearest even; x is rounded to float32 first (see the module docstring)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_widen(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def rne_bf16(x):
    return bf16_widen(bf16_bits(x))


def trunc_bf16(x):
    """the mutation: the low 16 bits dropped"""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def bracket(p):
    """(lo, hi) of the stored bf16 value per element, as float32"""
    a = p.allowed()
    return rne_bf16(p.ref - a), rne_bf16(p.ref + a)


def bracket_outside(p, v):
    """number of elements of the stored values v (float32, widened) outside the bracket, or not +0 where s == 0"""
    lo, hi = bracket(p)
    v = np.asarray(v, np.float32)
    bad = (v < lo) | (v > hi) | ~np.isfinite(v)
    zero = p.s == 0
    bad |= zero & (v.view(np.uint32) != 0)
    return int(bad.sum())


def bracket_ratio(p, v):
    """the RATIO figure of a bf16 output: per element the least |acc - f64| of any accumulator that rounds to the stored value v (the
    distance from f64 to v's rounding interval, half a bf16 step either side of v), as (d - 2^-24 s) / (s Y) like Product.ratio - what
    is printed; the bracket is what is asserted (the two agree up to the rounding of the bracket's end points, 2^-24 / Y)"""
    v = np.asarray(v, np.float32)
    live = p.s > 0
    if not live.any():
        return 0.0
    m = bf16_bits(np.abs(v)).astype(np.int32)
    mag = np.abs(v).astype(np.float64)
    up = bf16_widen((m + 1).astype(np.uint16)).astype(np.float64)
    down = bf16_widen(np.maximum(m - 1, 0).astype(np.uint16)).astype(np.float64)
    r = p.ref * np.where(np.signbit(v), -1.0, 1.0)
    d = np.maximum(np.maximum((mag + down) / 2 - r, r - (mag + up) / 2), 0.0)
    d = np.where(mag == 0, np.abs(p.ref), d)
    return float(((d - U * p.s)[live] / (p.s[live] * max(p.Y, 1e-300))).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# the case
# ---------------------------------------------------------------------------------------------------------------------------------
def patches(x):
    """X[M][25] of x[B][H][W]"""
    B, H, W = x.shape
    Ho, Wo = out_hw(H, W)
    return im2col(x.reshape(-1, 1), gather_index(B, H, W, Ho, Wo, 5, 2, False))


def wgrad_product(c, g, y):
    """the weight gradient GIVEN g and y (float32 [M][32]) with the case's bn and patches"""
    v = types.SimpleNamespace(bn=c.bn, g=g, y32=y)
    dy64, D = dy_terms(v)
    return Product(np.ascontiguousarray(dy32_of(g, y, c.bn).T), np.ascontiguousarray(dy64.T), np.ascontiguousarray(D.T), c.X)


@functools.lru_cache(maxsize=None)
def stem5_case(B, H, W, bf16=False):
    """conv_ref.stem_case at k = 5, pad = 2, stride = 2, C = 32 (never written afterwards).  A few input pixels are exactly zero, and
    one whole image when B > 1 (its outputs have s == 0).  bf16: g and the y the gradient is given are rounded to bf16 and widened.
    c.wgrad only where the gradient has a kernel (wgrad_fits)."""
    rng = np.random.default_rng(100003 * B + 1009 * H + W)
    c = types.SimpleNamespace(B=B, H=H, W=W, bf16=bf16)
    c.Ho, c.Wo = out_hw(H, W)
    c.M = B * c.Ho * c.Wo
    c.x = rng.uniform(-0.5, 0.5, (B, H, W)).astype(np.float32)
    n = c.x.size
    c.x.reshape(-1)[[1, n // 2, n - 2]] = 0.0
    if B > 1:
        c.x[B // 2] = 0.0
    c.w = (rng.normal(0, 1, (C, TAPS)) * 0.2).astype(np.float32)
    c.piv = rng.normal(0, 0.1, C).astype(np.float32)
    c.X = patches(c.x)
    c.fwd = Product(c.X, c.X.astype(np.float64), np.abs(c.X).astype(np.float64), np.ascontiguousarray(c.w.T))
    c.y32 = c.fwd.ref.astype(np.float32)
    c.g = rng.normal(0, 1, (c.M, C)).astype(np.float32)
    c.bn = bn_block(C, rng)
    c.dw0 = rng.normal(0, 1, (C, TAPS)).astype(np.float32)
    if bf16:
        c.y32, c.g = rne_bf16(c.y32), rne_bf16(c.g)
    if wgrad_fits(W):
        c.wgrad = wgrad_product(c, c.g, c.y32)
    return c


def onto(p, dw0):
    """the product p accumulated onto dw0: reference dw0 + p, scale s + |dw0| (Product.ratio applies)"""
    d = dw0.astype(np.float64)
    q = types.SimpleNamespace(ref=p.ref + d, s=p.s + np.abs(d), floor=p.floor, Y=p.Y)
    q.ratio = lambda x, mask=None: Product.ratio(q, x, mask)
    q.allowed = lambda: Product.allowed(q)
    return q


def sums_outside(S1, S2, flat, own):
    """worst error / tolerance of the column sums S1, S2 [32] (the rows of `part` added in float64): flat = reference of y - pivot,
    own = the values the kernel stored, - pivot; both [M][32] float64.  <= 1 passes."""
    t1 = SUM_TOL * np.abs(flat).sum(0).max()
    e = [np.abs(S1 - flat.sum(0)).max() / t1]
    for v in (flat, own):
        q = (v ** 2).sum(0)
        e.append((np.abs(S2 - q) / (SUM_TOL * q)).max())
    return float(max(e))
