"""Float64 reference, yardstick and cases of the fp32 depthwise 3x3 pair (csrc/dwconv_tiled.hip: ttk_dwconv3x3_fwd, ttk_dwconv3x3_bwd_data,
their _rawskip forms and the fused weight gradient).  Plain numpy on the CPU; tests/test_dw_rows_gpu.py compares the kernels with it through
the C ABI, element by element, tests/test_dw_ref.py pins it on its own without a GPU.  The constants U, MARGIN, UNDECIDED_* and the rows of
a BatchNorm block are tests/conv_ref.py's, imported and not restated.

Reference, in float64 of the float32 inputs (tensors here are channels-last [B][H][W][C]; the device stores channel blocks):
    a_in   = relu(scale (yprev - mean) + beta (+ x))        x: none | a stored activation | relu(bn_skip(raw)), the raw residual form
    y      = dwconv3x3(a_in, w, stride, pad 1)              tap (kh, kw) of output (ho, wo) reads input (ho S - 1 + kh, wo S - 1 + kw)
    dy     = ga (g - gmean) + gb (y_stored - mean)          y_stored: the float64 y rounded once - the backward kernel is GIVEN it
    G      = convT(dy, w) (+ skip_grad)
    g_prev = G [pre > 0]                                    pre = the argument of the relu above
    dW[c][kh 3 + kw] = sum over input pixels of dy(tap) a_in
Per-element scale s: the same contraction over absolute values, with the term bounds of the operands the device forms in float32 on load
(the reasoning of tests/pw_ref.py): P = |scale| (|yprev| + |mean|) + |beta| + |x| in place of |a_in| wherever pre is open or undecided and 0
where it is decidedly closed (there a_in == 0 on any device); for the raw residual |x| is in turn its own P_skip or 0;
D = |ga| (|g| + |gmean|) + |gb| (|y| + |mean|) in place of |dy|.

Yardstick Y, on the case's OWN data, never on the kernel's output; E(x) = max over elements |x - f64| / s.
    y, G   the 9-step float32 fma chain in the kernel's tap order (kh outer, kw inner), operands formed in float32 by numpy (G: one more
           float32 addition for skip_grad);
    a_out  the float32 formation itself against P;
    dW     the LARGER of (1) one serial float32 fma chain per tap over all input pixels in (image, row, column) order and (2) the blocked sum
           that restates the kernel: every thread of a workgroup owns pixel slot p mod 32 of each tile the workgroup takes (`expected_path`,
           `tile_pixels`) and chains its pixels in order; the 8 slots of a wave fold as a butterfly, the four waves add in order, the
           workgroup rows add in row order.  With chains this short (2 to 21 terms per thread at these cases) (2) is the smaller figure; a
           kernel that summed serially would still be judged against (1), so the larger is taken: taking the smaller would gamble on the
           kernel's order.  For C > 64 both run on the first 64 channels - a maximum over a subset is never larger, which only tightens.
Criterion (tests/test_dw_rows_gpu.py), for every element of y, a_out, g_prev and dW:
    |x - f64| <= (MARGIN Y + 2^-24) s,      x == 0 exactly where s == 0
Masked elements follow conv_ref's UNDECIDED rule: |pre64| <= 2^-20 P - there g_prev must be 0 or within the bound of the unmasked value;
decidedly closed elements are exactly 0; at most UNDECIDED_CAP of a case's elements may be undecided (asserted from the reference alone).

Statistics, held to the tensor AS STORED.  The kernel rounds y - pivot once (float32), sums it and its square in float64 and rounds each
workgroup row once to float32, so with d = y - pivot
    |sum_rows part[0] - sum64 d|   <= U (sum |d| + sum_rows |part_row[0]|)
    |sum_rows part[1] - sum64 d^2| <= 2 U sum d^2 + U sum_rows |part_row[1]|
and the backward pair sum g_prev, sum g_prev (yprev - mean) in the first form (g_prev enters exactly, yprev - mean is rounded once).

Inputs (make_case), seeded by the case: yprev, raw, g, skip_grad ~ N(0, 1), a stored residual |N(0, 1)|, w ~ 0.3 N(0, 1) with two whole zero
channels, BatchNorm blocks from conv_ref.bn_block (GMEAN != 0), a random pivot, and (tensors of 8 pixels or more) two pixels whose a_in is
exactly zero in every channel (yprev = -50, residual closed).

`expected_path` restates dw_tiling and the kernels' tile order; CASES names the path each case is there for."""
import functools
import types

import numpy as np

from conv_ref import (bn_block, dy32_of, _err_over_s, U, MARGIN, UNDECIDED_CAP, UNDECIDED_REL, BN_SCALE, BN_BETA, BN_MEAN, BN_GA, BN_GB,
                      BN_GMEAN, BN_AUX, AUX_GMAX)

LDS_PIX = 368          # kLdsPixBudget32
MAX_BLOCKS = 768       # kMaxDwBlocks: 3 workgroups on each of 256 CUs
CARRY_REGS, BLOCK = 5, 256
COL_TILE, COL_TILE_MIN_W = 17, 48
MAX_DYN_LDS = 64 * 1024
PIX_SLOTS = 32         # pixel slots of a workgroup (256 threads / 8 channel quads)
YARD_CHANNELS = 64     # channels that carry the weight-gradient yardstick

# (B, H, W, C, stride, residual form).  Forward path | backward path.  rows = workgroups per 32-channel slab = min(768 / (C / 32), tiles).
CASES = [
    (7, 8, 78, 1024, 1, "stored"),   # carry, R = 2, 4 bands (H = 2 R), 28 tiles on 24 workgroups: runs of two inside an image, from mid-image and ACROSS images | same, the LDS ring; not lean
    (7, 7, 78, 1024, 1, "none"),     # the same with H one below a multiple of R (last band 1 row) | lean, ring
    (5, 9, 78, 1024, 1, "raw"),      # H one past: 5 bands, 25 tiles on 24 workgroups; <1, raw, carry> | <1, raw, ring>
    (13, 9, 33, 1024, 2, "none"),    # stride-2 carry (one shared row), R = 4, 2 bands, 26 tiles on 24 workgroups, a run across images | NI = 3, lean
    (13, 10, 33, 1024, 2, "stored"), # the same with H even: the row handed across the image boundary is a REAL row (H odd: the zero row below the image) | NI = 3, not lean
    (2, 9, 33, 32, 2, "raw"),        # <2, raw, carry> | <2, raw>
    (3, 6, 79, 1024, 1, "raw"),      # 5 column tiles of 16, the last 15 wide; one band; <1, raw, no carry> | same
    (2, 17, 79, 32, 1, "none"),      # column tiles, R = 18: H one below R | same
    (2, 18, 79, 32, 1, "stored"),    # ... H = R
    (2, 19, 79, 32, 1, "none"),      # ... H one past R: a second band of one row
    (2, 3, 256, 32, 1, "none"),      # the widest image: 16 column tiles of 16 | same, lean
    (2, 5, 158, 32, 2, "stored"),    # widest stride-2 carry (316 float4 of the 1280 registers), R = 1, 3 bands; odd x even | R = 4, 2 bands, not lean
    (2, 5, 159, 32, 2, "raw"),       # one past: no carry, R = 1; <2, raw, no carry> | R = 4, 2 bands, <2, raw>
    (1, 3, 163, 32, 2, "none"),      # FORWARD ONLY: the widest admitted stride-2 forward, 65 408 bytes of LDS
    (30, 5, 5, 1024, 1, "stored"),   # NI = 7, five tiles, the last of 2 images | same
    (9, 9, 9, 512, 2, "none"),       # NI = 3 | NI = 8, two tiles, the last of 1 image
    (3, 6, 9, 64, 2, "stored"),      # even x odd; <2, stored, no carry> (one band) | NI = 3
    (3, 1, 40, 64, 1, "none"),       # H = 1 | H = 1
    (3, 40, 1, 64, 2, "stored"),     # W = 1; even side H | W = 1
    (1, 1, 1, 32, 1, "stored"),      # single pixel
    (1, 1, 1, 32, 2, "none"),        # single pixel
    (2, 2, 2, 32, 2, "raw"),         # Ho = Wo = 1; even x even
    (5, 17, 17, 1024, 1, "raw"),     # one band, one image per tile (361 of 368 staged pixels) | same
]
FORWARD_ONLY = {(1, 3, 163, 32, 2, "none")}
# one case per tile form for the position-independence test (every image a copy of the first)
POSITION_CASES = [(7, 8, 78, 1024, 1, "stored"), (13, 10, 33, 1024, 2, "stored"), (2, 19, 79, 32, 1, "none"), (30, 5, 5, 1024, 1, "stored"),
                  (2, 5, 159, 32, 2, "raw")]
# stride-2 forward shapes the launcher refuses (LDS request over 64 KiB); never launched
OVERWIDE_FWD = [(1, 3, 164, 32, 2), (2, 5, 200, 64, 2), (1, 2, 256, 32, 2)]


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def shape_ok(B, H, W, C, stride):
    return B > 0 and H > 0 and 0 < W <= 256 and 32 <= C <= 1024 and C & (C - 1) == 0 and stride in (1, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tiling, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def _band_rows(Hg, Ws, s, bwd):
    sr = LDS_PIX // (Ws + 2)
    if not bwd:
        R = int((sr - 3) / s) + 1  # C division: truncates toward zero
    else:
        R = sr - 2 if s == 1 else 2 * (sr - 2)
    return min(max(R, 1), Hg)


def wg_tiles(P, wg):
    """the tiles workgroup row `wg` takes, in order"""
    if P.carry:
        return list(range(P.tiles * wg // P.rows, P.tiles * (wg + 1) // P.rows))
    return list(range(wg, P.tiles, P.rows))


def tile_geom(P, t):
    """(first image, images, band, first row, end row, first column, columns) of tile t on the grid the kernel iterates"""
    tb, ct = divmod(t, P.NCT)
    ti, band = divmod(tb, P.nbands)
    n0 = ti * P.NI
    nimg = min(P.NI, P.B - n0)
    cx0 = ct * P.TW
    tw = min(P.TW, P.Wg - cx0) if P.NCT > 1 else P.Wg
    r0 = band * P.R
    return n0, nimg, band, r0, min(r0 + P.R, P.Hg), cx0, tw


def tile_pixels(P, t):
    """flat pixels (n Hg + r) Wg + c of tile t in the order of the kernel's pixel index p"""
    n0, nimg, _, r0, r1, cx0, tw = tile_geom(P, t)
    n, r, c = np.meshgrid(np.arange(n0, n0 + nimg), np.arange(r0, r1), np.arange(cx0, cx0 + tw), indexing="ij")
    return ((n * P.Hg + r) * P.Wg + c).reshape(-1)


@functools.lru_cache(maxsize=None)
def expected_path(B, H, W, C, stride, backward):
    """dw_tiling(B, H, W, C, stride, backward) and what follows from the tile order.  Hg x Wg: the grid the kernel iterates (forward: output,
    backward: input pixels).  lds: dynamic LDS bytes of the launch.  walks: some workgroup takes two or more tiles; run_inside /
    run_crosses / run_midstart: in carry mode, some workgroup hands rows on between two bands of one image / goes from the last band of an
    image to the next image / starts its run at a band other than the first."""
    s, bwd = stride, bool(backward)
    Ho, Wo = out_hw(H, W, s)
    P = types.SimpleNamespace(B=B, H=H, W=W, C=C, stride=s, backward=bwd, Ho=Ho, Wo=Wo, NCT=1, TW=Wo)
    P.Hg, P.Wg = (H, W) if bwd else (Ho, Wo)
    carry = (s == 1 and Wo + 2 <= 80) if bwd else ((3 - s) * (W + 2) * 8 <= CARRY_REGS * BLOCK)
    if not carry and s == 1 and W >= COL_TILE_MIN_W:
        P.NCT = (W + COL_TILE - 1) // COL_TILE
        P.TW = (W + P.NCT - 1) // P.NCT
    Wt = P.TW if P.NCT > 1 else (Wo if bwd else W)
    P.R = _band_rows(P.Hg, Wt, s, bwd)
    P.nbands = (P.Hg + P.R - 1) // P.R
    P.nslabs = C // 32
    P.stage_rows = (P.R + 2 if s == 1 else P.R // 2 + 2) if bwd else (P.R - 1) * s + 3
    P.NI = 1
    if P.nbands == 1:
        carry = False
    if P.nbands == 1 and P.NCT == 1:
        P.NI = max(1, min(B, LDS_PIX // (P.stage_rows * ((Wo if bwd else W) + 2))))
    P.carry = carry
    P.tiles = ((B + P.NI - 1) // P.NI) * P.nbands * P.NCT
    P.rows = max(1, min(MAX_BLOCKS // P.nslabs, P.tiles))
    stage = P.NI * P.stage_rows * (Wt + 2) * 32
    P.lds = (stage + (45 * 32 if bwd else 16 * 32)) * 4
    P.walks = P.tiles > P.rows
    P.run_inside = P.run_crosses = P.run_midstart = False
    if carry:
        for wg in range(P.rows):
            ts = wg_tiles(P, wg)
            if len(ts) < 2:
                continue
            P.run_midstart |= ts[0] % P.nbands != 0
            for t in ts[:-1]:
                if (t + 1) % P.nbands == 0:
                    P.run_crosses = True
                else:
                    P.run_inside = True
    return P


def fwd_admitted(B, H, W, C, stride):
    return shape_ok(B, H, W, C, stride) and expected_path(B, H, W, C, stride, False).lds <= MAX_DYN_LDS


def fwd_instance(case):
    """(stride, residual form, carry) - the template arguments of dw_fwd_tiled_k the case reaches"""
    B, H, W, C, s, form = case
    return s, form, expected_path(B, H, W, C, s, False).carry


def bwd_instance(case):
    """(stride, form: lean | full | raw, carry) of dw_bwd_tiled_k with the block input recomputed"""
    B, H, W, C, s, form = case
    return s, {"none": "lean", "stored": "full", "raw": "raw"}[form], expected_path(B, H, W, C, s, True).carry


# ---------------------------------------------------------------------------------------------------------------------------------
# taps
# ---------------------------------------------------------------------------------------------------------------------------------
def fwd_taps(x, S, Ho, Wo):
    """(t, x at the input pixel tap t = kh 3 + kw of every output pixel reads: [B][Ho][Wo][C], zero outside the image)"""
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    for kh in range(3):
        for kw in range(3):
            yield kh * 3 + kw, xp[:, kh:kh + S * (Ho - 1) + 1:S, kw:kw + S * (Wo - 1) + 1:S]


def bwd_taps(dy, S, H, W, colfill=None, wrap=False):
    """(t, dy at the output pixel tap t of every INPUT pixel reads in the transposed convolution: [B][H][W][C], zero where there is none).
    Mutations: colfill[C] - at stride 1 the taps that fall on the padding columns -1 and Wo read this value instead of 0 (the staged
    padding formed as dy(0, 0)); wrap - stride 2, H even: the tap of the last input row that points at output row Ho, which the kernel skips
    with `ho > Ho - 1`, reads row 0 of the next image (the last image: its own last row)."""
    B, Ho, Wo, C = dy.shape
    for kh in range(3):
        for kw in range(3):
            Z = np.zeros((B, H + 2, W + 2, C), dy.dtype)
            Z[:, kh:kh + S * (Ho - 1) + 1:S, kw:kw + S * (Wo - 1) + 1:S] = dy
            D = Z[:, 1:H + 1, 1:W + 1]
            if colfill is not None and S == 1:
                hi = np.arange(H)
                ok = (hi + 1 - kh >= 0) & (hi + 1 - kh < Ho)
                if kw == 2:
                    D[:, ok, 0] = colfill
                if kw == 0:
                    D[:, ok, W - 1] = colfill
            if wrap and S == 2 and H % 2 == 0 and kh == 0:
                tw = np.arange(W) + 1 - kw
                sel = (tw >= 0) & (tw % 2 == 0) & (tw // 2 < Wo)
                src = np.concatenate([dy[1:, 0], dy[-1:, Ho - 1]])
                D[:, H - 1, sel] = src[:, tw[sel] // 2]
            yield kh * 3 + kw, D


def conv_fwd(x, w, S, Ho, Wo):
    """float64 depthwise 3x3 of x[B][H][W][C] with w[C][9]"""
    acc = np.zeros((x.shape[0], Ho, Wo, x.shape[3]))
    for t, xt in fwd_taps(x, S, Ho, Wo):
        acc += xt * w[:, t].astype(np.float64)
    return acc


def conv_bwd(dy, w, S, H, W, **mut):
    acc = np.zeros((dy.shape[0], H, W, dy.shape[3]))
    for t, dt in bwd_taps(dy, S, H, W, **mut):
        acc += dt * w[:, t].astype(np.float64)
    return acc


def _chain(taps, w):
    """the 9-step float32 fma chain in tap order (float32 + exact float64 product: a single rounding)"""
    acc = None
    for t, xt in taps:
        term = xt.astype(np.float64) * w[:, t].astype(np.float64)
        acc = term.astype(np.float32) if acc is None else (acc + term).astype(np.float32)  # (0 + term: the fma onto a zero accumulator)
    return acc


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
FORMS = ("none", "stored", "raw")


def case_seed(case):
    return int(sum(v * p for v, p in zip(case[:5], (1000003, 10007, 1009, 101, 11))) + 7 * FORMS.index(case[5]))


def _pre(bn, y, x=0.0):
    """(pre64, P) of scale (y - mean) + beta + x"""
    b, y64 = bn.astype(np.float64), y.astype(np.float64)
    pre = b[BN_SCALE] * (y64 - b[BN_MEAN]) + b[BN_BETA]
    P = np.abs(b[BN_SCALE]) * (np.abs(y64) + np.abs(b[BN_MEAN])) + np.abs(b[BN_BETA])
    return pre + x, P


def _pre32(bn, y):
    return (bn[BN_SCALE] * (y - bn[BN_MEAN]) + bn[BN_BETA]).astype(np.float32)  # float32 throughout (the device: one fma)


@functools.lru_cache(maxsize=2)
def make_case(case):
    """The float32 inputs of one case (never written afterwards) and everything the reference derives from the forward inputs."""
    B, H, W, C, S, form = case
    rng = np.random.default_rng(case_seed(case))
    c = types.SimpleNamespace(case=case, B=B, H=H, W=W, C=C, stride=S, form=form)
    c.Ho, c.Wo = out_hw(H, W, S)
    c.want_a = form != "none" and S == 1   # the block input is materialised (a_out) where the block has a residual connection
    c.has_sg = form != "none" and S == 1   # ... and then the gradient has a residual term
    f32 = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    c.yprev = f32(B, H, W, C)
    c.raw = f32(B, H, W, C) if form == "raw" else None
    c.x = np.abs(f32(B, H, W, C)) if form == "stored" else None
    c.zero_pixels = []
    if B * H * W >= 8:  # two pixels whose a_in is exactly zero: the second of the tensor and the last but one
        c.zero_pixels = [1, B * H * W - 2]
        c.yprev.reshape(-1, C)[c.zero_pixels] = -50.0
        if c.raw is not None:
            c.raw.reshape(-1, C)[c.zero_pixels] = -50.0
        if c.x is not None:
            c.x.reshape(-1, C)[c.zero_pixels] = 0.0
    c.w = (rng.normal(0, 1, (C, 9)) * 0.3).astype(np.float32)
    c.zero_channels = [1, C // 2 + 3]
    c.w[c.zero_channels] = 0.0
    c.bn_prev, c.bn_skip, c.bn_dw = bn_block(C, rng), bn_block(C, rng), bn_block(C, rng)
    c.piv = rng.normal(0, 0.5, C).astype(np.float32)
    c.g = f32(B, c.Ho, c.Wo, C)
    c.sg = f32(B, H, W, C) if c.has_sg else None
    # ---- the block input
    x64, xabs, x32 = 0.0, 0.0, None
    if form == "stored":
        x64, xabs, x32 = c.x.astype(np.float64), c.x.astype(np.float64), c.x
    elif form == "raw":
        ps, Ps = _pre(c.bn_skip, c.raw)
        x64 = np.maximum(ps, 0.0)
        xabs = np.where(ps >= -UNDECIDED_REL * Ps, Ps, 0.0)
        x32 = np.maximum(_pre32(c.bn_skip, c.raw), np.float32(0))
    c.pre64, c.P = _pre(c.bn_prev, c.yprev, x64)
    c.P = c.P + xabs
    c.undecided = (np.abs(c.pre64) <= UNDECIDED_REL * c.P) & (c.P > 0)
    c.open = c.pre64 > 0
    c.share = float(c.undecided.mean())
    c.a64 = np.maximum(c.pre64, 0.0)
    c.Aabs = np.where(c.open | c.undecided, c.P, 0.0)
    p32 = _pre32(c.bn_prev, c.yprev)
    c.a32 = np.maximum(p32 if x32 is None else (p32 + x32).astype(np.float32), np.float32(0))
    c.y64 = conv_fwd(c.a64, c.w, S, c.Ho, c.Wo)
    c.y32 = c.y64.astype(np.float32)  # what the backward kernels are GIVEN
    return c


class Quantity:
    """one output tensor: float64 value, per-element scale and yardstick"""

    def __init__(self, ref, s, yard, sel=None):
        self.ref, self.s = ref, s
        e = _err_over_s(yard, ref if sel is None else ref[sel], s if sel is None else s[sel])
        self.Y = float(e.max())

    def allowed(self):
        """per element: the largest |x - f64| the criterion accepts"""
        return (MARGIN * self.Y + U) * self.s

    def onto(self, base):
        """the same quantity accumulated onto `base`: one more term of the contraction"""
        q = Quantity.__new__(Quantity)
        q.ref, q.s, q.Y = self.ref + base, self.s + np.abs(base), self.Y
        return q

    def outside(self, x, mask=None):
        """worst |x - f64| / allowed over the elements (of mask); inf where s == 0 and x != 0"""
        e = _err_over_s(x, self.ref, self.allowed())
        return float(e.max() if mask is None else e[mask].max())


@functools.lru_cache(maxsize=2)
def forward(case):
    """(y, a): Quantity of the convolution output and of the materialised block input"""
    c = make_case(case)
    y = Quantity(c.y64, conv_fwd(c.Aabs, np.abs(c.w), c.stride, c.Ho, c.Wo), _chain(fwd_taps(c.a32, c.stride, c.Ho, c.Wo), c.w))
    return y, Quantity(c.a64, c.Aabs, c.a32)


def dy_terms(c):
    """(dy64, D): exact dy and the bound of its terms, [B][Ho][Wo][C]"""
    bn, g, y = c.bn_dw.astype(np.float64), c.g.astype(np.float64), c.y32.astype(np.float64)
    dy64 = bn[BN_GA] * (g - bn[BN_GMEAN]) + bn[BN_GB] * (y - bn[BN_MEAN])
    D = np.abs(bn[BN_GA]) * (np.abs(g) + np.abs(bn[BN_GMEAN])) + np.abs(bn[BN_GB]) * (np.abs(y) + np.abs(bn[BN_MEAN]))
    return dy64, D


def dy_fill(c):
    """dy of a padding pixel formed from zero loads instead of being left zero: ga (0 - gmean) + gb (0 - mean)"""
    bn = c.bn_dw.astype(np.float64)
    return bn[BN_GA] * (0.0 - bn[BN_GMEAN]) + bn[BN_GB] * (0.0 - bn[BN_MEAN])


@functools.lru_cache(maxsize=2)
def dgrad(case):
    """Quantity of the unmasked G[B][H][W][C] with .open / .undecided / .share for masked_outside"""
    c = make_case(case)
    dy64, D = dy_terms(c)
    dy32 = dy32_of(c.g, c.y32, c.bn_dw)
    ref, s = conv_bwd(dy64, c.w, c.stride, c.H, c.W), conv_bwd(D, np.abs(c.w), c.stride, c.H, c.W)
    yard = _chain(bwd_taps(dy32, c.stride, c.H, c.W), c.w)
    if c.sg is not None:
        ref, s, yard = ref + c.sg, s + np.abs(c.sg), (yard + c.sg).astype(np.float32)
    q = Quantity(ref, s, yard)
    q.open, q.undecided, q.share = c.open, c.undecided, c.share
    return q


def gprev_ref(case):
    """the float64 g_prev with the mask decided by pre64"""
    return dgrad(case).ref * make_case(case).open


def wgrad_terms(c, dy, a, nch=None, **mut):
    """T[9][B H W][channels]: the product dy(tap) * a of every input pixel, float64"""
    ch = slice(0, nch)
    return np.stack([(dt[..., ch].astype(np.float64) * a[..., ch]).reshape(-1, dt[..., ch].shape[-1])
                     for _, dt in bwd_taps(dy, c.stride, c.H, c.W, **mut)])


def wgrad_sum(c, dy, a, **mut):
    """sum over the input pixels of dy(tap) * a: [C][9], float64"""
    return np.stack([(dt.astype(np.float64) * a).reshape(-1, c.C).sum(0) for _, dt in bwd_taps(dy, c.stride, c.H, c.W, **mut)], 1)


def wgrad_pixel(c, dy, a, pix):
    """the [C][9] contribution of flat input pixel `pix` to wgrad_sum"""
    n, r = divmod(pix, c.H * c.W)
    return np.stack([dt[n, r // c.W, r % c.W].astype(np.float64) * a[n, r // c.W, r % c.W] for _, dt in bwd_taps(dy, c.stride, c.H, c.W)], 1)


def masked_outside(q, out):
    """worst |out - f64| / allowed of a masked gradient: decidedly closed elements must be 0 (else inf), undecided ones 0 or within the bound"""
    out = np.asarray(out, np.float64)
    e = _err_over_s(out, q.ref, q.allowed())
    e = np.where(q.undecided & (out == 0), 0.0, e)
    return float(np.where(~q.open & ~q.undecided, np.where(out == 0, 0.0, np.inf), e).max())


def blocked_sum(P, T):
    """T[9][pixels][ch] summed as the backward kernel does (module docstring); float32 throughout"""
    per_wg = []
    for wg in range(P.rows):
        slots = [[] for _ in range(PIX_SLOTS)]
        for t in wg_tiles(P, wg):
            px = tile_pixels(P, t)
            for sl in range(PIX_SLOTS):
                slots[sl].extend(px[sl::PIX_SLOTS])
        per_wg.append(slots)
    L = max(len(s) for slots in per_wg for s in slots)
    npix = T.shape[1]
    idx = np.full((P.rows, PIX_SLOTS, L), npix, np.int64)
    for r, slots in enumerate(per_wg):
        for sl, s in enumerate(slots):
            idx[r, sl, :len(s)] = s
    Tp = np.concatenate([T, np.zeros((9, 1, T.shape[2]))], 1)
    acc = np.zeros((9, P.rows, PIX_SLOTS, T.shape[2]), np.float32)
    for l in range(L):
        acc = (acc + Tp[:, idx[:, :, l]]).astype(np.float32)
    v = acc.reshape(9, P.rows, 4, 8, -1)
    for off in (1, 2, 4):  # the butterfly over the 8 pixel slots of a wave
        v = (v + v[:, :, :, np.arange(8) ^ off]).astype(np.float32)
    waves = v[:, :, :, 0]
    a = np.zeros_like(waves[:, :, 0])
    for w in range(4):
        a = (a + waves[:, :, w]).astype(np.float32)
    out = np.zeros_like(a[:, 0])
    for r in range(P.rows):
        out = (out + a[:, r]).astype(np.float32)
    return out


def serial_sum(T):
    """T[taps][pixels][ch] -> [taps][ch]: one float32 chain per tap over the pixels in order"""
    acc = np.zeros((T.shape[0], T.shape[2]), np.float32)
    for p in range(T.shape[1]):
        acc = (acc + T[:, p]).astype(np.float32)
    return acc


@functools.lru_cache(maxsize=2)
def wgrad(case):
    """Quantity of dW as [C][9]; .E_serial, .E_blocked: the two yardstick figures"""
    c = make_case(case)
    dy64, D = dy_terms(c)
    dy32 = dy32_of(c.g, c.y32, c.bn_dw)
    ref, s = wgrad_sum(c, dy64, c.a64), wgrad_sum(c, D, c.Aabs)
    nch = min(c.C, YARD_CHANNELS)
    T = wgrad_terms(c, dy32, c.a32.astype(np.float64), nch)
    P = expected_path(c.B, c.H, c.W, c.C, c.stride, True)
    serial, blocked = serial_sum(T).T, blocked_sum(P, T).T
    q = Quantity(ref, s, serial, np.s_[:nch])
    q.E_serial = q.Y
    q.E_blocked = float(_err_over_s(blocked, ref[:nch], s[:nch]).max())
    q.Y = max(q.E_serial, q.E_blocked)
    return q


# ---------------------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------------------
def stat_ratios(part, v, d, square, length=None):
    """part[rows][2][C] against the stored tensors: row 0 = sum v (forward: v = y - pivot; backward: v = g_prev), row 1 = sum v * d
    (forward, square: d = v, the bound 2 U sum v^2; backward: d = yprev - mean, the bound U sum |v d|), each plus U sum_rows |part_row|.
    length: the kernel sums in float32 and no term passes through more than `length` additions (tests/anyc_ref.py derives it): the bound
    is then length U sum |v| and (length + 2) U sum |v d|.
    v, d: [pixels][C] float64.  Returns the worst |error| / bound of either row (0 / 0 = 0)."""
    ps = np.asarray(part, np.float64)
    out = []
    for k, terms in ((0, v), (1, v * d)):
        err = np.abs(ps[:, k].sum(0) - terms.sum(0))
        if length is None:
            bound = (2.0 if (k == 1 and square) else 1.0) * U * np.abs(terms).sum(0) + U * np.abs(ps[:, k]).sum(0)
        else:
            bound = (length + 2.0 * k) * U * np.abs(terms).sum(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf)).max()))
    return out
