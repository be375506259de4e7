"""Float64 reference, criterion, cases and restated launch arithmetic of the pointwise kernels of the bf16-COMPUTE path: forward and data
gradient (csrc/bc_gemm.hip: bc_prepare_k, bc_gemm_e_k<MODE,NB,KH>, bc_gemm_l_k<MODE,NCT>; helpers of csrc/bc_common.h) and the weight
gradient (csrc/bc_wgrad.hip: bc_wgrad_k and the folds of bc_common.h - its section at the end of the file has its own notes).  Plain numpy
on the CPU; tests/test_bc_rows_gpu.py compares the kernels with it through the C ABI, tests/test_bc_ref.py pins it on its own without a GPU.
The fused backward (csrc/bc_fused.hip) and the depthwise pair (csrc/bc_dw.hip: tiling restated, forward and data gradient held bit for
bit where the emulation is exact) have their sections, with their own notes, after it.
Inputs: every case takes the FIRST of up to SALTS seeded draws whose operands meet the caps - a selection on the reference alone (the
draw is printed with every figure): the published shares of undecided and widened elements are those of the selected draws, not typical.

Layout.  off64: a C-channel tensor of M pixels is stored [C/64][M][64] (C = 32: plain [M][32]); to_blocks / from_blocks.

Operands.  The kernels form their operands from bf16 tensors with one or two fp32 fmas and round to bf16 (make_frag, store_block):
    forward        a    = relu(bf16(fma(sc, y, sh))),          sh = fma(-sc, mean, beta)
    data gradient  dy   = bf16(fma(ga, g, fma(gb, y, c0))),    c0 = -ga*gmean - gb*mean  (a plain expression: see below)
                   mask = [fma(sc, y_dw, sh) > 0]
A bf16 value times a float32 value has 32 significant bits, so the float64 product is exact; adding a float32 to it is exact in float64
unless the exponents are far apart, and then float32(float64 sum) IS fmaf - one rounding of the exact value.  `fma32` does that and takes
the TwoSum residual of the float64 addition: where it is not zero the exact value lies strictly between two neighbouring float64s and fma32
returns the float32 roundings of both (lo, hi) - rounding is monotone, the device's value is one of them or between.  Per-channel constants
are computed exactly (fractions.Fraction, `f32_of`).  c0 is not pinned by the source: the compiler may contract either product, so the
reference carries the three candidates (no contraction, the first product fused, the second) - `c0_candidates`.

Undecided.  An operand element is UNDECIDED when the bf16 roundings of its candidates (fma32's lo / hi, over the three c0) differ.  The
reference then contracts the first candidate and the element's spread delta = hi - lo widens the allowed error of every output that
contracts over it by |other operand| * delta (`widen`).  A mask element whose lo and hi lie on different sides of zero is undecided in
conv_ref's sense: the output may be +0 or the unmasked value.  No element is left out of a comparison.

Criterion, per output element, with s the contraction over absolute values (the larger candidate):
    |acc - f64| <= (MARGIN * Y + 2^-24) * s + widen              (MARGIN = 4, 2^-24: conv_ref.py)
and the bf16 value v the kernel stores is judged by stem_ref's bracket  rne(f64 - allowed) <= v <= rne(f64 + allowed),  +0 where s == 0.
Y is conv_ref.chain32 - one float32 fma per contraction step - on the case's own bf16 matrices (the bf16 x bf16 product is exact in
float32; only the accumulation order is the kernels'), over at most Y_ROWS rows of the case: the maximum over a subset is never larger than
the maximum over all rows, so the subset can only tighten the criterion.

Statistics (`part`), against the tensor AS STORED.  Row r of `part` holds the sums of a known set of pixels (row_of_pixel):
    E kernel: workgroup b's eight waves take the 32-pixel groups 8 b + wave + k * 8 * grid;  L kernel: row tile rt = pixels [rt RT, rt RT + RT).
A lane adds its values serially (E: NI per group; L: 2 x 4), then a shuffle tree (log2 of the pixels per instruction), then the waves
(E: 8, L: 4) - `stat_depth` counts these additions, + 1 for the fp32 subtraction that forms each term:
    |part[r][0] - sum d| <= L u sum |d|,      |part[r][1] - sum q| <= (L + 2) u sum |q|
with d = v - pivot, q = d^2 (forward); d = v, q = v (y_dw - mean) (data gradient), the right-hand sums over the row's pixels.

Constants.  "full": float32 draws as tests/test_bc_kernels_gpu.py's.  "short": every constant a small fixed-point number (scale and ga
multiples of 2^-7 in [0.5, 1.5], the rest multiples of 2^-8 below 1), so that c0 and sh are exact in every evaluation order: no operand
is undecided (asserted for every case).  For "full" the caps UNDECIDED_CAP and WIDENED_CAP are asserted for every case.

expected_path(mode, M, cin, cout): the kernel, its template arguments and launch plan, restated from launch_gemm / l_plan / e_grid."""
import fractions
import functools
import types

import numpy as np

from conv_ref import BN_BETA, BN_GA, BN_GB, BN_GMEAN, BN_MEAN, BN_RSTD, BN_SCALE, MARGIN, U, _err_over_s, chain32  # noqa: F401
from stem_ref import bf16_bits, bf16_widen, bracket, bracket_ratio, rne_bf16, trunc_bf16  # noqa: F401

Fr = fractions.Fraction
UNDECIDED_CAP = 1e-4      # largest share of undecided operand elements of a case ("full" constants)
WIDENED_CAP = 0.05        # largest share of output elements whose bound an undecided operand widened
Y_ROWS = 1024             # rows of a case the yardstick is evaluated on (the first Y_ROWS - 64 and the last 64)
TAIL = 4096               # elements after the end of an output that the GPU test watches: a 16-byte store of a short tile lands there


# ---------------------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------------------
def cbw(C):
    return C if C < 64 else 64


def off64(m, c, M, C):
    w = cbw(C)
    return ((c // w) * M + m) * w + c % w


def to_blocks(x):
    """x[M][C] -> the flat storage order"""
    M, C = x.shape
    w = cbw(C)
    return np.ascontiguousarray(x.reshape(M, C // w, w).transpose(1, 0, 2)).reshape(-1)


def from_blocks(flat, M, C):
    w = cbw(C)
    return np.ascontiguousarray(np.asarray(flat).reshape(C // w, M, w).transpose(1, 0, 2)).reshape(M, C)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact float32 arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def f32_of(q):
    """the float32 nearest to the rational q, ties to even (float(q) is correctly rounded to float64; its float32 rounding may be a
    double rounding, so the neighbours are compared exactly)"""
    f = np.float32(float(q))
    best, best_d = None, None
    for c in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
        d = abs(Fr(float(c)) - q)
        even = (np.float32(c).view(np.uint32) & 1) == 0
        if best is None or d < best_d or (d == best_d and even):
            best, best_d = np.float32(c), d
    return best


def _fr(v):
    return Fr(float(v))


def shift_of(bn):
    """sh = fma(-sc, mean, beta) per channel, exactly rounded (fill_cA, fill_cE)"""
    return np.array([f32_of(_fr(b) - _fr(s) * _fr(m)) for s, m, b in zip(bn[BN_SCALE], bn[BN_MEAN], bn[BN_BETA])], np.float32)


def c0_candidates(bn):
    """[3][C]: -ga*gmean - gb*mean as (plain, first product fused, second product fused)"""
    out = np.zeros((3, bn.shape[1]), np.float32)
    for c in range(bn.shape[1]):
        ga, gb, gm, mu = (_fr(bn[r, c]) for r in (BN_GA, BN_GB, BN_GMEAN, BN_MEAN))
        t1, t2 = f32_of(-ga * gm), f32_of(gb * mu)
        out[0, c] = f32_of(_fr(t1) - _fr(t2))
        out[1, c] = f32_of(-ga * gm - _fr(t2))
        out[2, c] = f32_of(_fr(t1) - gb * mu)
    return out


def fma32(x, k, c):
    """(lo, hi, inexact) of fmaf(k, x, c): x bf16 values (float32), k float32 per channel, c float32.  lo == hi where the float64 sum is
    exact (then it is fmaf bit for bit); elsewhere the float32 roundings of the two float64 neighbours that enclose the exact value."""
    p = x.astype(np.float64) * k.astype(np.float64)
    c = np.broadcast_to(c, p.shape).astype(np.float64)
    s = p + c
    bb = s - p
    r = (p - (s - bb)) + (c - bb)
    lo = hi = s.astype(np.float32)
    inexact = r != 0
    if inexact.any():
        lo = np.where(r < 0, np.nextafter(s, -np.inf).astype(np.float32), lo)
        hi = np.where(r > 0, np.nextafter(s, np.inf).astype(np.float32), hi)
    return lo, hi, inexact


def _operand(cands, inexact):
    """candidates (bf16 values, float32) -> the operand: .v nominal (the first), .lo / .hi, .delta, .undecided, .inexact"""
    lo, hi = np.minimum.reduce(cands), np.maximum.reduce(cands)
    o = types.SimpleNamespace(v=cands[0], lo=lo, hi=hi, inexact=inexact)
    o.delta = hi.astype(np.float64) - lo.astype(np.float64)
    o.undecided = o.delta != 0
    o.abs = np.maximum(np.abs(lo), np.abs(hi)).astype(np.float64)
    return o


def relu(v):
    return np.where(v > 0, v, np.float32(0))  # (+0 for -0 and negatives: relu_pk)


def act_operand(y, bn, round_bf16=rne_bf16):
    """a = relu(bf16(fma(sc, y, sh)))"""
    lo, hi, inexact = fma32(y, bn[BN_SCALE], shift_of(bn))
    return _operand([relu(round_bf16(lo)), relu(round_bf16(hi))], inexact)


def dy_operand(g, y, bn, round_bf16=rne_bf16):
    """dy = bf16(fma(ga, g, fma(gb, y, c0))) over the three c0"""
    cands, inexact = [], np.zeros(g.shape, bool)
    for c0 in c0_candidates(bn):
        ilo, ihi, ix = fma32(y, bn[BN_GB], c0)
        olo, _, ox1 = fma32(g, bn[BN_GA], ilo)
        _, ohi, ox2 = fma32(g, bn[BN_GA], ihi)
        inexact |= ix | ox1 | ox2
        cands += [round_bf16(olo), round_bf16(ohi)]
    return _operand(cands, inexact)


def mask_of(ydw, bn):
    """(open, undecided) of [fma(sc, y_dw, sh) > 0]"""
    lo, hi, _ = fma32(ydw, bn[BN_SCALE], shift_of(bn))
    return lo > 0, (lo > 0) != (hi > 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# one product
# ---------------------------------------------------------------------------------------------------------------------------------
def y_rows(M):
    return np.arange(M) if M <= Y_ROWS else np.concatenate([np.arange(Y_ROWS - 64), np.arange(M - 64, M)])


class BcProduct:
    """out[M][N] = A @ B: A an operand of _operand() ([M][K]), B[K][N] the bf16 weight image (float32 values)"""

    def __init__(self, A, B):
        B64 = B.astype(np.float64)
        self.A, self.B = A, B
        self.ref = A.v.astype(np.float64) @ B64
        self.s = A.abs @ np.abs(B64)
        self.widen = A.delta @ np.abs(B64) if A.undecided.any() else np.zeros_like(self.s)
        rows = y_rows(A.v.shape[0])
        self.Y = float(_err_over_s(chain32(A.v[rows], B), self.ref[rows], self.s[rows]).max())
        self.floor = np.zeros_like(self.s)

    def allowed(self):
        return (MARGIN * self.Y + U) * self.s + self.widen

    @property
    def widened_share(self):
        return float((self.widen > 0).mean())


def outside(p, v, open_=None, undecided=None):
    """number of stored values v (float32, widened bf16) outside the criterion.  open_ / undecided: the mask of the data gradient -
    closed elements must be +0, undecided ones +0 or inside the bracket."""
    lo, hi = bracket(p)
    v = np.ascontiguousarray(v, np.float32)
    zero_bits = v.view(np.uint32) == 0
    bad = (v < lo) | (v > hi) | ~np.isfinite(v) | ((p.s == 0) & ~zero_bits)
    if open_ is not None:
        bad = np.where(open_ & ~undecided, bad, np.where(undecided, bad & ~zero_bits, ~zero_bits))
    return int(bad.sum())


def excess(p, v, open_=None):
    """how far outside the worst element is: its distance to the bracket over its allowed error (0: all inside).  Closed elements count
    by their distance from 0."""
    lo, hi = bracket(p)
    v = np.asarray(v, np.float64)
    d = np.maximum(np.maximum(lo - v, v - hi), 0.0)
    if open_ is not None:
        d = np.where(open_, d, np.abs(v))
    a = np.maximum(p.allowed(), 1e-300)
    return float((d / a).max())


def ratio(p, v, open_=None):
    """the printed figure: stem_ref.bracket_ratio over the elements that are open and not widened (the widened ones are held by the
    bracket alone)"""
    q = types.SimpleNamespace(ref=p.ref, Y=p.Y, s=np.where((p.widen > 0) | (False if open_ is None else ~open_), 0.0, p.s))
    return bracket_ratio(q, v)


# ---------------------------------------------------------------------------------------------------------------------------------
# the host's launch arithmetic (csrc/bc_gemm.hip), restated
# ---------------------------------------------------------------------------------------------------------------------------------
E_INSTANCES = {(32, 64): (2, 1), (64, 128): (4, 2), (128, 128): (4, 4), (64, 32): (1, 2), (128, 64): (2, 4)}  # (K, N) -> (NB, KH)
LDS_LIMIT = 160 * 1024


def shape_ok(cin, cout):
    p2 = lambda v: 32 <= v <= 1024 and v & (v - 1) == 0
    return p2(cin) and p2(cout)


def is_e(K, N):
    return N <= 128 and K <= 256


def is_l(K, N):
    return N % 256 == 0 and K % 128 == 0


def is_l128(K, N):
    return N == 128 and K == 256


def e_grid(M):
    return min(-(-(-(-M // 32)) // 8), 256)


def l_plan(M, N, nct=256):
    ncol = N // nct
    t256 = -(-M // 256)
    rounds = -(-(t256 * ncol) // 256)
    target = max(rounds * 256 // ncol, 1)
    RT = min(max(-(-(-(-M // target)) // 8) * 8, 8), 256)
    nrt = -(-M // RT)
    return types.SimpleNamespace(RT=RT, nrt=nrt, ncol=ncol, grid=-(-nrt // 8) * 8 * ncol, rounds=rounds)


def e_lds_bytes(K, N):
    OC = 32 if N < 64 else 64
    return N * K * 2 + 3 * K * 4 + 3 * N * 4 + max(8 * 4 * OC * 16, 8 * 2 * N * 4)


def l_lds_bytes(K, nct=256):
    return (2 * nct * 8 + 2 * 2048) * 16 + 3 * nct * 4 + 3 * K * 4


def kn(mode, cin, cout):
    """(contraction channels, output channels) of the product"""
    return (cin, cout) if mode == "fwd" else (cout, cin)


def expected_path(mode, M, cin, cout):
    """None where the entry point refuses; else .kernel ("e" | "l"), .inst (the template arguments after MODE), .rows of `part`, .grid,
    .lds and for "l" the plan (RT, nrt, ncol, rounds, idle workgroups of the padded grid)"""
    K, N = kn(mode, cin, cout)
    if M < 1 or not shape_ok(cin, cout):
        return None
    if is_l128(K, N) or (not is_e(K, N) and is_l(K, N)):
        nct = 128 if is_l128(K, N) else 256
        p = l_plan(M, N, nct)
        return types.SimpleNamespace(kernel="l", inst=(nct,), rows=p.nrt, grid=p.grid, lds=l_lds_bytes(K, nct), RT=p.RT, nrt=p.nrt, ncol=p.ncol,
                                     rounds=p.rounds, idle=p.grid - p.nrt * p.ncol)
    if is_e(K, N) and (K, N) in E_INSTANCES:
        g = e_grid(M)
        groups = -(-M // 32)
        return types.SimpleNamespace(kernel="e", inst=E_INSTANCES[(K, N)], rows=g, grid=g, lds=e_lds_bytes(K, N), groups=groups,
                                     second_group=max(groups - 8 * g, 0))
    return None


def row_of_pixel(path, M):
    """[M]: the row of `part` each pixel's values are summed into"""
    pix = np.arange(M)
    if path.kernel == "l":
        return pix // path.RT
    return ((pix // 32) % (8 * path.grid)) // 8


def stat_depth(path, N):
    """L: the additions behind one value of `part` (+ 1: the subtraction that forms each term)"""
    if path.kernel == "l":
        return 2 * 4 + 3 + 4 + 1
    OC = 32 if N < 64 else 64
    ppi = 64 // (OC // 8)               # pixels per store instruction of a wave
    per_wave = -(-path.groups // (8 * path.grid))
    return per_wave * (32 // ppi) + int(np.log2(ppi)) + 8 + 1


def stats_outside(part, rows_of, d, q, L):
    """worst error / bound over the rows of part[rows][2][N] (float64) against the terms d, q [M][N] (float64) summed per row"""
    R = part.shape[0]
    worst = 0.0
    for col, t, depth in ((0, d, L), (1, q, L + 2)):
        S, Sabs = np.zeros((R, t.shape[1])), np.zeros((R, t.shape[1]))
        np.add.at(S, rows_of, t)
        np.add.at(Sabs, rows_of, np.abs(t))
        err, bound = np.abs(part[:, col] - S), depth * U * Sabs
        if not np.isfinite(part[:, col]).all() or (err[bound == 0] != 0).any():
            return float("inf")
        live = bound > 0
        if live.any():
            worst = max(worst, float((err[live] / bound[live]).max()))
    return worst


def sum_slots(path, M, N):
    """per pixel (row of `part`, wave, pixel slot of the lane, serial step of the lane) and the extents (waves, slots, steps)"""
    pix = np.arange(M)
    if path.kernel == "l":
        off = pix % path.RT
        return (pix // path.RT, off // 64, off % 8, (off % 64) // 32 * 4 + (off % 32) // 8), (4, 8, 8)
    OC = 32 if N < 64 else 64
    ppi = 64 // (OC // 8)
    ni = 32 // ppi
    g = pix // 32
    per_wave = -(-path.groups // (8 * path.grid))
    return ((g % (8 * path.grid)) // 8, g % 8, pix % 32 % ppi, g // (8 * path.grid) * ni + pix % 32 // ppi), (8, ppi, per_wave * ni)


def sum_model(path, t, N):
    """float32 model of one column of `part` in the kernels' order: the lane's serial sum, the __shfl_xor tree over the pixel slots, the
    waves in order.  t[M][N]: the terms (rounded to float32 first, as the kernel forms them)."""
    (row, wave, slot, step), (W, S, T) = sum_slots(path, t.shape[0], N)
    cube = np.zeros((path.rows, W, S, T, N), np.float32)
    cube[row, wave, slot, step] = t.astype(np.float32)
    lane = np.zeros((path.rows, W, S, N), np.float32)
    for k in range(T):
        lane = lane + cube[:, :, :, k]
    off = 1
    while off < S:
        lane = lane + lane[:, :, np.arange(S) ^ off]
        off *= 2
    out = np.zeros((path.rows, N), np.float32)
    for w in range(W):
        out = out + lane[:, w, 0]
    return out.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def bn_full(C, rng):
    """the distributions of tests/test_bc_kernels_gpu.py::_bn, full float32 mantissas"""
    bn = np.zeros((8, C), np.float32)
    bn[BN_SCALE] = rng.uniform(0.5, 1.5, C)
    bn[BN_BETA] = rng.normal(0, 0.2, C)
    bn[BN_MEAN] = rng.normal(0, 0.3, C)
    bn[BN_RSTD] = rng.uniform(0.5, 1.5, C)
    bn[BN_GA] = rng.uniform(0.5, 1.5, C)
    bn[BN_GB] = rng.normal(0, 0.2, C)
    bn[BN_GMEAN] = rng.normal(0, 0.05, C)
    return bn


def bn_short(C, rng):
    """the same distributions on fixed-point grids: scale, rstd, ga multiples of 2^-7 in [0.5, 1.5]; beta, mean, gb, gmean multiples of
    2^-8 below 1 - at most 8 significant bits each, every product a multiple of 2^-15 below 2, every sum of two exact in float32"""
    bn = bn_full(C, rng)
    for r in (BN_SCALE, BN_RSTD, BN_GA):
        bn[r] = np.round(bn[r] * 128) / 128
    for r in (BN_BETA, BN_MEAN, BN_GB, BN_GMEAN):
        bn[r] = np.clip(np.round(bn[r] * 256), -255, 255) / 256
    return bn


def significant_bits(x):
    m, _ = np.frexp(np.abs(np.asarray(x, np.float64)))
    i = np.round(m * 2.0 ** 53).astype(np.int64)
    low = np.where(i == 0, 1 << 53, i & -i)
    return np.where(i == 0, 0, 53 - np.log2(low.astype(np.float64)).astype(np.int64))


@functools.lru_cache(maxsize=4)
def pw_case(mode, M, cin, cout, family):
    """the first of SALTS seeded draws (_pw_case) whose operand meets UNDECIDED_CAP: in a tensor of fewer than 10^4 elements a single
    undecided element is above it"""
    for salt in range(SALTS):
        c = _pw_case(mode, M, cin, cout, family, salt)
        if c.op.undecided.mean() <= UNDECIDED_CAP and c.p.widened_share <= WIDENED_CAP:
            return c
    raise ValueError(f"no draw of {SALTS} meets the caps for {(mode, M, cin, cout, family)}")


def _pw_case(mode, M, cin, cout, family, salt):
    """The inputs of one case and its product (never written afterwards).  mode "fwd": y = a(ydw) @ W^T, [M][cout]; "dgrad":
    g_dw = dy(g, y) @ W under the mask of ydw, [M][cin].  Pixel 1 (M >= 3) makes a whole zero operand row in the forward (s == 0 over the
    output row); the last pixel is a copy of pixel 0 (M >= 2): its output row must repeat the bits."""
    rng = np.random.default_rng([{"fwd": 0, "dgrad": 1}[mode], M, cin, cout, {"full": 0, "short": 1}[family], salt])
    bn_of = bn_full if family == "full" else bn_short
    c = types.SimpleNamespace(mode=mode, M=M, cin=cin, cout=cout, family=family, salt=salt, path=expected_path(mode, M, cin, cout))
    c.K, c.N = kn(mode, cin, cout)
    c.w = (rng.normal(0, 1, (cout, cin)) / np.sqrt(cin)).astype(np.float32)
    c.wb = rne_bf16(c.w)                                         # the weight image's values
    c.ydw = rne_bf16(rng.normal(0, 1, (M, cin)))
    c.bn_dw, c.bn_pw = bn_of(cin, rng), bn_of(cout, rng)
    c.piv = rng.normal(0, 0.3, cout).astype(np.float32)
    if M >= 3:
        c.ydw[1] = -8.0                                          # scale > 0.5, |shift| < 2: a == 0 in every channel
    if mode == "dgrad":
        c.g, c.y = rne_bf16(rng.normal(0, 0.1, (M, cout))), rne_bf16(rng.normal(0, 1, (M, cout)))
    for t in (c.ydw,) + ((c.g, c.y) if mode == "dgrad" else ()):
        if M >= 2:
            t[M - 1] = t[0]
    if mode == "fwd":
        c.op = act_operand(c.ydw, c.bn_dw)
        c.p = BcProduct(c.op, np.ascontiguousarray(c.wb.T))
        c.open = c.mask_undecided = None
    else:
        c.op = dy_operand(c.g, c.y, c.bn_pw)
        c.p = BcProduct(c.op, c.wb)
        c.open, c.mask_undecided = mask_of(c.ydw, c.bn_dw)
    c.rows_of = row_of_pixel(c.path, M)
    c.L = stat_depth(c.path, c.N)
    return c


def stat_terms(c, v):
    """(d, q) of the stored values v [M][N] (float64)"""
    if c.mode == "fwd":
        d = v - c.piv.astype(np.float64)
        return d, d * d
    return v, v * (c.ydw.astype(np.float64) - c.bn_dw[BN_MEAN].astype(np.float64))


def model(c, mutate=None):
    """numpy emulation of the kernel: bf16 operands, fp32 accumulation per k16 MFMA step in channel order, one bf16 rounding, the mask.
    Returns the stored values [M][N] float32.  mutate: a planted error (tests/test_bc_ref.py)."""
    rnd = trunc_bf16 if mutate == "trunc_operand" else rne_bf16
    bn_dw, bn_pw = c.bn_dw, c.bn_pw
    wb = trunc_bf16(c.w) if mutate == "trunc_weights" else c.wb
    if c.mode == "fwd":
        bn = bn_dw.copy()
        if mutate == "shift_plus_mean":
            bn[BN_MEAN] = -bn[BN_MEAN]
        A = act_operand(c.ydw, bn, rnd).v
        B = wb.T
    else:
        bn = bn_pw.copy()
        if mutate == "gmean_mean_swapped":
            bn[[BN_GMEAN, BN_MEAN]] = bn[[BN_MEAN, BN_GMEAN]]
        A = dy_operand(c.g, c.y, bn, rnd).v
        B = wb
    A, B = A.astype(np.float64), np.ascontiguousarray(B).astype(np.float64)
    K = A.shape[1]
    if mutate == "drop_last_k16":
        K -= 16
    if mutate == "block_stride_64" and c.K > 64:   # the second 64-channel block of the operand read at the first block's base + 64 rows
        A = A.copy()
        A[:, 64:128] = np.roll(A[:, 64:128], 1, axis=0)
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k0 in range(0, K, 16):
        acc = (acc.astype(np.float64) + A[:, k0:k0 + 16] @ B[k0:k0 + 16]).astype(np.float32)
    if mutate == "tile_starts_late" and c.M > 1:   # every row tile / group reads from one pixel further on
        acc = np.concatenate([acc[1:], acc[-1:]])
    out = rne_bf16(acc)
    if c.mode == "dgrad":
        open_ = c.open
        if mutate == "mask_other_chunk":           # the mask operand of the next 8-channel chunk
            open_ = np.roll(open_, -8, axis=1)
        if mutate == "mask_ge":
            open_ = np.ones_like(open_)
        out = np.where(open_, out, np.float32(0))
    return out


def model_part(c, v, mutate=None):
    """float32 model of `part` for the stored values v"""
    d, q = stat_terms(c, v.astype(np.float64))
    if mutate == "second_sum_beta" and c.mode == "dgrad":
        q = v.astype(np.float64) * (c.ydw.astype(np.float64) - c.bn_dw[BN_BETA].astype(np.float64))
    if mutate == "padding_counted" and c.M % 32:   # the clamped copies of the last pixel enter the sums
        pad = 32 - c.M % 32
        d, q = d.copy(), q.copy()
        d[-1] *= 1 + pad
        q[-1] *= 1 + pad
    return np.stack([sum_model(c.path, d, c.N), sum_model(c.path, q, c.N)], 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------------------
def smallest_M(pred, N, nct=256, start=1, stop=140000):
    for M in range(start, stop):
        if pred(l_plan(M, N, nct), M):
            return M
    raise ValueError("no such M")


E_LAYERS = [(32, 64), (64, 128), (128, 128)]
E_M = [1, 31, 32, 33, 255, 256, 257]
E_BIG_M = 65536 + 256 + 1          # 2057 groups on the capped grid of 256 x 8 waves: nine waves take a second group
# the (NB, KH) pairs exist in both modes: the four instantiations no MobileNet layer reaches, which the entry points accept all the same
E_OFF_NETWORK = [("fwd", 33, 64, 32), ("fwd", 33, 128, 64), ("dgrad", 33, 64, 32), ("dgrad", 33, 128, 64)]
L128_CASES = [("dgrad", 1, 128, 256), ("dgrad", 257, 128, 256), ("fwd", 1, 256, 128), ("fwd", 263, 256, 128)]
L_FWD_LAYERS = [(128, 256), (256, 256), (256, 512), (512, 512), (512, 1024), (1024, 1024)]
L_DGRAD_LAYERS = [(256, 256), (256, 512), (512, 512), (512, 1024), (1024, 1024)]   # N = cin a multiple of 256, K = cout of 128


def _l_seams():
    """(mode, M, cin, cout) at the seams of l_plan, each on the cheapest layer that shows it (the plan depends on M and N alone)"""
    out = []
    wide = ("fwd", 128, 1024)      # ncol = 4, K = 128
    for rt in (16, 24, 32, 40):
        out.append((wide[0], smallest_M(lambda p, M: p.RT == rt, 1024), *wide[1:]))
    m16 = smallest_M(lambda p, M: p.RT == 16 and M % 16 == 0 and p.nrt % 8, 1024)
    out += [(wide[0], m16 - 1, *wide[1:]), (wide[0], m16, *wide[1:]), (wide[0], m16 + 1, *wide[1:])]
    out.append((wide[0], smallest_M(lambda p, M: 128 <= p.RT <= 248 and p.RT % 32, 1024), *wide[1:]))
    out.append((wide[0], smallest_M(lambda p, M: p.RT == 256, 1024), *wide[1:]))              # ncol = 4: M > 15 872
    out.append(("fwd", smallest_M(lambda p, M: p.RT == 256, 256, start=60000), 128, 256))     # ncol = 1: M > 63 488
    out.append(("fwd", smallest_M(lambda p, M: p.rounds == 2, 256, start=65000), 128, 256))   # two rounds
    out.append(("dgrad", smallest_M(lambda p, M: p.RT == 16, 512), 512, 256))                 # ncol = 2, data gradient, RT = 16
    return out


def _cases():
    out = []
    for cin, cout in E_LAYERS:
        for mode in ("fwd", "dgrad"):
            out += [(mode, M, cin, cout) for M in E_M]
    out += [("fwd", E_BIG_M, 32, 64), ("dgrad", E_BIG_M, 32, 64)]
    out += E_OFF_NETWORK
    out += L128_CASES
    for cin, cout in L_FWD_LAYERS:
        out += [("fwd", 1, cin, cout), ("fwd", 257, cin, cout)]
    for cin, cout in L_DGRAD_LAYERS:
        out += [("dgrad", 1, cin, cout), ("dgrad", 257, cin, cout)]
    out += _l_seams()
    return list(dict.fromkeys(out))


CASES = _cases()
FAMILIES = ("short", "full")
SMALL_CASES = [c for c in CASES if c[1] * max(c[2], c[3]) <= 300 * 1024]   # what the CPU test emulates (the large M repeat the arithmetic)

# shapes the entry points refuse (cin, cout): forward, and data gradient
REFUSED_FWD = [(32, 32), (64, 64), (32, 128), (64, 256), (128, 32)]
REFUSED_DGRAD = [(32, 32), (64, 64), (32, 128), (64, 256), (32, 256)]


def case_id(case):
    return f"{case[0]}-M{case[1]}-{case[2]}x{case[3]}"


# ---------------------------------------------------------------------------------------------------------------------------------
# pointwise weight gradient (csrc/bc_wgrad.hip):  dW[co][ci] (+)= sum_m dy[m][co] a[m][ci]
#
# Both operands are the bf16 operands above, so either may be undecided: widen = delta_dy^T |a| + |dy|^T delta_a (+ their product).
# A workgroup owns one TN x TK tile and one slice of `rows` pixels: per chunk of CP pixels the k16 MFMA steps, split between KS waves
# whose accumulators are added through LDS in wave order; it stores its tile to scratch[slice][cout][cin].  The slices are folded onto dW
# in a fixed order - fold_rows_fast_body's tree (slices >= 16 and cin * cout <= 65536) or fold_rows_wide_body's serial order - which
# `fold` restates exactly: the scratch tiles folded in numpy must give dW bit for bit.
# Yardstick: the larger of conv_ref.chain32 over all M pixels (the serial chain) and `wg_model` (the kernel's own order), against float64,
# on at most WG_Y_ROWS output channels.  Criterion: |dW - (dw0 + f64)| <= (MARGIN * Y + 2^-24) (s + |dw0|) + widen.
# ---------------------------------------------------------------------------------------------------------------------------------
WG_INSTANCES = {(64, 32): (2, 1, 128, 2, 1, 4), (128, 64): (4, 2, 64, 4, 2, 1), (128, 128): (4, 4, 64, 4, 2, 1),
                (256, 128): (8, 4, 32, 4, 2, 1), (256, 256): (8, 8, 32, 4, 2, 1)}   # (TN, TK) -> <TN32, TK32, CP, WN, WK, KS>
WG_Y_ROWS = 32
WG_WIDENED_CAP = 0.20


def fold_fast_ok(rows, n):
    return n % 4 == 0 and n <= 65536 and rows >= 16


def wgrad_plan(M, cin, cout):
    """None where ttk_bc_pw_bwd_weight refuses"""
    if not shape_ok(cin, cout) or M < 1:
        return None
    TN, TK = min(cout, 256), min(cin, 256)
    if (TN, TK) not in WG_INSTANCES:
        return None
    inst = WG_INSTANCES[(TN, TK)]
    CP, KS = inst[2], inst[5]
    tiles = (cout // TN) * (cin // TK)
    slices = min(max(256 // tiles, 1), -(-M // (2 * CP)))
    rows = -(-(-(-M // slices)) // CP) * CP
    slices = -(-M // rows)
    return types.SimpleNamespace(TN=TN, TK=TK, CP=CP, KS=KS, inst=inst, tiles=tiles, slices=slices, rows=rows, cap=max(256 // tiles, 1),
                                 grid=tiles * slices, scratch_bytes=slices * cin * cout * 4,
                                 fold="fast" if fold_fast_ok(slices, cin * cout) else "wide",
                                 lds=max(2 * CP * (wg_pitch(TN) + wg_pitch(TK)), 8 * (TN // 32 // inst[3]) * (TK // 32 // inst[4]) * 16 * 64 * 4 if KS > 1 else 0))


def wg_pitch(T):
    return 64 if T == 32 else 2 * T + 64


def fold(tiles, out, fast, accumulate=True, skip_row=None):
    """the slice tiles[rows][n] (float32) folded onto out[n]: fast - fold_rows_fast_body (row group ty adds the rows ty, ty + 64, ... from
    zero, the 64 groups are folded by the LDS tree, `out` is added last); else fold_rows_wide_body (the rows in order, onto `out`).
    skip_row: a planted error"""
    rows = tiles.shape[0]
    t = [np.zeros_like(tiles[r]) if r == skip_row else tiles[r] for r in range(rows)]
    if fast:
        sm = []
        for ty in range(64):
            a = np.zeros(tiles.shape[1], np.float32)
            for r in range(ty, rows, 64):
                a = a + t[r]
            sm.append(a)
        step = 32
        while step >= 1:
            for ty in range(step):
                sm[ty] = sm[ty] + sm[ty + step]
            step //= 2
        return sm[0] + out if accumulate else sm[0]
    a = out.astype(np.float32) if accumulate else np.zeros(tiles.shape[1], np.float32)
    for v in t:
        a = a + v
    return a


def wg_model(plan, D, A, M, mutate=None):
    """the slice tiles [slices][rows of D][cin] (float32) in the kernel's order; D[co][M], A[M][ci] float64 values of the bf16 operands"""
    out = np.zeros((plan.slices, D.shape[0], A.shape[1]), np.float32)
    for s in range(plan.slices):
        m0, m1 = s * plan.rows, min((s + 1) * plan.rows, M)
        if mutate == "slice_starts_late" and s > 0:
            m0 += 1
        acc = [np.zeros(out.shape[1:], np.float32) for _ in range(plan.KS)]
        steps = list(range(m0, m1, 16))
        if mutate == "drop_last_k16" and s == plan.slices - 1:
            steps = steps[:-1]
        for i, k in enumerate(steps):
            e = min(k + 16, m1)
            w = i % plan.KS
            acc[w] = (acc[w].astype(np.float64) + D[:, k:e] @ A[k:e]).astype(np.float32)
        t = acc[0]
        for w in range(1, plan.KS):
            t = t + acc[w]
        out[s] = t
    return out


SALTS = 32                # input draws a case may try until its operands meet the caps (a property of the reference alone)


def _wg_inputs(M, cin, cout, family, salt):
    rng = np.random.default_rng([2, M, cin, cout, {"full": 0, "short": 1}[family], salt])
    bn_of = bn_full if family == "full" else bn_short
    c = types.SimpleNamespace(M=M, cin=cin, cout=cout, family=family, salt=salt, plan=wgrad_plan(M, cin, cout))
    c.ydw = rne_bf16(rng.normal(0, 1, (M, cin)))
    c.g, c.y = rne_bf16(rng.normal(0, 0.1, (M, cout))), rne_bf16(rng.normal(0, 1, (M, cout)))
    c.bn_dw, c.bn_pw = bn_of(cin, rng), bn_of(cout, rng)
    c.dw0 = rng.normal(0, 1, (cout, cin)).astype(np.float32)
    c.opD, c.opA = dy_operand(c.g, c.y, c.bn_pw), act_operand(c.ydw, c.bn_dw)
    rows, cols = c.opD.undecided.any(0).mean(), c.opA.undecided.any(0).mean()   # dW[co][ci] is widened by an undecided dy[:, co] or a[:, ci]
    c.caps_met = max(c.opD.undecided.mean(), c.opA.undecided.mean()) <= UNDECIDED_CAP and 1 - (1 - rows) * (1 - cols) <= WG_WIDENED_CAP
    return c


@functools.lru_cache(maxsize=4)
def wg_case(M, cin, cout, family):
    """the inputs of one weight-gradient case: the first of SALTS seeded draws whose operands meet the caps (the share of widened outputs
    grows with M - one undecided dy element widens a whole row of dW: at the slice cap of 32 -> 64, M = 65 281, not every draw stays
    under WG_WIDENED_CAP; in a tensor of fewer than 10^4 elements one undecided element is above UNDECIDED_CAP)"""
    for salt in range(SALTS):
        c = _wg_inputs(M, cin, cout, family, salt)
        if c.caps_met:
            break
    else:
        raise ValueError(f"no draw of {SALTS} meets the caps for {(M, cin, cout, family)}")
    D, A = c.opD.v.astype(np.float64).T, c.opA.v.astype(np.float64)
    p = types.SimpleNamespace(ref=D @ A, s=c.opD.abs.T @ c.opA.abs, floor=0.0)
    p.widen = c.opD.delta.T @ c.opA.abs + c.opD.abs.T @ c.opA.delta + c.opD.delta.T @ c.opA.delta
    rows = np.arange(cout) if cout <= WG_Y_ROWS else np.concatenate([np.arange(WG_Y_ROWS - 8), np.arange(cout - 8, cout)])
    chain = chain32(np.ascontiguousarray(c.opD.v.T[rows]), c.opA.v)
    tiles = wg_model(c.plan, D[rows], A, M)
    own = fold(tiles.reshape(c.plan.slices, -1), None, c.plan.fold == "fast", False).reshape(len(rows), cin).astype(np.float64)
    p.Y_chain = float(_err_over_s(chain, p.ref[rows], p.s[rows]).max())
    p.Y_own = float(_err_over_s(own, p.ref[rows], p.s[rows]).max())
    p.Y = max(p.Y_chain, p.Y_own)
    p.allowed = lambda: (MARGIN * p.Y + U) * p.s + p.widen
    p.widened_share = float((p.widen > 0).mean())
    c.p, c.D, c.A = p, D, A
    return c


def wg_onto(p, dw0):
    """the gradient accumulated onto dw0 (stem_ref.onto): reference dw0 + dW, scale s + |dw0|"""
    d = dw0.astype(np.float64)
    return types.SimpleNamespace(ref=p.ref + d, s=p.s + np.abs(d), Y=p.Y, widen=p.widen)


def wg_ratio(q, x):
    """worst |x - f64| / allowed over the elements, and the figure without widening as Product.ratio gives it; exact zeros where s == 0"""
    x = np.asarray(x, np.float64)
    err = np.abs(x - q.ref)
    allowed = (MARGIN * q.Y + U) * q.s + q.widen
    if not np.isfinite(x).all() or (err[allowed == 0] != 0).any():
        return float("inf"), float("inf")
    live = allowed > 0
    plain = (q.widen == 0) & (q.s > 0)
    if q.Y == 0 or not plain.any():   # (one pixel: a single exact product, no yardstick to divide by)
        return float((err[live] / allowed[live]).max()), 0.0
    return float((err[live] / allowed[live]).max()), float(((err - U * q.s)[plain] / (q.s[plain] * q.Y)).max())


def _wg_cases():
    out = []
    for cin, cout in [(32, 64), (64, 128), (128, 128), (128, 256), (256, 256)]:
        CP = wgrad_plan(1, cin, cout).CP
        out += [(M, cin, cout) for M in (1, CP - 1, CP, CP + 1, 2 * CP, 2 * CP + 1, 30 * CP, 32 * CP)]
    for cin, cout in [(32, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 1024), (1024, 1024)]:
        cap = wgrad_plan(1, cin, cout).cap
        M = next(M for M in range(1, 1 << 20) if wgrad_plan(M, cin, cout).slices == cap)
        out.append((M, cin, cout))
    return list(dict.fromkeys(out))


WG_CASES = _wg_cases()
WG_REFUSED = [(256, 128), (64, 64), (64, 32), (32, 32), (64, 256)]


def wg_id(case):
    return f"M{case[0]}-{case[1]}x{case[2]}"


# ---------------------------------------------------------------------------------------------------------------------------------
# depthwise 3x3, pad 1, stride 1 | 2 (csrc/bc_dw.hip): the host's tiling restated, the forward held bit for bit
#
# Forward.  a_in = relu(bf16(fl32(fma(sc, y, sh)) + skip)) (zero outside the image), then per output and channel nine fp32 fmas in
# (kh, kw) order from a zero accumulator, acc = fma(a_in, w, acc), and ONE bf16 rounding.  Both steps are emulated in float64 with a
# TwoSum residual per step (bf16 x fp32 is exact in float64): where every residual is zero the stored value must equal the emulation
# BIT FOR BIT (dw_fwd.exact); elsewhere it is held by the bracket of the float64 contraction with Y = the emulated chain itself.
# a_out must equal the emulated a_in bit for bit wherever it is decided.
# Statistics: workgroup row r = blockIdx / nslabs sums the tiles it walks (dw_tiles / dw_row_of_output); a thread adds ceil(npix / slots)
# values per tile, then the shuffle tree over the lanes KQ apart, then four waves: dw_stat_depth.
# ---------------------------------------------------------------------------------------------------------------------------------
K_BLOCK = 256
PIX_BUDGET = {False: 560, True: 512}    # kPixBudgetFwd / kPixBudgetBwd (128-byte pixels)
CARRY_REGS, COL_TILE_MIN_W, COL_TILE = 5, 48, 17
DW_WGS = 2


def dw_shape_ok(B, H, W, C, stride):
    return B > 0 and H > 0 and 0 < W <= 256 and 32 <= C <= 1024 and C & (C - 1) == 0 and stride in (1, 2)


def band_rows(Hgrid, Wstage, stride, backward, budget):
    stage_rows = budget // (Wstage + 2)
    if not backward:
        R = int((stage_rows - 3) / stride) + 1          # (C division: truncation towards zero)
    else:
        R = stage_rows - 2 if stride == 1 else 2 * (stage_rows - 2)
    return min(max(R, 1), Hgrid)


def dw_tiling(B, H, W, C, stride, backward):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    t = types.SimpleNamespace(SL=cbw(C), Ho=Ho, Wo=Wo)
    KQ = t.SL // 8
    t.pix_budget = PIX_BUDGET[backward] * 64 // t.SL
    t.NCT, t.TW = 1, Wo
    t.carry = (not backward) and (3 - stride) * (W + 2) * KQ <= CARRY_REGS * K_BLOCK
    if not t.carry and stride == 1 and W >= COL_TILE_MIN_W and COL_TILE < W:
        t.NCT = -(-W // COL_TILE)
        t.TW = -(-W // t.NCT)
    Wtile = t.TW if t.NCT > 1 else (Wo if backward else W)
    t.R = band_rows(H if backward else Ho, Wtile, stride, backward, t.pix_budget)
    t.nbands = -(-(H if backward else Ho) // t.R)
    t.nslabs = C // t.SL
    t.stage_rows = (t.R + 2 if stride == 1 else t.R // 2 + 2) if backward else (t.R - 1) * stride + 3
    t.NI = 1
    if t.nbands == 1:
        t.carry = False
    if t.nbands == 1 and t.NCT == 1:
        t.NI = min(max(t.pix_budget // (t.stage_rows * ((Wo if backward else W) + 2)), 1), B)
    t.tiles = -(-B // t.NI) * t.nbands * t.NCT
    t.rows = min(max(256 * DW_WGS // t.nslabs, 1), t.tiles)
    t.grid = t.rows * t.nslabs
    t.stage_pix = t.NI * t.stage_rows * ((t.TW if t.NCT > 1 else (Wo if backward else W)) + 2)
    t.lds = t.stage_pix * t.SL * 2 + ((9 + 4 * 9 + 6) if backward else (9 + 2 * 4)) * t.SL * 4
    t.over_budget = t.stage_pix > t.pix_budget
    return t


def dw_fwd_tiles(t, B):
    """per tile of the forward: (workgroup row, images n0:n1, output rows o0:o1, output columns x0:x1)"""
    out = []
    for k in range(t.tiles):
        row = next(r for r in range(t.rows) if t.tiles * r // t.rows <= k < t.tiles * (r + 1) // t.rows) if t.carry else k % t.rows
        tb, ct = divmod(k, t.NCT)
        ti, band = divmod(tb, t.nbands)
        x0 = ct * t.TW
        out.append((row, ti * t.NI, min(ti * t.NI + t.NI, B), band * t.R, min(band * t.R + t.R, t.Ho), x0, min(x0 + t.TW, t.Wo) if t.NCT > 1 else t.Wo))
    return out


def dw_row_of_output(t, B):
    """[B][Ho][Wo] workgroup row of every output pixel, and L of the statistics"""
    rows = np.full((B, t.Ho, t.Wo), -1)
    slots = K_BLOCK // (t.SL // 8)
    serial = np.zeros(t.rows, int)
    for row, n0, n1, o0, o1, x0, x1 in dw_fwd_tiles(t, B):
        assert (rows[n0:n1, o0:o1, x0:x1] == -1).all()
        rows[n0:n1, o0:o1, x0:x1] = row
        serial[row] += -(-((n1 - n0) * (o1 - o0) * (x1 - x0)) // slots)
    assert (rows >= 0).all()
    return rows, int(serial.max()) + int(np.log2(64 // (t.SL // 8))) + 4 + 1


def add32(a, b):
    """(lo, hi, inexact) of the float32 sum a + b (b bf16 values): fma32 with a unit factor"""
    return fma32(b, np.ones(b.shape[-1], np.float32), a)


def dw_a_in(y, bn, skip, mutate=None):
    """the block input [B][H][W][C] as an operand (bf16 values): relu(bf16(fl32(fma(sc, y, sh)) + skip))"""
    sh = shift_of(bn)
    if mutate == "skip_before_rounding" and skip is not None:   # fma(sc, y, sh + skip): one rounding instead of two
        lo, hi, ix = fma32(y, bn[BN_SCALE], (sh.astype(np.float64) + skip.astype(np.float64)))
        return _operand([relu(rne_bf16(lo)), relu(rne_bf16(hi))], ix)
    lo, hi, ix = fma32(y, bn[BN_SCALE], sh)
    if skip is not None:
        lo, _, ix1 = add32(lo, skip)
        _, hi, ix2 = add32(hi, skip)
        ix = ix | ix1 | ix2
    if mutate == "relu_before_rounding":                         # the sign of a value that rounds to -0 is lost only after the rounding:
        return _operand([np.abs(rne_bf16(np.maximum(lo, 0)))], ix)   # (numerically the same: the planted error is a no-op, asserted)
    return _operand([relu(rne_bf16(lo)), relu(rne_bf16(hi))], ix)


def dw_taps(a, stride, mutate=None):
    """[9][B][Ho][Wo][C] float64: tap (kh, kw) of every output pixel, zeros outside the image"""
    B, H, W, C = a.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if mutate == "swap_hw":                                      # H and W exchanged in the bounds and the row pitch
        flat = a.reshape(B, H * W, C)
        hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        idx = hh * H + ww
        ok = (ww < H) & (hh < W) & (idx < H * W)
        a = np.where(ok[None, :, :, None], flat[:, np.where(ok, idx, 0)], 0.0)
    pad = np.zeros((B, H + 2, W + 2, C), np.float64)
    pad[:, 1:H + 1, 1:W + 1] = a
    if mutate == "halo_wraps":                                   # the left halo column reads the last pixel of the previous row
        pad[:, 2:H + 1, 0] = a[:, :H - 1, W - 1]
    return np.stack([pad[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride] for kh in range(3) for kw in range(3)])


def dw_chain(taps, w):
    """the nine fmas in float64 with a TwoSum residual per step: (acc float32 [B][Ho][Wo][C], exact: every residual zero)"""
    acc = np.zeros(taps.shape[1:], np.float32)
    exact = np.ones(taps.shape[1:], bool)
    for t in range(9):
        p = taps[t] * w[:, t].astype(np.float64)
        c = acc.astype(np.float64)
        s = p + c
        bb = s - p
        exact &= ((p - (s - bb)) + (c - bb)) == 0
        acc = s.astype(np.float32)
    return acc, exact


@functools.lru_cache(maxsize=4)
def dw_case(B, H, W, C, stride, skip, family):
    """the first of SALTS seeded draws whose block input meets UNDECIDED_CAP (as pw_case)"""
    for salt in range(SALTS):
        c = _dw_case(B, H, W, C, stride, skip, family, salt)
        if c.a.undecided.mean() <= UNDECIDED_CAP:
            return c
    raise ValueError("no draw meets the caps")


def _dw_case(B, H, W, C, stride, skip, family, salt):
    rng = np.random.default_rng([3, B, H, W, C, stride, int(skip), {"full": 0, "short": 1}[family], salt])
    c = types.SimpleNamespace(B=B, H=H, W=W, C=C, stride=stride, skip=skip, family=family, salt=salt, t=dw_tiling(B, H, W, C, stride, False))
    c.Ho, c.Wo = c.t.Ho, c.t.Wo
    c.y = rne_bf16(rng.normal(0, 1, (B, H, W, C)))
    c.sk = rne_bf16(np.abs(rng.normal(0, 1, (B, H, W, C)))) if skip else None
    c.bn = (bn_full if family == "full" else bn_short)(C, rng)
    c.w = (rng.normal(0, 1, (C, 9)) * 0.3).astype(np.float32)
    c.piv = rng.normal(0, 0.5, C).astype(np.float32)
    if skip:                                                     # plant pixels where `skip` added before the fp32 rounding would show in bf16
        yc, kc = rne_bf16(rng.normal(0, 1, (1 << 21, 1))), rne_bf16(np.abs(rng.normal(0, 1, (1 << 21, 1))))
        one = np.float32([1.0])
        two = rne_bf16(add32(fma32(yc, c.bn[BN_SCALE][:1], shift_of(c.bn[:, :1]))[0], kc)[0])
        fused = rne_bf16(fma32(yc, c.bn[BN_SCALE][:1], shift_of(c.bn[:, :1]).astype(np.float64) + kc.astype(np.float64))[0])
        hit = np.where((two != fused)[:, 0] & (two > 0)[:, 0])[0][:min(4, B * H * W)]
        c.y.reshape(-1, C)[:len(hit), 0], c.sk.reshape(-1, C)[:len(hit), 0] = yc[hit, 0], kc[hit, 0]
        c.planted = len(hit)
        del one
    if B > 1:
        c.y[B - 1] = c.y[0]                                      # a copy of an image: the same bits come out
        if skip:
            c.sk[B - 1] = c.sk[0]
    c.a = dw_a_in(c.y, c.bn, c.sk)
    taps = dw_taps(c.a.v.astype(np.float64), stride)
    c.acc, c.exact = dw_chain(taps, c.w)
    c.exact &= ~dw_taps(c.a.undecided.astype(np.float64), stride).any(0)
    w64 = c.w.astype(np.float64).T.reshape(9, 1, 1, 1, C)
    p = types.SimpleNamespace(ref=(taps * w64).sum(0), s=(np.abs(taps) * np.abs(w64)).sum(0), floor=0.0)
    p.widen = (dw_taps(c.a.delta, stride) * np.abs(w64)).sum(0)
    p.Y = float(_err_over_s(c.acc.astype(np.float64), p.ref, p.s).max())
    p.allowed = lambda: (MARGIN * p.Y + U) * p.s + p.widen
    c.p = p
    c.want_a = skip and stride == 1
    return c


def dw_fwd_outside(c, v):
    """(elements outside: not the emulation's bits where it is exact, outside the bracket elsewhere; the share held bit for bit)"""
    v = np.ascontiguousarray(v, np.float32)
    want = rne_bf16(c.acc)
    bits_bad = c.exact & (v.view(np.uint32) != (want + np.float32(0)).view(np.uint32)) & ~((v == 0) & (want == 0) & (v.view(np.uint32) == 0))
    lo, hi = bracket(c.p)
    bad = np.where(c.exact, bits_bad, (v < lo) | (v > hi)) | ~np.isfinite(v) | ((c.p.s == 0) & (v.view(np.uint32) != 0))
    return int(bad.sum()), float(c.exact.mean())


# (B, H, W, C, stride, skip): every S x SKIP x SL x CARRY of bc_dw_fwd_k and the seams of `tiling` (tests/test_bc_ref.py asserts them)
DW_FWD_BASE = [
    (2, 11, 78, 64, 1), (2, 11, 79, 64, 1),      # SL = 64, stride 1: the last carried width | column tiles begin
    (1, 7, 158, 64, 2), (1, 7, 159, 64, 2),      # SL = 64, stride 2: the carry ends
    (1, 11, 158, 32, 1), (1, 11, 159, 32, 1),    # SL = 32, stride 1: the carry ends, column tiles
    (1, 40, 50, 32, 2), (3, 9, 9, 32, 2),        # SL = 32, stride 2: carried | one band, several images per tile
]
DW_FWD_CASES = [b + (s,) for b in DW_FWD_BASE for s in (False, True)] + [
    (2, 9, 78, 64, 1, True), (2, 10, 78, 64, 1, True),            # H one below | at a multiple of R = 5 (11: one past), carried
    (2, 28, 79, 64, 1, True), (2, 29, 79, 64, 1, False), (2, 30, 79, 64, 1, True), (1, 59, 79, 64, 1, False),   # column tiles AND bands: H = R - 1 | R | R + 1 | 2 R + 1, R = 29
    (1, 1, 159, 64, 2, False), (1, 3, 159, 64, 2, False), (1, 5, 159, 64, 2, True),   # plain bands (no carry, no column tiles) exist with R = 1 only (test_bc_ref): Ho = 1 | 2 | 3
    (1, 5, 256, 64, 1, True),                                     # W = 256: sixteen column tiles
    (1, 3, 185, 64, 2, False), (1, 4, 200, 64, 2, True), (1, 3, 256, 64, 2, False), (1, 4, 255, 64, 2, False),  # R clamped to 1, stage_rows = 3 over the budget
    (23, 5, 5, 64, 1, True), (5, 17, 17, 128, 1, True),           # nbands == 1, NI = 11 > 1, B no multiple of NI
    (1, 1, 1, 32, 1, False), (1, 1, 9, 64, 2, False), (2, 9, 1, 64, 1, True),   # a pixel, a row, a column
    (2, 5, 5, 1024, 1, True), (7, 6, 79, 1024, 1, False),         # 16 slabs of 32 rows; 35 tiles per slab on 32 rows: a workgroup walks
]
DW_REFUSED = [(1, 5, 257, 64, 1), (1, 5, 5, 48, 1), (1, 5, 5, 2048, 1), (1, 5, 5, 16, 1), (1, 5, 5, 64, 3)]


def dw_id(case):
    return "x".join(str(int(v)) for v in case)


# ---------------------------------------------------------------------------------------------------------------------------------
# fused pointwise backward (csrc/bc_fused.hip: bc_bwd_fused_k<TN32, TK32, CP>): the data gradient and the weight gradient of the three
# early layers from one pass over the pixels.  One workgroup per slice of `rows` pixels (fused_plan); row `slice` of `part` holds the
# sums of its pixels: a wave owns one (channel block, 32-pixel group) unit of a chunk of CP pixels, a lane adds NI values per chunk, then
# the shuffle tree, then the CP / 32 units of a channel block.  The data gradient is the pointwise one (same operands, same criterion, and
# bitwise ttk_bc_pw_bwd_data's); dW is held to wg_case's criterion (Y: the serial chain over all M pixels dominates every tiling's own
# order) and to the numpy fold of the scratch bit for bit: fold_rows_fast_body's tree from 16 slices on, fold_partials_k's serial order below.
# ---------------------------------------------------------------------------------------------------------------------------------
FUSED_INSTANCES = {(32, 64): (2, 1, 128), (64, 128): (4, 2, 64), (128, 128): (4, 4, 32)}   # (cin, cout) -> <TN32, TK32, CP>


def fused_plan(M, cin, cout):
    if (cin, cout) not in FUSED_INSTANCES or M < 1:
        return None
    inst = FUSED_INSTANCES[(cin, cout)]
    CP = inst[2]
    slices = min(256, -(-M // (2 * CP)))
    rows = -(-(-(-M // slices)) // CP) * CP
    slices = -(-M // rows)
    OC = 32 if cin < 64 else 64
    ppi = 64 // (OC // 8)
    depth = (rows // CP) * (32 // ppi) + int(np.log2(ppi)) + CP // 32 + 1
    TN, TK = cout, cin
    WN, WK = (4 if inst[0] >= 4 else 2), (2 if inst[1] >= 2 else 1)
    KS = 8 // (WN * WK)
    bufs, redw = 2 * CP * (wg_pitch(TN) + 2 * wg_pitch(TK)), (8 * (inst[0] // WN) * (inst[1] // WK) * 16 * 64 * 4 if KS > 1 else 0)
    return types.SimpleNamespace(inst=inst, CP=CP, slices=slices, rows=rows, depth=depth, scratch_bytes=slices * cin * cout * 4,
                                 fold="fast" if fold_fast_ok(slices, cin * cout) else "plain", lds=max(bufs, redw) + TK * TN * 2 + 3 * TK * 4 + 8 * 4 * OC * 16)


@functools.lru_cache(maxsize=2)
def fused_case(M, cin, cout, family):
    """wg_case's inputs with a weight matrix: .dg the data-gradient product, .open / .mask_undecided its mask"""
    c = wg_case(M, cin, cout, family)
    f = types.SimpleNamespace(c=c, plan=fused_plan(M, cin, cout))
    rng = np.random.default_rng([4, M, cin, cout])
    f.w = (rng.normal(0, 1, (cout, cin)) / np.sqrt(cin)).astype(np.float32)
    f.dg = BcProduct(c.opD, rne_bf16(f.w))
    f.open, f.mask_undecided = mask_of(c.ydw, c.bn_dw)
    return f


def _fused_cases():
    out = []
    for (cin, cout), (_, _, CP) in FUSED_INSTANCES.items():
        cap = next(M for M in range(1, 1 << 20) if fused_plan(M, cin, cout).slices == 256)
        out += [(M, cin, cout) for M in (1, CP - 1, CP, CP + 1, 2 * CP, 2 * CP + 1, 30 * CP, 32 * CP, cap)]
    return out


FUSED_CASES = _fused_cases()


# ---------------------------------------------------------------------------------------------------------------------------------
# depthwise data gradient and fused weight gradient (bc_dw_bwd_k<S, SL, LEAN>)
#
# dy = bf16(fma(ga, g, fma(gb, y, c0))) is staged (zero outside); per input pixel G = fma(dy_t, w_t, G) over the taps t = 0..8 in order
# from zero (stride 2: the taps of the pixel's parity class, the others contribute nothing), + skip_grad (one fp32 addition), masked by
# a_in > 0 (a_in given, or recomputed as the forward formed it), ONE bf16 rounding.  Emulated like the forward: bit for bit where every
# TwoSum residual is zero and no tap is undecided, the bracket elsewhere.  dW[c][t] = sum over the input pixels of dy_t a_in: a thread's
# serial sum, the shuffle tree, four waves, then workgroup rows (folded, or float atomics) - held to (4 Y + 2^-24) s + widening with Y the
# serial fp32 chain over all pixels (it dominates the tree orders; MARGIN covers the order as in conv_ref).
# ---------------------------------------------------------------------------------------------------------------------------------
def dw_taps_t(dy, H, W, stride, mutate=None):
    """[9][B][H][W][C] float64: dy at the output pixel that tap t of every INPUT pixel points at, zero where there is none"""
    B, Ho, Wo, C = dy.shape
    out = np.zeros((9, B, H, W, C), np.float64)
    for kh in range(3):
        for kw in range(3):
            hi, wi = np.arange(H) + 1 - kh, np.arange(W) + 1 - kw
            okh = (hi >= 0) & (hi % stride == 0) & (hi // stride < Ho)
            okw = (wi >= 0) & (wi % stride == 0) & (wi // stride < Wo)
            if mutate == "parity":                               # the column parity classes of stride 2 exchanged
                okw = (wi >= 0) & ((wi + 1) % stride == 0) & (wi // stride < Wo)
            sub = dy[:, (hi // stride)[okh]][:, :, (wi // stride)[okw]]
            out[kh * 3 + kw][np.ix_(np.arange(B), np.where(okh)[0], np.where(okw)[0])] = sub
    return out


DW_FORMS = ("lean", "skip", "skip_in")   # no residual operands | skip_prev + skip_grad (stride 1) | skip_prev alone


@functools.lru_cache(maxsize=2)
def dw_bwd_case(B, H, W, C, stride, form, family):
    """the first of SALTS seeded draws whose operands meet UNDECIDED_CAP and whose data gradient meets WIDENED_CAP (as pw_case)"""
    for salt in range(SALTS):
        c = _dw_bwd_case(B, H, W, C, stride, form, family, salt)
        if max(c.dy.undecided.mean(), c.a.undecided.mean()) <= UNDECIDED_CAP and (c.p.widen > 0).mean() <= WIDENED_CAP \
                and (c.q.widen > 0).mean() <= WG_WIDENED_CAP:
            return c
    raise ValueError("no draw meets the caps")


def _dw_bwd_case(B, H, W, C, stride, form, family, salt):
    rng = np.random.default_rng([5, B, H, W, C, stride, DW_FORMS.index(form), {"full": 0, "short": 1}[family], salt])
    bn_of = bn_full if family == "full" else bn_short
    c = types.SimpleNamespace(B=B, H=H, W=W, C=C, stride=stride, form=form, family=family, salt=salt, t=dw_tiling(B, H, W, C, stride, True))
    c.Ho, c.Wo = c.t.Ho, c.t.Wo
    c.yprev = rne_bf16(rng.normal(0, 1, (B, H, W, C)))
    c.sk = rne_bf16(np.abs(rng.normal(0, 1, (B, H, W, C)))) if form != "lean" else None
    c.sg = rne_bf16(rng.normal(0, 0.1, (B, H, W, C))) if form == "skip" else None
    c.bn_prev, c.bn_dw = bn_of(C, rng), bn_of(C, rng)
    c.w = (rng.normal(0, 1, (C, 9)) * 0.3).astype(np.float32)
    c.g, c.ydw = rne_bf16(rng.normal(0, 0.1, (B, c.Ho, c.Wo, C))), rne_bf16(rng.normal(0, 1, (B, c.Ho, c.Wo, C)))
    c.dw0 = rng.normal(0, 1, (C, 9)).astype(np.float32)
    if B > 1:                                                    # a copy of an image: the same bits come out
        for x in (c.yprev, c.sk, c.sg, c.g, c.ydw):
            if x is not None:
                x[B - 1] = x[0]
    c.a = dw_a_in(c.yprev, c.bn_prev, c.sk)
    c.dy = dy_operand(c.g.reshape(-1, C), c.ydw.reshape(-1, C), c.bn_dw)
    rs = lambda x: x.reshape(B, c.Ho, c.Wo, C)
    taps = dw_taps_t(rs(c.dy.v.astype(np.float64)), H, W, stride)
    tdelta, tabs = dw_taps_t(rs(c.dy.delta), H, W, stride), dw_taps_t(rs(c.dy.abs), H, W, stride)
    # ---- data gradient
    acc, exact = dw_chain(taps, c.w)
    ref = (taps * c.w.astype(np.float64).T.reshape(9, 1, 1, 1, C)).sum(0)
    s = (tabs * np.abs(c.w.astype(np.float64)).T.reshape(9, 1, 1, 1, C)).sum(0)
    if c.sg is not None:
        lo, hi, ix = add32(acc, c.sg)
        acc, exact = lo, exact & ~ix
        ref, s = ref + c.sg, s + np.abs(c.sg)
    c.acc, c.exact = acc, exact & ~(tdelta != 0).any(0)
    p = types.SimpleNamespace(ref=ref, s=s, floor=0.0)
    p.widen = (tdelta * np.abs(c.w.astype(np.float64)).T.reshape(9, 1, 1, 1, C)).sum(0)
    p.Y = float(_err_over_s(acc.astype(np.float64), ref, s).max())
    p.allowed = lambda: (MARGIN * p.Y + U) * p.s + p.widen
    c.p = p
    c.open, c.mask_undecided = c.a.lo > 0, (c.a.lo > 0) != (c.a.hi > 0)
    # ---- weight gradient [C][9]
    a64 = c.a.v.astype(np.float64)
    q = types.SimpleNamespace(ref=(taps * a64).sum((1, 2, 3)).T, s=(tabs * c.a.abs).sum((1, 2, 3)).T)
    q.widen = ((tdelta * c.a.abs).sum((1, 2, 3)) + (tabs * c.a.delta).sum((1, 2, 3))).T
    chain = np.zeros((9, C), np.float32)
    tp, ap = taps.reshape(9, -1, C), a64.reshape(-1, C)
    for m in range(ap.shape[0]):
        chain = (chain + tp[:, m] * ap[m]).astype(np.float32)
    q.Y = float(_err_over_s(chain.T.astype(np.float64), q.ref, q.s).max())
    c.q = q
    return c


def dw_bwd_outside(c, v):
    """elements of the stored g_prev outside: closed -> +0; open -> the emulation's bits where it is exact, the bracket elsewhere"""
    v = np.ascontiguousarray(v, np.float32)
    zero = v.view(np.uint32) == 0
    want = rne_bf16(c.acc)
    lo, hi = bracket(c.p)
    inside = np.where(c.exact, (v == want) & (np.signbit(v) == np.signbit(want)) | ((want == 0) & zero), (v >= lo) & (v <= hi)) & np.isfinite(v)
    inside &= ~((c.p.s == 0) & ~zero)
    bad = np.where(c.mask_undecided, ~(inside | zero), np.where(c.open, ~inside, ~zero))
    return int(bad.sum()), float((c.exact | ~c.open).mean())


def dw_wgrad_model(c, skip_row=None):
    """numpy emulation of the fused weight gradient: per workgroup row (dw_bwd_rows) the float32 serial sum of dy_t a_in over its pixels,
    the rows then folded as the launch folds them (bc_ref.fold; skip_row: a planted error) -> dW[C][9]"""
    t = c.t
    rows_of, _ = dw_bwd_rows(t, c.B, c.H, c.W, c.stride)
    taps = dw_taps_t(c.dy.v.astype(np.float64).reshape(c.B, c.Ho, c.Wo, c.C), c.H, c.W, c.stride).reshape(9, -1, c.C)
    a = c.a.v.astype(np.float64).reshape(-1, c.C)
    tiles = np.zeros((t.rows, c.C, 9), np.float32)
    for m, r in enumerate(rows_of.reshape(-1)):
        tiles[r] = (tiles[r] + (taps[:, m] * a[m]).T).astype(np.float32)
    return fold(tiles.reshape(t.rows, -1), None, fold_fast_ok(t.rows, 9 * c.C), False, skip_row).reshape(c.C, 9)


def dw_bwd_rows(t, B, H, W, stride):
    """([B][H][W] workgroup row of every input pixel, L): tile k goes to row k % rows; a thread adds at most ceil(npix / slots) (+ 3: the
    four parity classes of stride 2 each round up) values per tile"""
    rows = np.full((B, H, W), -1)
    slots = K_BLOCK // (t.SL // 8)
    serial = np.zeros(t.rows, int)
    for k in range(t.tiles):
        tb, ct = divmod(k, t.NCT)
        ti, band = divmod(tb, t.nbands)
        n0, n1, h0, h1 = ti * t.NI, min(ti * t.NI + t.NI, B), band * t.R, min(band * t.R + t.R, H)
        x0, x1 = (ct * t.TW, min(ct * t.TW + t.TW, W)) if t.NCT > 1 else (0, W)
        assert (rows[n0:n1, h0:h1, x0:x1] == -1).all()
        rows[n0:n1, h0:h1, x0:x1] = k % t.rows
        serial[k % t.rows] += -(-((n1 - n0) * (h1 - h0) * (x1 - x0)) // slots) + (3 if stride == 2 else 0)
    assert (rows >= 0).all()
    return rows, int(serial.max()) + int(np.log2(64 // (t.SL // 8))) + 4 + 1


# (B, H, W, C, stride, form): every S x SL x LEAN of bc_dw_bwd_k and the seams of `tiling`
DW_BWD_CASES = [
    (2, 9, 47, 64, 1, "lean"), (2, 9, 48, 64, 1, "lean"), (2, 9, 48, 64, 1, "skip"),       # column tiles begin at W = 48
    (1, 9, 50, 64, 1, "skip"), (1, 9, 52, 64, 1, "lean"),                                  # a narrower last column tile | an even split
    (2, 3, 256, 64, 1, "skip"),                                                            # W = 256: 32 tiles on 32 rows (the fast fold)
    (2, 7, 10, 64, 2, "lean"), (2, 10, 7, 64, 2, "skip_in"), (3, 8, 6, 64, 2, "lean"), (2, 9, 5, 64, 2, "skip_in"),   # the four parities
    (1, 5, 9, 32, 2, "lean"), (1, 5, 9, 32, 2, "skip_in"), (2, 9, 9, 32, 1, "lean"), (2, 9, 9, 32, 1, "skip"),        # SL = 32; R clamped to an odd H
    (1, 40, 50, 32, 1, "lean"),                                                            # SL = 32 column tiles of 40 rows
    (2, 25, 48, 64, 1, "lean"), (2, 26, 48, 64, 1, "skip"), (2, 27, 48, 64, 1, "lean"), (1, 53, 48, 64, 1, "skip"),    # column tiles AND bands: H = R - 1 | R | R + 1 | 2 R + 1, R = 26
    (2, 7, 47, 64, 1, "skip"), (2, 8, 47, 64, 1, "lean"), (1, 17, 47, 64, 1, "skip"),      # plain bands, stride 1: H = R - 1 | R | 2 R + 1, R = 8 (9: above)
    (1, 15, 94, 64, 2, "lean"), (1, 16, 94, 64, 2, "skip_in"), (1, 17, 94, 64, 2, "lean"), (1, 33, 94, 64, 2, "skip_in"),   # plain bands, stride 2: R = 16
    (1, 1, 1, 64, 1, "lean"), (1, 1, 9, 64, 2, "lean"), (2, 9, 1, 64, 1, "skip"),          # a pixel, a row, a column
    (23, 5, 5, 128, 1, "skip"), (2, 5, 5, 1024, 1, "skip"), (7, 6, 79, 1024, 1, "lean"),   # NI > 1; 16 slabs; 35 tiles on 32 rows
]


def dwb_id(case):
    return "x".join(str(v) for v in case)
