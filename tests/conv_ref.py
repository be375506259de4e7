"""Float64 reference, yardstick and cases of the implicit-GEMM convolutions of the ResNet18 variant (csrc/conv.hip; the GATHER / CONV
forms of pw16_k and pw16_wgrad_k in csrc/pwconv_f16.hip).  Plain numpy on the CPU; tests/test_conv_rows_gpu.py compares the kernels
with it through the C ABI, tests/test_conv_ref.py pins it on its own without a GPU.

Reference.  An explicit im2col of the channels-last activation a[B][H][W][Cin] for (k, stride, pad = k // 2): `gather_index` lists, per
GEMM row (a pixel of the grid) and tap, the flat source pixel the tap points at (or -1: padding / a tap that misses the stride grid), in
the forward form (grid = output, source = input) and in the transposed form of the data gradient (grid = input, source = output).  The
contraction order is (tap, channel) with the channel fastest - the order of the kernels.  From it, in float64, of the float32 inputs:
    y    = im2col(a) @ W_f                      W_f[(t, ci)][co] = w[co][ci][t]
    g_in = im2col^T(dy) @ W_b  (raw | masked)   W_b[(t, co)][ci] = w[co][ci][t]      dy = ga*(g - gmean) + gb*(y - mean)
    dw   = dy^T @ im2col(a)                     [co][(t, ci)], contraction over the output pixels
and the per-element scale s = sum |operand_a| * |operand_b| over the same contraction.  Where operand_a is dy, which the kernels form in
float32 on load (or ttk_bn_bwd_apply does, once), the scale takes D = |ga|(|g| + |gmean|) + |gb|(|y| + |mean|) in place of |dy|: the
device rounds every term of dy, and the cancellation between the terms is not the kernels' error.

Yardstick.  `chain32` - one float32 fma per contraction step - and `split_model` - the three-product fp16 split of csrc/split16.h
(h_a l_b + l_a h_b + h_a h_b per k16 block, each block exact, added to a float32 accumulator; after tools/exp/split16.py) - are evaluated
on the case's OWN matrices.  E(x) = max over elements |x - f64| / s; Y = max(E(chain32), E(split_model)) over the whole product.

Criterion (tests/test_conv_rows_gpu.py), for every element of every row:
    |x - f64| <= (MARGIN * Y + 2^-24) * s + floor,      x == 0 exactly where s == 0
  * MARGIN = 4 is a margin over a yardstick computed on the CPU, not fitted to the kernel: it allows for the MFMA's own accumulation
    inside a k16 block (the model treats a block as exact), for the slice / atomic summation order of the weight gradient, and for the
    luck of one random draw of rounding errors (Y is the maximum over a few thousand elements; another correct summation order of the same
    elements has another maximum).  Every mutation of tests/test_conv_ref.py lands more than 10x outside it.
  * 2^-24 s: the final float32 rounding of the output (|y| <= s).
  * floor: the range term of the split (tests/test_range_stress_gpu.py): an element under 2^-17 of its tensor's bound keeps
    an absolute error of 2^-25 / S only; floor = floor_a @ |b| + |a| @ floor_b through the same im2col.
  * The yardstick Y is the product's maximum, each ROW of the kernel's output is held to it: a single row of the yardstick may by luck
    carry no rounding error at all (a row with one non-zero product), a row of the kernel output is never allowed more than the worst row
    of the yardstick, times MARGIN.
Masked data gradient: the mask is [pre > 0], pre = scale*(mask_y - mean) + beta formed in float32 on the device.  An element is UNDECIDED
when |pre64| <= 2^-20 * (|scale|(|mask_y| + |mean|) + |beta|): there the device may take either side - the output must be 0 or within the
bound of the unmasked value.  Elsewhere pre64 decides.  At most UNDECIDED_CAP of a case's elements may be undecided (the seeds are chosen so;
tests/test_conv_ref.py asserts it from the reference alone).

Inputs (make_case), seeded by the case: post-ReLU activations with two whole zero channels and two exactly-zero pixels, He-scaled weights,
BatchNorm blocks as tests/test_conv_gpu.py draws them (GMEAN != 0: a padded tap formed as ga*(0 - gmean) instead of 0 shows), bounds with
that file's slack of 1.7."""
import functools
import types

import numpy as np

U = 2.0 ** -24            # unit roundoff of float32
MARGIN = 4.0              # see the module docstring
SLACK = 1.7               # looseness of the operand bounds (tests/test_conv_gpu.py: LOOSE)
UNDECIDED_CAP = 1e-3      # largest share of undecided mask elements in one case
UNDECIDED_REL = 2.0 ** -20
BN_SCALE, BN_BETA, BN_MEAN, BN_RSTD, BN_GA, BN_GB, BN_GMEAN, BN_AUX = range(8)  # rows of a BatchNorm block (include/ttk.h)
AUX_ACT_BOUND, AUX_DY_BOUND, AUX_GMAX = range(3)

# (B, H, W, Cin, Cout, k, stride); M = B*Ho*Wo rows forward, B*H*W rows in the data gradient.  Tiles of the forward / data-gradient
# GEMM (TTK_CONV_TILES): Nout = 64 mod 128 -> 128x64, 128 mod 256 -> 256x128, 0 mod 256 -> 128x256 (Nout = Cout forward, Cin backward).
# Weight-gradient tiles (launch_conv_wgrad16): Cout = 64 and 576 columns -> 64x192, Cout = 64 otherwise -> 64x256, Cout >= 128 -> 128x256.
CASES = [
    # ---- stride 1, k = 3: the three tile forms with M below / exactly / one past a tile, not square
    (2, 4, 16, 64, 64, 3, 1),      # M = 128: exactly one 128x64 tile forward and backward; 64x192 weight-gradient tiles (3 of them)
    (3, 1, 43, 64, 64, 3, 1),      # M = 129: one tile + 1 row; H = 1 (kh = 0, 2 always padded); TWO weight-gradient slices, ragged last (33 rows)
    (2, 8, 16, 128, 128, 3, 1),    # M = 256: exactly one 256x128 tile; 128x256 weight-gradient tiles, 1152 columns = 4.5 tiles
    (1, 257, 1, 128, 128, 3, 1),   # M = 257: 256x128 tile + 1 row; W = 1 (kw = 0, 2 always padded); three slices
    (1, 16, 8, 256, 256, 3, 1),    # M = 128: exactly one 128x256 tile
    (1, 4, 9, 512, 512, 3, 1),     # the one 512: M = 36 below a 128x256 tile, two column tiles; K * Nout = 2.36 M
    (2, 5, 3, 256, 64, 3, 1),      # 64x256 weight-gradient tiles (Cout = 64, Cin = 256); forward 128x64, backward 128x256, M = 30
    (1, 7, 20, 64, 128, 3, 1),     # M = 140 below a 256x128 tile forward (Nout = 128), 128x64 + 12 rows backward (Nout = 64)
    # ---- stride 1, k = 1
    (1, 3, 43, 256, 256, 1, 1),    # M = 129: 128x256 tile + 1 row; 1x1 weight gradient keeps the atomics (no scratch)
    (2, 1, 6, 64, 64, 1, 1),       # H = 1
    (2, 5, 1, 64, 128, 1, 1),      # W = 1
    # ---- stride 2, k = 3: (H, W) in the four parity combinations, not square - parity classes of unequal size, the upper-bound test
    # of the transposed gather decides on every even side
    (2, 7, 10, 64, 128, 3, 2),     # odd x even
    (2, 10, 7, 128, 256, 3, 2),    # even x odd
    (3, 8, 6, 64, 64, 3, 2),       # even x even
    (2, 9, 5, 256, 512, 3, 2),     # odd x odd
    (1, 6, 4, 64, 192, 3, 2),      # Cout = 192 in the data gradient (Kc = 192: six k32 steps per tap)
    # ... and the degenerate grids: empty parity classes (ctile[c] == ctile[c + 1])
    (1, 1, 1, 64, 128, 3, 2),      # only class (0,0): one row
    (2, 1, 6, 128, 128, 3, 2),     # H = 1: no odd rows - classes (1,1), (1,0) empty
    (2, 6, 1, 64, 64, 3, 2),       # W = 1: no odd columns - classes (1,1), (0,1) empty
    (1, 2, 2, 128, 256, 3, 2),     # every class one pixel
    (2, 2, 3, 64, 128, 3, 2),      # class (1,1) 1 pixel, (1,0) 2, (0,1) 1, (0,0) 2 per image
    # ---- stride 2, k = 1: memset + the (even, even) class only; the odd pixels of the data gradient are exact zeros
    (2, 7, 10, 64, 128, 1, 2),
    (2, 10, 7, 128, 256, 1, 2),
    (3, 8, 6, 64, 128, 1, 2),
    (2, 9, 5, 256, 512, 1, 2),
    (1, 1, 1, 64, 128, 1, 2),
    (2, 1, 6, 128, 256, 1, 2),
    (2, 6, 1, 64, 128, 1, 2),
    (1, 2, 2, 128, 256, 1, 2),
    (2, 2, 3, 64, 128, 1, 2),
    # ---- channel counts conv_shape_ok admits beside the ResNet's (no data gradient: Cin % 64 != 0 is refused)
    (2, 12, 17, 32, 64, 3, 1),     # Cin = 32, k = 3: 288 weight-gradient columns = one 256-column tile + 32; kpt = 1 (a tap = one k32 step)
    (2, 6, 5, 32, 64, 1, 2),       # Cin = 32, k = 1: 32 columns in a 256-column tile, K = 32 = a single k32 step
    (2, 5, 7, 96, 192, 3, 1),      # Cin = 96: 864 columns = three full tiles + 96; Cout = 192: ragged second 128-row tile; Nout = 192 -> 128x64
]
MULTI_SLICE_CASE = (3, 1, 43, 64, 64, 3, 1)  # smallest M (129) with two slices: wgrad_slices caps the count at ceil(M / 128)
MULTI_SLICE_COUNT = 2


def out_hw(H, W, k, stride):
    pad = k // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def has_dgrad(case):
    return case[3] % 64 == 0  # ttk_conv_bwd_data refuses other input channel counts


# ---------------------------------------------------------------------------------------------------------------------------------
# the split arithmetic (after tools/exp/split16.py; csrc/split16.h)
# ---------------------------------------------------------------------------------------------------------------------------------
def pow2_scale(bound):
    """S = 2^(14 - floor(log2 bound)): bound * S in [2^14, 2^15); 1 for an unknown (zero) bound (split16.h)"""
    if not float(bound) > 0.0:
        return 1.0
    return 2.0 ** (14 - int(np.floor(np.log2(float(bound)))))


def floor_abs(x, bound):
    """absolute error floor of every element of x under the split with `bound`: 0 where all 22 bits are kept"""
    S = pow2_scale(bound)
    return np.where(np.abs(x) * S >= 2.0 ** -3, 0.0, 2.0 ** -25 / S)


def split_f16_bits(x, S):
    """(h, l) as float16 arrays: h = fp16(x S), l = fp16(x S - h), float32 arithmetic as on the device"""
    xs = x.astype(np.float32) * np.float32(S)
    h = xs.astype(np.float16)
    l = (xs - h.astype(np.float32)).astype(np.float16)
    return h, l


def split_f16(x, S):
    h, l = split_f16_bits(x, S)
    return h.astype(np.float64), l.astype(np.float64)


def mfma_acc(terms, kblk=16):
    """terms: [(A[M,K], B[K,N]), ...] piece products, accumulated per k-block exactly, then added (float32 rounding) to the accumulator"""
    M, K = terms[0][0].shape
    acc = np.zeros((M, terms[0][1].shape[1]), np.float32)
    for k0 in range(0, K, kblk):
        for a, b in terms:
            acc = (acc.astype(np.float64) + a[:, k0:k0 + kblk] @ b[k0:k0 + kblk, :]).astype(np.float32)
    return acc.astype(np.float64)


def split_model(A, B, bound_a, bound_b, drop_low=None):
    """A[M,K] @ B[K,N] as the split kernels compute it.  drop_low = (row, k0, k1): the low piece of A[row, k0:k1] is lost (a mutation)."""
    Sa, Sb = pow2_scale(bound_a), pow2_scale(bound_b)
    ha, la = split_f16(A, Sa)
    hb, lb = split_f16(B, Sb)
    if drop_low is not None:
        row, k0, k1 = drop_low
        la[row, k0:k1] = 0.0
    acc = mfma_acc([(ha, lb), (la, hb), (ha, hb)]) / (Sa * Sb)
    return acc.astype(np.float32).astype(np.float64)


def chain32(A, B):
    """A[M,K] @ B[K,N], one float32 fma per contraction step (vectorised over (M, N))"""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in range(A.shape[1]):
        acc = (acc + A64[:, k:k + 1] * B64[k:k + 1, :]).astype(np.float32)  # float32 + float64 -> float64: a single rounding
    return acc.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# im2col
# ---------------------------------------------------------------------------------------------------------------------------------
def gather_index(B, Hs, Ws, Hg, Wg, k, stride, transposed, mutate=None):
    """idx[B*Hg*Wg][k*k]: flat pixel (n*Hs + sh)*Ws + sw of the [B][Hs][Ws] source that tap (kh, kw) of grid pixel (n, gh, gw) reads, -1
    where it contributes zero (conv_geom.h).  Mutations (tests/test_conv_ref.py): "wrap" - the transposed gather without its upper-bound
    test (sh == Hs reads the next image's row 0, the last image its own last row); "swap" - Hs and Ws
    exchanged in the bounds and the row pitch."""
    pad = k // 2
    n, gh, gw = np.meshgrid(np.arange(B), np.arange(Hg), np.arange(Wg), indexing="ij")
    n, gh, gw = n.reshape(-1, 1), gh.reshape(-1, 1), gw.reshape(-1, 1)
    kh, kw = np.divmod(np.arange(k * k), k)
    kh, kw = kh[None, :], kw[None, :]
    if not transposed:
        sh, sw = gh * stride - pad + kh, gw * stride - pad + kw
        ok = np.ones(sh.shape, bool)
    else:
        th, tw = gh + pad - kh, gw + pad - kw
        ok = (th >= 0) & (tw >= 0) & (th % stride == 0) & (tw % stride == 0)
        sh, sw = th // stride, tw // stride
    Hb, Wb = (Ws, Hs) if mutate == "swap" else (Hs, Ws)
    if mutate == "wrap":
        inside = (sh >= 0) & (sw >= 0) & (sh <= Hs) & (sw < Ws)
        flat = (n * Hs + sh) * Ws + sw
        flat = np.where(flat >= B * Hs * Ws, (n * Hs + Hs - 1) * Ws + sw, flat)
    else:
        inside = (sh >= 0) & (sw >= 0) & (sh < Hb) & (sw < Wb)
        flat = np.clip(n * Hs * Ws + sh * Wb + sw, 0, B * Hs * Ws - 1)
    return np.where(ok & inside, flat, -1)


def im2col(x, idx, fill=None):
    """x[pixels][C] gathered to [rows][taps*C] (channel fastest); taps with idx == -1 read zeros, or the row `fill`[C] (a mutation)"""
    C = x.shape[1]
    src = np.concatenate([x, np.zeros((1, C), x.dtype) if fill is None else fill.reshape(1, C).astype(x.dtype)], 0)
    return src[np.where(idx < 0, x.shape[0], idx)].reshape(idx.shape[0], idx.shape[1] * C)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def bn_block(C, rng):
    """as tests/test_conv_gpu.py: _bn_block"""
    bn = np.zeros((8, C), np.float32)
    bn[BN_SCALE] = rng.uniform(0.5, 1.5, C)
    bn[BN_BETA] = rng.normal(0, 0.2, C)
    bn[BN_MEAN] = rng.normal(0, 0.3, C)
    bn[BN_RSTD] = rng.uniform(0.5, 2.0, C)
    bn[BN_GA] = rng.uniform(0.5, 1.5, C)
    bn[BN_GB] = rng.normal(0, 0.2, C)
    bn[BN_GMEAN] = rng.normal(0, 0.05, C)
    return bn


def case_seed(case):
    return int(sum(v * p for v, p in zip(case, (1000003, 10007, 1009, 101, 11, 7, 3))))


def dy32_of(g, y, bn):
    """dy as the device forms it: float32 arithmetic (the device may contract the products into fmas; the scale D covers either)"""
    return (bn[BN_GA] * (g - bn[BN_GMEAN]) + bn[BN_GB] * (y - bn[BN_MEAN])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def make_case(case):
    """The float32 inputs of one case (never written afterwards): a, w, the statistics pivot, g, the conv output y32 the backward kernels
    are GIVEN (the float64 result rounded once), its BatchNorm block bn (DY bound set), the mask operand of the data gradient."""
    B, H, W, Cin, Cout, k, stride = case
    rng = np.random.default_rng(case_seed(case))
    c = types.SimpleNamespace(case=case, B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, stride=stride, pad=k // 2)
    c.Ho, c.Wo = out_hw(H, W, k, stride)
    c.M, c.Min, c.T = B * c.Ho * c.Wo, B * H * W, k * k
    a = np.maximum(rng.normal(0, 1, (B, H, W, Cin)), 0).astype(np.float32)  # a post-ReLU activation
    c.zero_channels = [1, Cin // 2 + 3]
    a[..., c.zero_channels] = 0.0
    if c.Min >= 8:  # a few exactly-zero pixels (the second and the last but one: never the only pixel a strided case reads)
        a.reshape(c.Min, Cin)[[1, c.Min - 2]] = 0.0
    c.a = a
    c.w = (rng.normal(0, 1, (Cout, Cin, k, k)) * np.sqrt(2.0 / (k * k * Cout))).astype(np.float32)
    c.piv = rng.normal(0, 0.5, Cout).astype(np.float32)
    c.a_bound = np.float32(SLACK * float(a.max()))
    c.idx_f = gather_index(B, H, W, c.Ho, c.Wo, k, stride, False)
    c.idx_t = gather_index(B, c.Ho, c.Wo, H, W, k, stride, True)
    c.Wf = np.ascontiguousarray(c.w.reshape(Cout, Cin, c.T).transpose(2, 1, 0).reshape(c.T * Cin, Cout))  # [(t, ci)][co]
    c.Wb = np.ascontiguousarray(c.w.reshape(Cout, Cin, c.T).transpose(2, 0, 1).reshape(c.T * Cout, Cin))  # [(t, co)][ci]
    c.A = im2col(a.reshape(c.Min, Cin), c.idx_f)                                                            # [M][(t, ci)]
    c.y64 = c.A.astype(np.float64) @ c.Wf.astype(np.float64)
    c.y32 = c.y64.astype(np.float32)
    c.g = rng.normal(0, 1, (c.M, Cout)).astype(np.float32)
    c.bn = bn_block(Cout, rng)
    c.dy32 = dy32_of(c.g, c.y32, c.bn)
    c.bn[BN_AUX, AUX_DY_BOUND] = SLACK * float(np.abs(c.dy32).max())
    c.dy_bound = c.bn[BN_AUX, AUX_DY_BOUND]
    c.w_bound = np.float32(np.abs(c.w).max())  # the weights' bound is their measured maximum (ttk_conv_weight_repack)
    c.mask_y = rng.normal(0, 1, (c.Min, Cin)).astype(np.float32)
    c.mbn = bn_block(Cin, rng)
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# reference and yardstick of one product
# ---------------------------------------------------------------------------------------------------------------------------------
def _err_over_s(x, ref, s):
    """|x - ref| / s per element; 0 / 0 = 0, anything else over 0 is infinitely far out"""
    err = np.abs(np.asarray(x, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, err / np.where(s > 0, s, 1.0), np.where(err == 0, 0.0, np.inf))


class Product:
    """out[M,N] = A @ B with its float64 value, scale, range floor and yardstick.  A32 / B32: the float32 operand values the device
    splits; A64: the exact operand (float64 of the inputs); Aabs: |A| or the term bound D."""

    def __init__(self, A32, A64, Aabs, B32, bound_a=None, bound_b=None):
        """bounds None: a plain float32 kernel (the 7x7 stem) - no split, no range floor, the fma chain is the whole yardstick"""
        B64 = B32.astype(np.float64)
        self.A32, self.B32, self.bound_a, self.bound_b = A32, B32, bound_a, bound_b
        self.ref = A64 @ B64
        self.s = Aabs @ np.abs(B64)
        self.chain = chain32(A32, B32)
        self.E_chain_rows = self.E_rows(self.chain)
        self.E_chain = self.Y = float(self.E_chain_rows.max())
        self.floor = np.zeros_like(self.s)
        if bound_a is not None:
            self.floor = floor_abs(A32, bound_a) @ np.abs(B64) + Aabs @ floor_abs(B32, bound_b)
            self.model = split_model(A32, B32, bound_a, bound_b)
            self.E_model_rows = self.E_rows(self.model)
            self.E_model = float(self.E_model_rows.max())
            self.Y = max(self.E_chain, self.E_model)

    def E_rows(self, x):
        return _err_over_s(x, self.ref, self.s).max(1)

    def E(self, x):
        return float(self.E_rows(x).max())

    def allowed(self):
        """per element: the largest |x - f64| the criterion accepts"""
        return (MARGIN * self.Y + U) * self.s + self.floor

    def ratio(self, x, mask=None):
        """(worst (|x - f64| - floor - 2^-24 s) / (s Y) over the elements with s > 0, exact zeros kept where s == 0); mask: elements judged"""
        x = np.asarray(x, np.float64)
        live = self.s > 0 if mask is None else (self.s > 0) & mask
        zeros_ok = bool(np.all(x[(self.s == 0) if mask is None else ((self.s == 0) & mask)] == 0))
        if not live.any():
            return 0.0, zeros_ok
        r = (np.abs(x - self.ref) - self.floor - U * self.s)[live] / (self.s[live] * max(self.Y, 1e-300))
        return (float(r.max()) if np.isfinite(r).all() else float("inf")), zeros_ok

    def rel(self, x):
        """the whole-tensor figure of tests/test_conv_gpu.py"""
        return float(np.linalg.norm(np.asarray(x, np.float64) - self.ref) / max(np.linalg.norm(self.ref), 1e-30))


def dy_terms(c):
    """(dy64, D) of the case: exact dy and the bound of its terms, [M][Cout]"""
    bn, g, y = c.bn.astype(np.float64), c.g.astype(np.float64), c.y32.astype(np.float64)
    dy64 = bn[BN_GA] * (g - bn[BN_GMEAN]) + bn[BN_GB] * (y - bn[BN_MEAN])
    D = np.abs(bn[BN_GA]) * (np.abs(g) + np.abs(bn[BN_GMEAN])) + np.abs(bn[BN_GB]) * (np.abs(y) + np.abs(bn[BN_MEAN]))
    return dy64, D


@functools.lru_cache(maxsize=8)
def forward(case):
    c = make_case(case)
    return Product(c.A, c.A.astype(np.float64), np.abs(c.A).astype(np.float64), c.Wf, c.a_bound, c.w_bound)


@functools.lru_cache(maxsize=8)
def dgrad(case):
    """the raw data gradient [B*H*W][Cin]; .undecided / .open / .share: the mask of the masked form"""
    c = make_case(case)
    dy64, D = dy_terms(c)
    p = Product(im2col(c.dy32, c.idx_t), im2col(dy64, c.idx_t), im2col(D, c.idx_t), c.Wb, c.dy_bound, c.w_bound)
    mb, my = c.mbn.astype(np.float64), c.mask_y.astype(np.float64)
    pre = mb[BN_SCALE] * (my - mb[BN_MEAN]) + mb[BN_BETA]
    p.undecided = np.abs(pre) <= UNDECIDED_REL * (np.abs(mb[BN_SCALE]) * (np.abs(my) + np.abs(mb[BN_MEAN])) + np.abs(mb[BN_BETA]))
    p.open = pre > 0
    p.share = float(p.undecided.mean())
    return p


@functools.lru_cache(maxsize=8)
def wgrad(case):
    """dw as [Cout][(t, ci)]: the order of the contraction (wgrad_from_torch brings torch's [Cout][Cin][k][k] into it)"""
    c = make_case(case)
    dy64, D = dy_terms(c)
    return Product(np.ascontiguousarray(c.dy32.T), np.ascontiguousarray(dy64.T), np.ascontiguousarray(D.T), c.A, c.dy_bound, c.a_bound)


def wgrad_from_torch(c, dw):
    """dw[Cout][Cin][k][k] -> [Cout][(t, ci)]"""
    return np.asarray(dw).reshape(c.Cout, c.Cin, c.T).transpose(0, 2, 1).reshape(c.Cout, c.T * c.Cin)


def masked_ratio(p, out):
    """The masked data gradient `out` against the raw product p: (ratio over the open and undecided-but-nonzero elements, closed elements
    exactly zero and no undecided element anything but 0 or the unmasked value)."""
    out = np.asarray(out, np.float64)
    closed = ~p.open & ~p.undecided
    either_zero = p.undecided & (out == 0)
    judged = ~closed & ~either_zero
    ratio, zeros_ok = p.ratio(out, judged)
    return ratio, zeros_ok and bool(np.all(out[closed] == 0))


def wgrad_slices(M, Cout, ncols):
    """the slice count of launch_conv_wgrad16 (conv_wgrad_plan / wgrad_slices in csrc/pwconv_f16.hip), restated"""
    bn = 192 if Cout <= 64 and ncols % 192 == 0 and ncols % 256 != 0 else 256
    tiles = -(-Cout // (64 if Cout <= 64 else 128)) * -(-ncols // bn)
    slices = max((512 if bn == 192 else 256) // tiles, 1)
    slices = min(slices, -(-M // 128))
    rows = -(-(-(-M // slices)) // 32) * 32
    return -(-M // rows), rows


# ---------------------------------------------------------------------------------------------------------------------------------
# the non-GEMM neighbours whose old tests have a whole-tensor figure only: the 7x7 stem (49-tap contraction) and the 3x3 blur (9 taps)
# ---------------------------------------------------------------------------------------------------------------------------------
def stem_case(B, H, W):
    """inputs as tests/test_resnet_kernels_gpu.py draws them; x[B][H][W] (one channel), w[64][49]"""
    rng = np.random.default_rng(100003 * B + 1009 * H + W)
    c = types.SimpleNamespace(B=B, H=H, W=W)
    c.Ho, c.Wo = out_hw(H, W, 7, 2)
    c.M = B * c.Ho * c.Wo
    c.x = rng.uniform(-0.5, 0.5, (B, H, W)).astype(np.float32)
    c.w = (rng.normal(0, 1, (64, 49)) * 0.2).astype(np.float32)
    c.piv = rng.normal(0, 0.1, 64).astype(np.float32)
    c.X = im2col(c.x.reshape(-1, 1), gather_index(B, H, W, c.Ho, c.Wo, 7, 2, False))  # [M][49]
    c.fwd = Product(c.X, c.X.astype(np.float64), np.abs(c.X).astype(np.float64), np.ascontiguousarray(c.w.T))
    c.y32 = c.fwd.ref.astype(np.float32)
    c.g = rng.normal(0, 1, (c.M, 64)).astype(np.float32)
    c.bn = bn_block(64, rng)
    c.dy32 = dy32_of(c.g, c.y32, c.bn)
    dy64, D = dy_terms(c)
    c.wgrad = Product(np.ascontiguousarray(c.dy32.T), np.ascontiguousarray(dy64.T), np.ascontiguousarray(D.T), c.X)
    return c


BLUR_TAPS = np.outer([0.25, 0.5, 0.25], [0.25, 0.5, 0.25]).reshape(9)  # exact in float32


class BlurProduct:
    """out[row][c] = sum_t BLUR_TAPS[t] * v[idx[row][t]][c] (depthwise): float64 value, scale and the float32 fma chain in tap order.
    v32: the float32 operand, v64 / vabs: its exact value and the bound of its terms (ga + gb is rounded once before the taps)."""

    def __init__(self, v32, v64, vabs, idx):
        C = v32.shape[1]
        g = lambda x: im2col(x, idx).reshape(idx.shape[0], 9, C)
        self.ref = np.einsum("t,rtc->rc", BLUR_TAPS, g(v64))
        self.s = np.einsum("t,rtc->rc", BLUR_TAPS, g(vabs))
        acc, taps = np.zeros((idx.shape[0], C), np.float32), g(v32).astype(np.float64)
        for t in range(9):
            acc = (acc + BLUR_TAPS[t] * taps[:, t]).astype(np.float32)
        self.chain = acc.astype(np.float64)
        self.floor = np.zeros_like(self.s)
        self.E_chain = self.Y = float(_err_over_s(self.chain, self.ref, self.s).max())

    ratio = Product.ratio
