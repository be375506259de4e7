"""Float64 reference, yardstick, restated host logic and cases of the any-channel-count kernel family (ttk_anyc_*: csrc/anyc_pw.hip,
csrc/anyc_pix.hip, csrc/anyc_common.h).  Plain numpy on the CPU; tests/test_anyc_rows_gpu.py compares the kernels with it through the C
ABI, element by element, tests/test_anyc_ref.py pins it on its own without a GPU.  The arithmetic is the sibling files', imported and not
restated: U, MARGIN, UNDECIDED_CAP, bn_block, dy32_of, dy_terms, chain32 and the im2col of tests/conv_ref.py; Judged (conv_ref.Product with
the operand formed on load), the blocked chain and the inputs of tests/pw_ref.py (make_case; its SLACK bounds and UNDECIDED_REL band come
with it); Quantity, conv_fwd / conv_bwd (through forward / dgrad), wgrad_terms, serial_sum, stat_ratios, masked_outside and the inputs of
tests/dw_ref.py (make_case).

Criterion, for every element of every output:
    |x - f64| <= (MARGIN * Y + 2^-24) * s,      x == 0 exactly where s == 0
s: the same contraction over absolute values with the term bounds P (an activation formed on load: |scale| (|y| + |mean|) + |beta| + |skip|)
and D (dy formed on load) of pw_ref / dw_ref.  Masked elements follow conv_ref's UNDECIDED rule (decidedly closed: exactly 0; undecided: 0
or within the bound; at most UNDECIDED_CAP of a case's elements undecided).  Y is measured on the case's own data, never on the kernel's
output:
    pointwise      all three GEMMs run on the exact-fp32 matrix instruction: the float32 fma chain alone, no range floor (the yardstick of
                   pw_ref.is_fp32_form); the weight gradient with M > YARD_KBLOCK the smaller of the full and the blocked chain of pw_ref.
    depthwise      y, G: the 9-step chain in the kernel's tap order (dw_ref); a_out: the float32 formation against P; dW: the LARGER of the
                   serial per-tap chain over all input pixels and `blocked_sum`, this family's order: thread pl of workgroup row r chains
                   the pixels m = r * 32 + pl, + rows * 32, ...; the 32 lanes add in lane order; the workgroup rows add as
                   launch_fold_partials chooses (`fold_form`, `fold`).  Past YARD_KBLOCK pixels the serial chain is cut every YARD_KBLOCK
                   pixels like pw_ref's, and the smaller of the full and the cut chain takes its place (pw_ref, "Long contractions").
    stem           the same with 25 taps (the forward: conv_ref.chain32 over the im2col in tap order).
    avgpool_fwd    the serial float32 chain over HW, then one multiplication by the float32 1 / HW.
    avgpool_bwd    the float32 formation gfeat * (1 / HW) itself, against |gfeat| / HW; bn_act: the formation against P.  Where the
                   formation is exact (HW = 1: 1 / HW = 1) Y is 0 and the criterion is the final rounding alone.

Statistics, held to the tensor AS STORED.  The family sums in float32: a thread over its pixels, then the 32 pixel lanes in lane order; the
rows meet on the host in float64.  A sum of n float32 terms in which no term passes through more than L rounded additions has
|fl(sum) - sum| <= ((1 + U)^L - 1) sum |term| (Higham, Accuracy and Stability, 4.2).
  * Pixel kernels: a thread adds at most ceil(M / (32 rows)) terms (the first onto an exact zero), the lane fold adds 32 (the first onto
    an exact zero): at most ceil(M / (32 rows)) + 30 rounded additions.  L = ceil(M / (32 rows)) + 32 leaves two in hand, which covers the
    second-order part of (1 + U)^L - 1 for every L < 2^23 (L^2 U^2 / 2 < 2 U).
  * GEMM epilogue (gemm_partials): 16 rows per lane, one shuffle between the half waves, 4 waves in order: at most 19 rounded additions;
    L = 16 + 1 + 4 = 21.
      first moment    |sum_rows part[0] - sum64 d|   <= L U sum |d|
      second moment   |sum_rows part[1] - sum64 d^2| <= (L + 2) U sum d^2
d = the stored float32 output minus the pivot, rounded once (the kernel's own float32 subtraction, which numpy repeats bit for bit); its
square enters the accumulator through an fma, unrounded - the 2 U are kept for a device that rounds the product.  The backward pair
sum g, sum g (y - mean) has the same form (g enters exactly, y - mean is rounded once, the product through an fma).  TTK_AUX_GMAX is a
maximum: exact.

Inputs.  Pointwise: pw_ref.make_case with one zero-operand channel moved into the narrow last channel block (`pw_planted`); depthwise,
pooling, bn_act: dw_ref.make_case (pooling as an HW x 1 image; two whole zero weight channels, two pixels with a_in exactly zero); stem:
`stem_case`, after conv_ref.stem_case.

The host logic the kernels' launchers apply is restated as pure functions (c_ok, blk_w, n_blk, off, pix_rows, grid_1d, wgrad_slices,
rows_per, fold_form) and compared with the C ABI in the GPU file.  The case tables name the feature each line is there for."""
import functools
import types

import numpy as np

import conv_ref
import dw_ref
import pw_ref
from conv_ref import (U, MARGIN, UNDECIDED_CAP, bn_block, dy32_of, dy_terms, chain32, _err_over_s, BN_SCALE, BN_BETA, BN_MEAN, BN_GA, BN_GMEAN,
                      BN_AUX, AUX_GMAX)
from dw_ref import Quantity, conv_bwd, wgrad_terms, serial_sum, stat_ratios, masked_outside
from pw_ref import Judged, YARD_KBLOCK, YARD_WGRAD_ROWS

YARD_CHANNELS = dw_ref.YARD_CHANNELS
GEMM_STAT_LENGTH = 16 + 1 + 4


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------------
# host logic, restated (csrc/anyc_common.h, the launchers of csrc/anyc_pw.hip and csrc/anyc_pix.hip, launch_fold_partials)
# ---------------------------------------------------------------------------------------------------------------------------------
MAX_C, PIX_LANES, MAX_ROWS, BLOCK, MAX_GRID_1D = 2048, 32, 1024, 256, 4096


def c_ok(C):
    return 8 <= C <= MAX_C and C % 8 == 0


def blk_w(C, cb):
    return min(C - 32 * cb, 32)


def n_blk(C):
    return (C + 31) >> 5


def off(m, c, M, C, narrow_stride=None):
    """element (m, c) of an [M][C] activation in the family's layout; narrow_stride: the row stride taken for the narrow last block
    (a mutation; None: blk_w).  m, c: integers or arrays."""
    cb = np.asarray(c) >> 5
    w = np.minimum(C - 32 * cb, 32)
    if narrow_stride is not None:
        w = np.where(w < 32, narrow_stride, w)
    return cb * M * 32 + np.asarray(m) * w + (np.asarray(c) & 31)


def to_blocks(x):
    """x[..., C] channels-last -> the flat storage order"""
    C = x.shape[-1]
    rows = x.reshape(-1, C)
    M = rows.shape[0]
    out = np.empty(M * C, x.dtype)
    m, c = np.meshgrid(np.arange(M), np.arange(C), indexing="ij")
    out[off(m, c, M, C)] = rows
    return out


def from_blocks(flat, M, C, narrow_stride=None):
    """the [M][C] values a kernel reads from `flat`; with the mutated stride the reads past the end take the last element"""
    m, c = np.meshgrid(np.arange(M), np.arange(C), indexing="ij")
    return flat[np.minimum(off(m, c, M, C, narrow_stride), flat.size - 1)]


def pix_rows(M):
    """ttk_anyc_partial_rows: workgroup rows (grid.x) of a pixel-wise kernel over M pixels, 4 pixels per lane, at most 1024"""
    return min(max(_cdiv(M, 4 * PIX_LANES), 1), MAX_ROWS)


def grid_1d(items):
    return min(max(_cdiv(items, BLOCK), 1), MAX_GRID_1D)


def gemm_rows(M):
    return _cdiv(M, 128)


def pix_stat_length(M):
    return _cdiv(M, PIX_LANES * pix_rows(M)) + 32


def wgrad_slices(M, Cin, Cout):
    tiles = n_blk(Cin) * n_blk(Cout)
    return max(min(4096 // tiles, _cdiv(M, 64)), 1)


def rows_per(M, Cin, Cout):
    return _cdiv(_cdiv(M, wgrad_slices(M, Cin, Cout)), 8) * 8


def slice_plan(M, Cin, Cout):
    """[(first row, end row)] of every slice the weight-gradient kernel is launched with; end <= first: an empty slice (a zero tile)"""
    r = rows_per(M, Cin, Cout)
    return [(s * r, min(s * r + r, M)) for s in range(wgrad_slices(M, Cin, Cout))]


def fold_form(rows, n):
    """the kernel launch_fold_partials takes for `rows` rows of n outputs"""
    return "wide" if rows >= 64 and n <= 65536 else "plain"


def fold(partial, base=None, form=None):
    """partial[rows][n] float32 folded as launch_fold_partials does, bit for bit: plain - serial in row order, from `base` (accumulate) or 0;
    wide - 8 row groups (r = q, q + 8, ...) each serial from 0, then base + the groups in order"""
    partial = np.asarray(partial, np.float32)
    rows, n = partial.shape
    form = form or fold_form(rows, n)
    start = np.zeros(n, np.float32) if base is None else np.asarray(base, np.float32).reshape(n).copy()
    if form == "plain":
        a = start
        for r in range(rows):
            a = a + partial[r]
        return a
    groups = np.zeros((8, n), np.float32)
    for r in range(rows):
        groups[r % 8] = groups[r % 8] + partial[r]
    t = start
    for q in range(8):
        t = t + groups[q]
    return t


def blocked_sum(T, rows=None):
    """T[taps][pixels][ch] (float64 products) summed in this family's order, float32 throughout: -> [taps][ch]"""
    K, M, ch = T.shape
    rows = rows or pix_rows(M)
    steps = _cdiv(M, PIX_LANES * rows)
    Tp = np.zeros((K, steps * rows * PIX_LANES, ch))
    Tp[:, :M] = T
    Tp = Tp.reshape(K, steps, rows, PIX_LANES, ch)
    acc = np.zeros((K, rows, PIX_LANES, ch), np.float32)
    for l in range(steps):
        acc = (acc + Tp[:, l]).astype(np.float32)
    s = np.zeros((K, rows, ch), np.float32)
    for i in range(PIX_LANES):
        s = s + acc[:, :, i]
    return fold(s.transpose(1, 0, 2).reshape(rows, K * ch)).reshape(K, ch)


def stat_rows_model(v, d, rows=None, drop=None):
    """part[rows][2][C] as a pixel kernel of the family sums it, float32 throughout: v[M][C] (float32: y - pivot | g) and v * d through an fma;
    thread pl of row r takes the pixels r * 32 + pl, + rows * 32, ..., then the 32 lanes add in lane order.  drop: a pixel left out."""
    M, C = v.shape
    rows = rows or pix_rows(M)
    steps = _cdiv(M, PIX_LANES * rows)
    T = np.zeros((2, steps * rows * PIX_LANES, C))
    T[0, :M], T[1, :M] = v, v.astype(np.float64) * d
    if drop is not None:
        T[:, drop] = 0.0
    T = T.reshape(2, steps, rows, PIX_LANES, C)
    acc = np.zeros((2, rows, PIX_LANES, C), np.float32)
    for l in range(steps):
        acc = (acc + T[:, l]).astype(np.float32)
    s = np.zeros((2, rows, C), np.float32)
    for i in range(PIX_LANES):
        s = s + acc[:, :, i]
    return s.transpose(1, 0, 2)


def cut_serial_sum(T, block=YARD_KBLOCK):
    """serial_sum with the chain cut every `block` pixels, the block results added in float32 in order (pw_ref, "Long contractions")"""
    acc = np.zeros((T.shape[0], T.shape[2]), np.float32)
    for p0 in range(0, T.shape[1], block):
        acc = acc + serial_sum(T[:, p0:p0 + block])
    return acc


def _wgrad_yard(ref, s, T):
    """Quantity of a [ch][taps] weight gradient whose first T.shape[2] channels carry the yardstick: max(serial, blocked)"""
    nch = T.shape[2]
    q = Quantity(ref, s, serial_sum(T).T, np.s_[:nch])
    q.E_serial = q.Y
    if T.shape[1] > YARD_KBLOCK:
        q.E_serial = min(q.E_serial, float(_err_over_s(cut_serial_sum(T).T, ref[:nch], s[:nch]).max()))
    q.E_blocked = float(_err_over_s(blocked_sum(T).T, ref[:nch], s[:nch]).max())
    q.Y = max(q.E_serial, q.E_blocked)
    return q


def outside(q, x, masked=False):
    """worst |x - f64| / allowed of either kind of reference (Judged | Quantity); inf where an exact zero is not kept"""
    if masked:
        return masked_outside(q, x)
    return float(_err_over_s(np.asarray(x, np.float64), q.ref, q.allowed()).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# pointwise
# ---------------------------------------------------------------------------------------------------------------------------------
# (M, Cin, Cout): entries - f forward, d data gradient, w weight gradient
PW_TABLE = [
    ((1, 8, 8), "fdw"),           # one row, one 8-group, one quad of columns
    ((31, 8, 2048), "fdw"),       # one below a wave tile, shortest K, widest N (32 column tiles)
    ((32, 16, 24), "fdw"),        # at the wave tile
    ((33, 24, 40), "fdw"),        # one past the wave tile; K one narrow block of 24; N = 32 + 8 (second half-tile 8 wide)
    ((127, 72, 24), "fdw"),       # one below the workgroup tile; K = 32 + 32 + 8
    ((128, 48, 96), "fdw"),       # at the workgroup tile; a 0.75-width layer
    ((129, 40, 72), "fdw"),       # one past; N = a second column tile of 8; three weight-gradient slices, the last ragged
    ((161, 104, 136), "fdw"),     # 3 and 4 full blocks plus 8
    ((200, 2048, 8), "fdw"),      # longest K, narrowest N
    ((100, 2048, 2048), "fdw"),   # 4096 weight-gradient tiles, so one slice over all of M
    ((30, 72, 16), "fdw"),        # N = 16 forward (the table's other 16-wide blocks are on the K side), K = 16 in the data gradient
    ((7, 8, 16), "w"),            # below one 8-row step; the 4-row halves
    ((9, 24, 40), "w"),           # past one 8-row step
    ((63, 40, 72), "w"),          # below the one-slice seam
    ((64, 72, 24), "w"),          # at the one-slice seam
    ((65, 24, 48), "w"),          # first M with two slices (40 + 25)
    ((4032, 8, 8), "w"),          # 63 slices: plain fold
    ((4033, 8, 8), "w"),          # 64 slices, the last of one row: wide fold
    ((641, 520, 680), "w"),       # the tenth slice starts past M: a zero tile
]
PW_ENTRIES = dict(PW_TABLE)
PW_CASES = list(PW_ENTRIES)
EMPTY_SLICE_CASE = (641, 520, 680)
# the slice plans the table is there for: (slices, rows per slice)
PW_SLICE_PLANS = {(129, 40, 72): (3, 48), (100, 2048, 2048): (1, 104), (63, 40, 72): (1, 64), (64, 72, 24): (1, 64), (65, 24, 48): (2, 40),
                  (4032, 8, 8): (63, 64), (4033, 8, 8): (64, 64), (641, 520, 680): (10, 72)}
SIDE_PW, SIDE_DW, SIDE_POOL = (129, 32, 64), (2, 6, 7, 32, 2, "none"), (3, 25, 64, "none")  # accepted by both families


def pw_cases_of(letter):
    return [c for c in PW_CASES if letter in PW_ENTRIES[c]]


def pw_planted(Cin):
    """(zero-operand channels, always-closed channel): the second zero channel inside the narrow last block where there is one"""
    return ((1, Cin - 3) if Cin % 32 else (1, Cin // 2 + 3)), Cin // 4 + 2


def pw_case(case):
    zero, closed = pw_planted(case[1])
    return pw_ref.make_case(tuple(case), zero, closed)


@functools.lru_cache(maxsize=4)
def pw_forward(case):
    c = pw_case(case)
    return Judged(c.a32, c.a64, c.aabs, np.ascontiguousarray(c.w.T), rows=pw_ref._end_rows(c.M))


@functools.lru_cache(maxsize=4)
def pw_dgrad(case):
    """the raw data gradient [M][Cin] with .open / .undecided / .share for the masked judgement"""
    c = pw_case(case)
    dy64, D = dy_terms(c)
    p = Judged(c.dy32, dy64, D, c.w, rows=pw_ref._end_rows(c.M))
    p.open, p.undecided, p.share = c.open, c.undecided, c.share
    return p


@functools.lru_cache(maxsize=4)
def pw_wgrad(case):
    c = pw_case(case)
    dy64, D = dy_terms(c)
    rows = None if c.Cout <= YARD_WGRAD_ROWS else np.arange(YARD_WGRAD_ROWS) * (c.Cout // YARD_WGRAD_ROWS)
    T = np.ascontiguousarray
    return Judged(T(c.dy32.T), T(dy64.T), T(D.T), c.a32, c.a64, c.aabs, rows=rows, kblock=YARD_KBLOCK)


def onto(q, base):
    """a weight gradient accumulated onto `base`: one more term of the contraction"""
    r = types.SimpleNamespace(ref=q.ref + base, s=q.s + np.abs(base), Y=q.Y)
    r.allowed = lambda: (MARGIN * r.Y + U) * r.s
    return r


def _bn_act64(bn, y, x=0.0):
    b = bn.astype(np.float64)
    return np.maximum(b[BN_SCALE] * (y.astype(np.float64) - b[BN_MEAN]) + b[BN_BETA] + x, 0.0)


def pw_forward_model(c, mutate=None):
    """the float64 forward product of case c under a mutation of the kernel:
    "stride32"   the narrow last block of ydw is addressed with row stride 32 instead of blk_w
    "drop8"      the last 8-group of K in the narrow block is dropped
    "acc_row"    the accumulator-to-row map has h and r >> 2 exchanged: rows are stored in the wrong places, some never"""
    ydw = c.ydw
    if mutate == "stride32":
        ydw = from_blocks(to_blocks(c.ydw), c.M, c.Cin, narrow_stride=32)
    a = _bn_act64(c.bn_dw, ydw)
    k_end = c.Cin - 8 if (mutate == "drop8" and c.Cin % 32) else c.Cin
    y = a[:, :k_end] @ c.w.astype(np.float64).T[:k_end]
    if mutate == "acc_row":
        out = np.zeros_like(y)
        for r in range(16):
            for h in range(2):
                good, bad = (r & 3) + 8 * (r >> 2) + 4 * h, (r & 3) + 8 * h + 4 * (r >> 2)
                for m0 in range(0, c.M, 32):
                    if m0 + good < c.M and m0 + bad < c.M:
                        out[m0 + bad] = y[m0 + good]
        y = out
    return y


def pw_wgrad_model(c, mutate=None):
    """the float64 weight gradient of case c summed slice by slice under a mutation of the kernel:
    "pad_rows"   the rows between a slice's end and the next 8-row step enter as dy = ga (0 - gmean), with the a of a load clamped to the
                 slice's last row
    "overlap"    rows_per is not rounded up to 8: the 8-row steps of a slice run into the next slice, those rows count twice"""
    dy64, _ = dy_terms(c)
    a64 = c.a64
    bn = c.bn.astype(np.float64)
    dy_fill = bn[BN_GA] * (0.0 - bn[BN_GMEAN])
    plan = slice_plan(c.M, c.Cin, c.Cout)
    if mutate == "overlap":
        raw = _cdiv(c.M, len(plan))
        plan = [(s * raw, min(s * raw + _cdiv(raw, 8) * 8, c.M)) for s in range(len(plan))]
    dw = np.zeros((c.Cout, c.Cin))
    for mb, me in plan:
        if me <= mb:
            continue
        dw += dy64[mb:me].T @ a64[mb:me]
        if mutate == "pad_rows":
            dw += (-(me - mb) % 8) * np.outer(dy_fill, a64[me - 1])
    return dw


def pad_rows(M, Cin, Cout):
    """rows the 8-row steps of the weight gradient form past the ends of its slices"""
    return sum(-(me - mb) % 8 for mb, me in slice_plan(M, Cin, Cout) if me > mb)


def overlap_rows(M, Cin, Cout):
    """rows counted twice were rows_per not rounded up to 8"""
    n = wgrad_slices(M, Cin, Cout)
    raw = _cdiv(M, n)
    return sum(max(min(s * raw + _cdiv(raw, 8) * 8, M) - (s + 1) * raw, 0) for s in range(n - 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# depthwise
# ---------------------------------------------------------------------------------------------------------------------------------
# (B, H, W, C, stride, skip)
DW_CASES = [
    (2, 5, 9, 8, 1, "skip"),        # non-square, one quad pair
    (3, 9, 5, 24, 2, "none"),       # non-square the other way, odd x odd, narrow block of 24
    (2, 6, 7, 40, 2, "none"),       # even x odd, 32 + 8
    (2, 7, 6, 72, 2, "none"),       # odd x even
    (2, 4, 3, 72, 1, "skip"),       # narrow block with skip
    (2, 2, 2, 16, 2, "none"),       # Ho = Wo = 1
    (1, 1, 1, 8, 1, "skip"),        # single pixel
    (1, 1, 1, 8, 2, "none"),        # single pixel
    (3, 1, 40, 16, 1, "none"),      # H = 1
    (3, 40, 1, 16, 2, "none"),      # W = 1
    (1, 3, 3, 2048, 1, "none"),     # 64 channel blocks
    (5, 5, 5, 768, 1, "skip"),      # 125 pixels in and out: ragged pixel lanes in the one workgroup row
    (1, 3, 43, 768, 1, "skip"),     # 129 pixels: two workgroup rows, the second with one pixel
    (2, 257, 257, 8, 1, "none"),    # 132 098 pixels, past the 1024-row cap of pix_rows
]
DW_POSITION_CASES = [(3, 9, 5, 24, 2, "none"), (2, 6, 7, 40, 2, "none"), (5, 5, 5, 768, 1, "skip")]


def dw_key(case):
    """the case as dw_ref.make_case takes it: a stored residual where this family has a skip"""
    return tuple(case[:5]) + ({"skip": "stored", "none": "none"}[case[5]],)


def dw_case(case):
    return dw_ref.make_case(dw_key(case))


def dw_forward(case):
    """(y, a_out) as dw_ref.Quantity"""
    return dw_ref.forward(dw_key(case))


def dw_dgrad(case):
    return dw_ref.dgrad(dw_key(case))


@functools.lru_cache(maxsize=2)
def dw_wgrad(case):
    """Quantity of dW[C][9]; .E_serial, .E_blocked: the two yardstick figures"""
    c = dw_case(case)
    dy64, D = dw_ref.dy_terms(c)
    dy32 = dy32_of(c.g, c.y32, c.bn_dw)
    ref, s = dw_ref.wgrad_sum(c, dy64, c.a64), dw_ref.wgrad_sum(c, D, c.Aabs)
    return _wgrad_yard(ref, s, wgrad_terms(c, dy32, c.a32.astype(np.float64), min(c.C, YARD_CHANNELS)))


def dw_gather(c, mutate=None):
    """idx[B Ho Wo][9] of the forward taps (conv_ref.gather_index).  Mutations: "swap" - H and W exchanged in the input index;
    "wrapcol" - the column test of the border is missing: the tap left of column 0 reads the previous row's last pixel"""
    if mutate != "wrapcol":
        return conv_ref.gather_index(c.B, c.H, c.W, c.Ho, c.Wo, 3, c.stride, False, mutate)
    n, oh, ow = (v.reshape(-1, 1) for v in np.meshgrid(np.arange(c.B), np.arange(c.Ho), np.arange(c.Wo), indexing="ij"))
    kh, kw = (v[None, :] for v in np.divmod(np.arange(9), 3))
    ih, iw = oh * c.stride - 1 + kh, ow * c.stride - 1 + kw
    flat = np.clip((n * c.H + ih) * c.W + iw, 0, c.B * c.H * c.W - 1)
    return np.where((ih >= 0) & (ih < c.H), flat, -1)


def dw_forward_model(c, mutate=None):
    """the float64 forward output [B][Ho][Wo][C] from the gathered taps"""
    taps = conv_ref.im2col(c.a64.reshape(-1, c.C), dw_gather(c, mutate)).reshape(-1, 9, c.C)
    return np.einsum("mtc,ct->mc", taps, c.w.astype(np.float64)).reshape(c.B, c.Ho, c.Wo, c.C)


# ---------------------------------------------------------------------------------------------------------------------------------
# stem
# ---------------------------------------------------------------------------------------------------------------------------------
# (B, H, W, Cout)
STEM_CASES = [
    (1, 5, 5, 8),      # the smallest admitted image
    (2, 6, 9, 24),     # even x odd, narrow block of 24
    (2, 9, 6, 40),     # odd x even, 32 + 8
    (3, 8, 8, 64),     # even x even, two full blocks
    (1, 33, 17, 16),   # several workgroup rows, non-square
]


@functools.lru_cache(maxsize=None)
def stem_case(case):
    """inputs after conv_ref.stem_case: x[B][H][W] (one channel), w[Cout][25]; .fwd, .wgrad: Quantity of y[M][Cout] and dW[Cout][25]"""
    B, H, W, C = case
    rng = np.random.default_rng(100003 * B + 1009 * H + 101 * W + C)
    c = types.SimpleNamespace(case=case, B=B, H=H, W=W, C=C, Ho=(H + 1) // 2, Wo=(W + 1) // 2)
    c.M = B * c.Ho * c.Wo
    c.x = rng.uniform(-0.5, 0.5, (B, H, W)).astype(np.float32)
    c.w = (rng.normal(0, 1, (C, 25)) * 0.2).astype(np.float32)
    c.piv = rng.normal(0, 0.1, C).astype(np.float32)
    c.X = conv_ref.im2col(c.x.reshape(-1, 1), conv_ref.gather_index(B, H, W, c.Ho, c.Wo, 5, 2, False))  # [M][25], tap = kh 5 + kw
    X64, w64 = c.X.astype(np.float64), c.w.astype(np.float64)
    c.fwd = Quantity(X64 @ w64.T, np.abs(X64) @ np.abs(w64).T, chain32(c.X, np.ascontiguousarray(c.w.T)))
    c.y32 = c.fwd.ref.astype(np.float32)
    c.g = rng.normal(0, 1, (c.M, C)).astype(np.float32)
    c.bn = bn_block(C, rng)
    c.dy32 = dy32_of(c.g, c.y32, c.bn)
    dy64, D = dy_terms(c)
    nch = min(C, YARD_CHANNELS)
    T = c.dy32.astype(np.float64)[None, :, :nch] * X64.T[:, :, None]  # [25][M][ch]
    c.wgrad = _wgrad_yard(dy64.T @ X64, D.T @ np.abs(X64), T)
    return c


def stem_forward_model(c, mutate=None):
    """float64 y[M][Cout]; "taps_swapped": the weight tap is read with kh and kw exchanged"""
    w = c.w.astype(np.float64)
    if mutate == "taps_swapped":
        w = w.reshape(c.C, 5, 5).transpose(0, 2, 1).reshape(c.C, 25)
    return c.X.astype(np.float64) @ w.T


# ---------------------------------------------------------------------------------------------------------------------------------
# global average pool and bn_act
# ---------------------------------------------------------------------------------------------------------------------------------
# (B, HW, C, skip)
POOL_CASES = [
    (1, 1, 8, "none"),         # smallest
    (3, 25, 24, "skip"),       # narrow block with skip
    (5, 7, 40, "none"),        # 32 + 8
    (2, 81, 2048, "skip"),     # widest
    (2100, 1, 2048, "none"),   # 1 075 200 items, past the 4096-workgroup cap: both grid-stride loops take a second step
]
POOL_FWD_ONLY = {(2100, 1, 2048, "none")}  # avgpool_fwd and bn_act only


def pool_key(case):
    B, HW, C, skip = case
    return (B, HW, 1, C, 1, skip)


@functools.lru_cache(maxsize=2)
def pool_case(case):
    """the inputs of dw_ref.make_case on an HW x 1 image (y = its yprev, bn = its bn_prev, skip = its stored residual) and gfeat[B][C];
    .feat, .act, .gin: Quantity of the features, of bn_act's output and of the unmasked pooled gradient (with the mask fields)"""
    B, HW, C, skip = case
    d = dw_case(pool_key(case))
    c = types.SimpleNamespace(case=case, B=B, HW=HW, C=C, M=B * HW, y=d.yprev.reshape(B, HW, C), bn=d.bn_prev,
                              skip=None if d.x is None else d.x.reshape(B, HW, C))
    sh = (B, HW, C)
    c.a64, c.a32, c.Aabs, c.pre64 = d.a64.reshape(sh), d.a32.reshape(sh), d.Aabs.reshape(sh), d.pre64.reshape(sh)
    c.open, c.undecided, c.share = d.open.reshape(sh), d.undecided.reshape(sh), d.share
    inv = np.float32(1.0) / np.float32(HW)
    acc = np.zeros((B, C), np.float32)
    for p in range(HW):
        acc = acc + c.a32[:, p]
    c.feat = Quantity(c.a64.sum(1) / HW, c.Aabs.sum(1) / HW, acc * inv)
    c.act = Quantity(c.a64, c.Aabs, c.a32)
    c.gfeat = np.random.default_rng(dw_ref.case_seed(dw_key(pool_key(case))) + 5).normal(0, 1, (B, C)).astype(np.float32)
    g64 = c.gfeat.astype(np.float64)
    full = lambda v: np.ascontiguousarray(np.broadcast_to(v[:, None, :], sh))
    c.gin = Quantity(full(g64 / HW), full(np.abs(g64) / HW), full(c.gfeat * inv))
    c.gin.open, c.gin.undecided, c.gin.share = c.open, c.undecided, c.share
    return c


def pool_bwd_model(c, mutate=None):
    """float64 g[B][HW][C]; "mask_without_skip": the mask sign is taken from the pre-activation without the residual"""
    pre = c.pre64 - (c.skip.astype(np.float64) if (mutate == "mask_without_skip" and c.skip is not None) else 0.0)
    return c.gin.ref * (pre > 0)
