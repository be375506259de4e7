"""Float64 reference, yardstick and cases of the MobileNet pointwise (1x1) GEMMs (csrc/pwconv.hip, pwconv_f16.hip, pwconv_r.hip,
pw_bwd_fused.hip).  Plain numpy on the CPU; tests/test_pw_rows_gpu.py compares the kernels with it through the C ABI, row by row,
tests/test_pw_ref.py pins it on its own without a GPU.  The arithmetic - `Product`, `chain32`, `split_model`, the criterion
    |x - f64| <= (MARGIN * Y + 2^-24) * s + floor,      x == 0 exactly where s == 0
and its derivation - is tests/conv_ref.py's, imported and not restated: a pointwise layer is the k = 1, stride 1 case of that file
(im2col is the identity), with two differences.

1. The forward and weight-gradient operand `a` is FORMED ON LOAD from the depthwise layer's raw output ydw and its BatchNorm block:
       a = max(scale * (ydw - mean) + beta, 0)                                  (float32; the device may contract the products into fmas)
   where conv_ref's `a` is a stored activation.  So `a` is to these products what `dy` is to conv_ref's: A32 is the float32 value numpy
   forms, A64 = max(pre64, 0) the exact value of the float32 inputs, and the scale takes
       P = |scale| (|ydw| + |mean|) + |beta|
   in place of |a| - the device rounds every term of pre, and the cancellation between the terms is not the GEMM's error - wherever the
   pre-activation is open or undecided, and 0 where it is decidedly closed (there a == 0 on any device).  Undecided is conv_ref.dgrad's
   definition, |pre64| <= 2^-20 * P, with one refinement that follows from it: where P == 0 (scale == 0 and beta == 0) every term is zero,
   pre is exactly 0 in any float32 formation and [0 > 0] is closed - decided.
   The weight gradient dy^T @ a has BOTH operands formed on load: `Judged` takes the exact value and the term bound of the B operand too.
2. The data gradient is masked by the layer's own input, [bn_dw(ydw) > 0], the same pre as in 1: conv_ref.masked_ratio judges it
   (decidedly closed elements exactly 0, undecided ones 0 or within the bound, at most UNDECIDED_CAP of a case's elements undecided).

Products:  forward a @ w^T [M][Cout];  dgrad (dy @ w) * mask [M][Cin];  wgrad dy^T @ a [Cout][Cin];  dy = ga (g - gmean) + gb (y - mean)
and its term bound D from conv_ref.dy_terms.

Yardstick by form.  The forms on the fp32 matrix instruction (pw_gemm_k, pw_wgrad_k, pw_bwd_fused_k<32,64>: `is_fp32_form`) are held to
the fma chain alone, without a range floor (Product with bound_a = None); the split forms to max(chain, split model) with the bounds the
kernels are given: SLACK * max|a|, SLACK * max|dy32| and max|w| (the prepare step measures the weights).

Yardstick cost.  For M > 1024 chain32 and split_model run on the first 256 and the last 256 rows only; for the weight gradient on the
full contraction, but for 64 of the Cout output rows.  EVERY row of the kernel's output is still judged against the float64 product
(one matmul).  A maximum over a subset is never larger than the maximum over all rows, so this only tightens the criterion.

Long contractions.  The weight gradient contracts over M, and the fused cases that make a workgroup walk two tiles have M up to 32 801.
One float32 accumulator over that many steps is no yardstick any more: with these inputs (dy and a have non-zero means, so the
accumulator grows linearly) its error grows like sqrt(M) and measures E = 1.0e-6 at M = 32 801 and 1.3e-6 at M = 8 201 - outside the band
(0, 2^-20) that tests/test_pw_ref.py holds every yardstick to, and 4 Y of it would let through what the kernels' own tests at small M
catch.  For M > YARD_KBLOCK = 1024 the yardstick is therefore ALSO evaluated with the contraction cut into blocks of 1024 steps, each
block its own chain / split model, the block results added in float32 in order - the accuracy class of a kernel that gives no
accumulator more than 1024 rows, which every weight-gradient form does at these M (the slice plans above; the fused kernels have at
least 128 walkers) - and Y is the SMALLER of the two figures: never larger than the full chain's, so this, too, only tightens.

Inputs (make_case), seeded by the case: ydw ~ N(0, 1), He-scaled w, g ~ N(0, 1), BatchNorm blocks from conv_ref.bn_block (GMEAN != 0: a row
past M formed as ga * (0 - gmean) instead of 0 shows), a random statistics pivot, y = the float64 forward result rounded once (the backward
kernels are GIVEN it).  Two input channels have scale = 0, beta = 0 (exactly-zero operand columns: their weight-gradient columns must be
exactly 0), one has beta = -50 (closed in every row: its data-gradient column must be exactly 0).

Cases (CASES): (M, Cin, Cout) and the entry points it runs - f forward, d data gradient, n both with wsplit = NULL, w weight gradient,
u fused backward - each with the kernel instantiation it is there for; `expected_path` restates the dispatch of launch_gemm,
f16r_gemm_shape, f16_gemm_shape, r_plan, f16t_wgrad_shape, f16_wgrad_shape, fp32_wgrad_plan and fused_shape and names the kernel a shape
reaches.  M is the smallest at which a form can still go wrong: one below, at, and one past a row tile, the first M with two slices."""
import functools
import types

import numpy as np

from conv_ref import (Product, chain32, split_model, pow2_scale, floor_abs, bn_block, dy32_of, dy_terms, masked_ratio, MARGIN, U, SLACK,
                      UNDECIDED_CAP, UNDECIDED_REL, BN_SCALE, BN_BETA, BN_MEAN, BN_GA, BN_GB, BN_GMEAN, BN_AUX, AUX_ACT_BOUND, AUX_DY_BOUND)

YARD_ROWS = 256        # rows at either end that carry the yardstick when M > 1024
YARD_WGRAD_ROWS = 64   # output rows of the weight gradient that carry it
YARD_KBLOCK = 1024    # longest single-accumulator chain of the weight-gradient yardstick
CUS = 256              # compute units of the MI355X (r_plan's cost model asks the device)


# ---------------------------------------------------------------------------------------------------------------------------------
# the dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def shape_ok(M, Cin, Cout):
    p2 = lambda v: 32 <= v <= 1024 and v & (v - 1) == 0
    return M > 0 and p2(Cin) and p2(Cout)


def f16r_gemm_shape(K, Nout, dgrad):
    if K < 128 or K > 1024 or K % 32 or Nout < 256 or Nout % 256:
        return False
    return not (dgrad and K == 256 and Nout == 256)


def f16_gemm_shape(K, Nout):
    return K >= 64 and K % 32 == 0 and ((Nout >= 256 and Nout % 256 == 0) or Nout == 128)


def r_plan(M, K, Nout, cus=CUS):
    """(rblk, rt, row_blocks) of csrc/pwconv_r.hip: r_plan"""
    ct, steps = Nout // 256, K // 32
    best, best_cost = None, 1e300
    for rblk in (4, 6, 8):
        for r in range(1, 4097):
            rb = cus * r // ct
            if rb < 1:
                continue
            rt = _cdiv(M, rb)
            if rt > 32 * rblk:
                continue
            rt = max(rt, 32)
            row_blocks = _cdiv(M, rt)
            rounds = float(_cdiv(row_blocks * ct, cus))
            step = max(384.0 * rblk, rt * 128.0 / 12.0 + 32768.0 / 35.0)
            cost = rounds * (steps * step + rt * 1024.0 / 10.0 + 3000.0)
            if cost < best_cost:
                best_cost, best = cost, (rblk, rt, row_blocks)
            break
    return best if best is not None else (8, 256, _cdiv(M, 256))


def tile_rows(M, K, Nout, dgrad, cus=CUS):
    """ttk_pwconv_tile_rows"""
    return 32 * r_plan(M, K, Nout, cus)[0] if f16r_gemm_shape(K, Nout, dgrad) else 0


def partial_rows(M, K, Nout, dgrad, cus=CUS):
    """ttk_partial_rows_pwconv"""
    return r_plan(M, K, Nout, cus)[2] if f16r_gemm_shape(K, Nout, dgrad) else _cdiv(M, 128)


def gemm_path(M, K, Nout, dgrad, wsplit=True, cus=CUS):
    mode = "DGRAD" if dgrad else "FWD"
    if wsplit and f16r_gemm_shape(K, Nout, dgrad):
        rblk = r_plan(M, K, Nout, cus)[0]
        return f"pw16m_k<{rblk},DGRAD>" if dgrad and rblk < 8 else f"pw16r_k<{rblk},{mode}>"
    if wsplit and f16_gemm_shape(K, Nout):
        return f"pw16_k<128,256,{mode}>" if Nout % 256 == 0 else f"pw16_k<256,128,{mode}>"
    if Nout >= 128:
        return f"pw_gemm_k<128,2,2,{mode},2>"
    if Nout == 64:
        return f"pw_gemm_k<64,2,2,{mode},{1 if K == 32 else 2}>"
    return f"pw_gemm_k<32,4,1,{mode},2>"


def f16t_wgrad_shape(Cin, Cout):
    return Cin >= 256 and Cin % 256 == 0 and Cout >= 128 and Cout % 128 == 0 and not (Cin == 256 and Cout == 256)


def f16_wgrad_shape(Cin, Cout):
    if Cin < 128 or Cout < 128 or Cin % 128 or Cout % 128:
        return False
    return Cin % 256 == 0 or Cout % 256 == 0 or (Cin == 128 and Cout == 128)


def _slices(M, slices, min_rows):
    slices = max(min(slices, _cdiv(M, min_rows)), 1)
    rows = _cdiv(_cdiv(M, slices), 32) * 32
    return _cdiv(M, rows), rows


def wgrad_plan(M, Cin, Cout, scratch):
    """(kernel, slices, rows per slice, scratch form is reproducible) of ttk_pwconv1x1_bwd_weight: t_wgrad_plan (csrc/pwconv_r.hip),
    wgrad_slices (pwconv_f16.hip) and fp32_wgrad_plan (pwconv.hip)"""
    if scratch and f16t_wgrad_shape(Cin, Cout):
        return ("pw16u_wgrad_k",) + _slices(M, max(256 // ((Cout // 128) * (Cin // 256)), 1), 64) + (True,)
    if f16_wgrad_shape(Cin, Cout):
        if Cin % 256 == 0:
            name, tiles = "pw16_wgrad_k<128,256>", (Cout // 128) * (Cin // 256)
        elif Cout % 256 == 0:
            name, tiles = "pw16_wgrad_k<256,128>", (Cout // 256) * (Cin // 128)
        else:
            name, tiles = "pw16_wgrad_k<128,128>", 1
        return (name,) + _slices(M, max(256 // tiles, 1), 128) + (True,)
    bn, bk = min(Cout, 128), min(Cin, 128)
    assert bn < 128 or bk < 128  # powers of two: Cin, Cout >= 128 is an f16_wgrad_shape
    return (f"pw_wgrad_k<{bn},{bk}>",) + _slices(M, 1024 // ((Cout // bn) * (Cin // bk)), 256) + (not (bn == 32 and bk == 32),)


def wgrad_partial_bytes(M, Cin, Cout):
    """ttk_pwconv_wgrad_partial_bytes: 0 = no reproducible form (32 -> 32: four waves share the one tile through atomics)"""
    if not shape_ok(M, Cin, Cout):
        return 0
    _, slices, _, reproducible = wgrad_plan(M, Cin, Cout, True)
    return 4 * Cin * Cout * slices if reproducible else 0


FUSED = {(32, 64): ("pw_bwd_fused_k<32,64>", 64, 512), (64, 128): ("pw_bwd_fused16_k<64,128>", 32, 256),
         (128, 128): ("pw_bwd_fused16_k<128,128>", 32, 256), (128, 256): ("pw_bwd_fused16w_k<128>", 32, 256),
         (256, 256): ("pw_bwd_fused16w_k<256>", 32, 128)}  # (Cin, Cout): kernel, rows of a tile, walkers of the persistent grid


def fused_rows(M, Cin, Cout):
    """ttk_pwconv1x1_bwd_fused_rows: walkers = rows of `part` = slices of the scratch form"""
    if (Cin, Cout) not in FUSED or M <= 0:
        return 0
    _, tile, cap = FUSED[(Cin, Cout)]
    return min(_cdiv(M, tile), cap)


def expected_path(M, Cin, Cout, cus=CUS):
    """kernel instantiation per entry point and form for one shape"""
    return {"fwd": gemm_path(M, Cin, Cout, False, True, cus), "fwd_nosplit": gemm_path(M, Cin, Cout, False, False, cus),
            "dgrad": gemm_path(M, Cout, Cin, True, True, cus), "dgrad_nosplit": gemm_path(M, Cout, Cin, True, False, cus),
            "wgrad": wgrad_plan(M, Cin, Cout, False)[0], "wgrad_scratch": wgrad_plan(M, Cin, Cout, True)[0] if wgrad_partial_bytes(M, Cin, Cout) else None,
            "fused": FUSED[(Cin, Cout)][0] if (Cin, Cout) in FUSED else None}


def is_fp32_form(name):
    return name.startswith(("pw_gemm_k", "pw_wgrad_k", "pw_bwd_fused_k"))


NAMES = ([f"pw_gemm_k<{t},{m},{s}>" for t, s in (("32,4,1", 2), ("64,2,2", 1), ("64,2,2", 2), ("128,2,2", 2)) for m in ("FWD", "DGRAD")]
         + [f"pw16_k<{t},{m}>" for t in ("256,128", "128,256") for m in ("FWD", "DGRAD")]
         + ["pw16r_k<4,FWD>", "pw16r_k<6,FWD>", "pw16r_k<8,FWD>", "pw16m_k<4,DGRAD>", "pw16m_k<6,DGRAD>", "pw16r_k<8,DGRAD>"]
         + ["pw16u_wgrad_k", "pw16_wgrad_k<128,128>", "pw16_wgrad_k<128,256>", "pw16_wgrad_k<256,128>"]
         + [f"pw_wgrad_k<{bn},{bk}>" for bn in (32, 64, 128) for bk in (32, 64, 128) if bn < 128 or bk < 128]
         + [v[0] for v in FUSED.values()])

# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
_TABLE = []


def _rows(ms, cin, cout, what):
    _TABLE.extend(((m, cin, cout), what) for m in ms)


_T = (127, 128, 129)  # around the 128-row tile of pw_gemm_k and of pw16_k<128,256>
# ---- forward / data gradient on fp32 MFMA (forward: K = Cin, Nout = Cout; data gradient: K = Cout, Nout = Cin)
_rows(_T, 32, 32, "fd")       # pw_gemm_k<32,4,1,FWD,2> and <32,4,1,DGRAD,2>, K = 32: one LDS stage
_rows(_T, 64, 32, "fd")       # pw_gemm_k<32,4,1,FWD,2> at K = 64 (two stages); data gradient K = 32, Nout = 64: pw_gemm_k<64,2,2,DGRAD,1>
_rows(_T, 32, 64, "fd")       # pw_gemm_k<64,2,2,FWD,1>; data gradient K = 64, Nout = 32: pw_gemm_k<32,4,1,DGRAD,2>
_rows(_T, 64, 64, "fd")       # pw_gemm_k<64,2,2,FWD,2> and <64,2,2,DGRAD,2>
_rows(_T, 32, 128, "fd")      # pw_gemm_k<128,2,2,FWD,2> at K = 32 (f16_gemm_shape needs K >= 64); data gradient K = 128: <32,4,1,DGRAD,2>, four stages
_rows(_T, 32, 256, "f")       # pw_gemm_k<128,2,2,FWD,2>, two column tiles
_rows(_T, 128, 32, "d")       # pw_gemm_k<128,2,2,DGRAD,2> at K = 32
_rows((129,), 256, 32, "d")   # ... two column tiles
_rows((129,), 128, 256, "n")  # wsplit = NULL: pw_gemm_k<128,2,2,FWD,2> at K = 128, <128,2,2,DGRAD,2> at K = 256
_rows((129,), 256, 128, "n")  # wsplit = NULL: pw_gemm_k<128,2,2,FWD,2> at K = 256, <128,2,2,DGRAD,2> at K = 128 (two column tiles)
# ---- pw16_k<256,128> (Nout = 128): 256-row tiles
_R = (255, 256, 257)
_rows(_R, 64, 128, "fd")      # pw16_k<256,128,FWD> at K = 64; data gradient K = 128, Nout = 64: pw_gemm_k<64,2,2,DGRAD,2>
_rows(_R, 128, 64, "fd")      # pw16_k<256,128,DGRAD> at K = 64; forward K = 128, Nout = 64: pw_gemm_k<64,2,2,FWD,2>
_rows(_R, 128, 128, "fd")     # pw16_k<256,128,FWD> and <256,128,DGRAD> at K = 128
_rows(_R, 512, 128, "f")      # pw16_k<256,128,FWD> at K = 512
_rows(_R, 128, 512, "d")      # pw16_k<256,128,DGRAD> at K = 512
# ---- pw16_k<128,256>: K = 64 (below f16r_gemm_shape), and the data gradient of 256 -> 256
_rows(_T, 64, 256, "f")       # pw16_k<128,256,FWD> at K = 64
_rows(_T, 256, 64, "d")       # pw16_k<128,256,DGRAD> at K = 64
_rows(_T, 256, 256, "d")      # pw16_k<128,256,DGRAD> at K = 256 (the shape f16r_gemm_shape leaves out)
# ---- row-block kernels at 128-row tiles (rblk 4; the smallest row block is 32 rows), K = 128: four k32 steps
_rows((31, 32, 33, 130), 128, 256, "f")  # pw16r_k<4,FWD>
_rows((31, 32, 33, 130), 256, 128, "d")  # pw16m_k<4,DGRAD>
_rows((33,), 1024, 256, "f")  # pw16r_k<4,FWD> at K = 1024
_rows((33,), 256, 1024, "d")  # pw16m_k<4,DGRAD> at K = 1024
# (heights 6 and 8 - pw16r_k<6|8,FWD>, pw16m_k<6,DGRAD>, pw16r_k<8,DGRAD> - at the smallest M the cost model gives them: tall_cases)
# ---- weight gradient
for _ci, _co in ((256, 128), (512, 128), (256, 512), (512, 512)):
    _rows((64, 65, 97), _ci, _co, "w")   # scratch: pw16u_wgrad_k, second slice from M = 65 (t_wgrad_plan); atomic: pw16_wgrad_k<128,256>
_W = (128, 129, 161)                      # wgrad_slices: second slice from M = 129, ragged at 161
_rows(_W, 128, 128, "w")      # pw16_wgrad_k<128,128>
_rows(_W, 256, 256, "w")      # pw16_wgrad_k<128,256> in both forms (f16t_wgrad_shape leaves 256 x 256 out)
_rows(_W, 256, 128, "w")      # pw16_wgrad_k<128,256> without scratch (with: pw16u_wgrad_k)
_rows(_W, 128, 256, "w")      # pw16_wgrad_k<256,128>
for _co in (32, 64, 128):
    for _ci in (32, 64, 128):
        if _co < 128 or _ci < 128:
            _rows((256, 257, 300), _ci, _co, "w")  # pw_wgrad_k<Cout,Cin>: second slice from M = 257 (fp32_wgrad_plan), ragged at 300
# ---- fused backward: around one row tile, and one ragged stage past the persistent grid (a workgroup walks two tiles)
for (_ci, _co), (_name, _tile, _cap) in FUSED.items():
    _rows((_tile - 1, _tile, _tile + 1, _cap * _tile + (33 if _tile == 64 else 9)), _ci, _co, "u")  # the kernel FUSED names

ENTRIES = {}
for _case, _what in _TABLE:
    ENTRIES[_case] = "".join(sorted(set(ENTRIES.get(_case, "") + _what)))
CASES = list(ENTRIES)
TALL = [(128, 1024, False, 192), (128, 1024, False, 256), (1024, 128, True, 192), (1024, 128, True, 256)]  # (Cin, Cout, dgrad, tile rows)
TALL_LIMIT = 20000


def find_tall_M(tile_rows_fn, Cin, Cout, dgrad, want):
    """smallest M below TALL_LIMIT at which tile_rows_fn(M, K, Nout, dgrad) == want (four column tiles: the row count is lowest)"""
    K, Nout = (Cout, Cin) if dgrad else (Cin, Cout)
    return next((M for M in range(1, TALL_LIMIT) if tile_rows_fn(M, K, Nout, int(dgrad)) == want), None)


def cases_of(letter):
    return [c for c in CASES if letter in ENTRIES[c]]


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def make_case(case, zero_channels=None, closed_channel=None):
    """The float32 inputs of one case (never written afterwards) and the exact operand `a` with its term bound.  zero_channels (a tuple),
    closed_channel: where the planted channels go (tests/anyc_ref.py puts one into the narrow last channel block); None: the tuned
    family's places."""
    M, Cin, Cout = case
    rng = np.random.default_rng(1000003 * M + 1009 * Cin + Cout)
    c = types.SimpleNamespace(case=case, M=M, Cin=Cin, Cout=Cout)
    c.ydw = rng.normal(0, 1, (M, Cin)).astype(np.float32)
    c.w = (rng.normal(0, 1, (Cout, Cin)) * np.sqrt(2.0 / Cout)).astype(np.float32)
    c.piv = rng.normal(0, 0.5, Cout).astype(np.float32)
    c.bn_dw, c.bn = bn_block(Cin, rng), bn_block(Cout, rng)  # c.bn: the pointwise layer's own block (conv_ref.dy_terms reads it)
    c.zero_channels = [1, Cin // 2 + 3] if zero_channels is None else list(zero_channels)
    c.closed_channel = Cin // 4 + 2 if closed_channel is None else closed_channel
    c.bn_dw[BN_SCALE, c.zero_channels] = 0.0
    c.bn_dw[BN_BETA, c.zero_channels] = 0.0
    c.bn_dw[BN_BETA, c.closed_channel] = -50.0
    b = c.bn_dw
    c.a32 = np.maximum(b[BN_SCALE] * (c.ydw - b[BN_MEAN]) + b[BN_BETA], 0).astype(np.float32)
    b64, y64 = b.astype(np.float64), c.ydw.astype(np.float64)
    c.pre64 = b64[BN_SCALE] * (y64 - b64[BN_MEAN]) + b64[BN_BETA]
    c.a64 = np.maximum(c.pre64, 0)
    c.P = np.abs(b64[BN_SCALE]) * (np.abs(y64) + np.abs(b64[BN_MEAN])) + np.abs(b64[BN_BETA])
    c.undecided = (np.abs(c.pre64) <= UNDECIDED_REL * c.P) & (c.P > 0)
    c.open = c.pre64 > 0
    c.share = float(c.undecided.mean())
    c.aabs = np.where(~c.open & ~c.undecided, 0.0, c.P)
    c.a_bound = np.float32(SLACK * float(c.a32.max()))
    c.bn_dw[BN_AUX, AUX_ACT_BOUND] = c.a_bound
    c.w_bound = np.float32(np.abs(c.w).max())
    c.y64 = c.a64 @ c.w.astype(np.float64).T
    c.y32 = c.y64.astype(np.float32)
    c.g = rng.normal(0, 1, (M, Cout)).astype(np.float32)
    c.dy32 = dy32_of(c.g, c.y32, c.bn)
    c.dy_bound = np.float32(SLACK * float(np.abs(c.dy32).max()))
    c.bn[BN_AUX, AUX_DY_BOUND] = c.dy_bound
    c.bn_pw = c.bn
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# reference and yardstick of one product
# ---------------------------------------------------------------------------------------------------------------------------------
class Judged:
    """out = A @ B: float64 value, scale and range floor of EVERY row, the yardstick Y of conv_ref.Product on `rows` of A (None: all).
    B64 / Babs: exact value and term bound of a B operand that is formed on load too (None: B32 is given, as conv_ref's is)."""
    allowed, ratio, rel, E_rows, E = Product.allowed, Product.ratio, Product.rel, Product.E_rows, Product.E

    def __init__(self, A32, A64, Aabs, B32, B64=None, Babs=None, bounds=None, rows=None, kblock=None):
        ba, bb = bounds if bounds is not None else (None, None)
        sub = slice(None) if rows is None else rows
        y = Product(A32[sub], A64[sub], Aabs[sub], B32, ba, bb)
        if B64 is not None:
            y.ref, y.s = A64[sub] @ B64, Aabs[sub] @ Babs
            y.E_chain = y.Y = y.E(y.chain)
            if ba is not None:
                y.E_model = y.E(y.model)
                y.Y = max(y.E_chain, y.E_model)
        self.Y_full = y.Y
        if kblock is not None and A32.shape[1] > kblock:  # a long contraction: see "Long contractions" in the module docstring
            def blocked(f):
                acc = np.zeros(y.ref.shape, np.float32)
                for k0 in range(0, A32.shape[1], kblock):
                    acc = (acc.astype(np.float64) + f(np.ascontiguousarray(y.A32[:, k0:k0 + kblock]), B32[k0:k0 + kblock])).astype(np.float32)
                return acc.astype(np.float64)
            y.chain_blocked = blocked(chain32)
            Yb = y.E(y.chain_blocked)
            if ba is not None:
                y.model_blocked = blocked(lambda a, b: split_model(a, b, ba, bb))
                Yb = max(Yb, y.E(y.model_blocked))
            y.Y = min(y.Y, Yb)
        self.yard, self.Y, self.E_chain, self.E_model = y, y.Y, y.E_chain, getattr(y, "E_model", None)
        self.A32, self.B32, self.bound_a, self.bound_b = A32, B32, ba, bb
        if rows is None:
            self.ref, self.s, self.floor = y.ref, y.s, y.floor
            return
        B64 = B32.astype(np.float64) if B64 is None else B64
        self.ref, self.s = A64 @ B64, Aabs @ (np.abs(B64) if Babs is None else Babs)
        self.floor = np.zeros_like(self.s)
        if ba is not None:
            self.floor = floor_abs(A32, ba) @ np.abs(B32.astype(np.float64)) + Aabs @ floor_abs(B32, bb)


def _end_rows(M):
    return None if M <= 1024 else np.r_[0:YARD_ROWS, M - YARD_ROWS:M]


@functools.lru_cache(maxsize=6)
def forward(case, split):
    c = make_case(case)
    return Judged(c.a32, c.a64, c.aabs, np.ascontiguousarray(c.w.T), bounds=(c.a_bound, c.w_bound) if split else None, rows=_end_rows(c.M))


@functools.lru_cache(maxsize=6)
def dgrad(case, split):
    """the raw data gradient [M][Cin]; .open / .undecided / .share: the mask of conv_ref.masked_ratio"""
    c = make_case(case)
    dy64, D = dy_terms(c)
    p = Judged(c.dy32, dy64, D, c.w, bounds=(c.dy_bound, c.w_bound) if split else None, rows=_end_rows(c.M))
    p.open, p.undecided, p.share = c.open, c.undecided, c.share
    return p


@functools.lru_cache(maxsize=6)
def wgrad(case, split):
    c = make_case(case)
    dy64, D = dy_terms(c)
    rows = None if c.Cout <= YARD_WGRAD_ROWS else np.arange(YARD_WGRAD_ROWS) * (c.Cout // YARD_WGRAD_ROWS)
    T = np.ascontiguousarray
    return Judged(T(c.dy32.T), T(dy64.T), T(D.T), c.a32, c.a64, c.aabs, bounds=(c.dy_bound, c.a_bound) if split else None, rows=rows,
                  kblock=YARD_KBLOCK)
