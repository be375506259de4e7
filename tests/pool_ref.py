"""Float64 reference of the kernels between the backbone and the heads: global average pooling with the last BatchNorm + residual +
ReLU applied on load and its backward (csrc/pool.hip, csrc/bc_pool.hip), and the activation-materialising kernel (csrc/bn_act.hip).
Plain float64 torch on channels-last values [B][HW][C]; tests/test_pool_gpu.py compares the kernels with it (there the same code runs on the
device tensors, in float64), tests/test_pool_ref.py pins it on its own without a GPU.

What is computed, from the float32 (or bf16) values the kernels are GIVEN, widened to float64:
    skip = stored operand | max(scale_s*(raw - mean_s) + beta_s, 0) for a raw residual operand | 0
    pre  = scale*(y - mean) + beta + skip          a = max(pre, 0)          feat = mean_hw(a)
    g    = gfeat/HW * [pre > 0]                    partial columns sum(g), sum(g*(y - mean))          gmax = max|g|
The bf16-compute pair applies the map as one fma, scale*y + (beta - scale*mean) (tests/test_bc_kernels_gpu.py, _fwd_map): the same
function of the same inputs, so it has the same float64 reference and differs only in where its float32 roundings fall.

Every tolerance is derived from u = 2^-24, the unit roundoff of float32, and
    terms = |scale|*(|y| + |mean|) + |beta| + |skip|      (+ |scale_s|*(|raw| + |mean_s|) + |beta_s| with a raw operand),
which bounds every intermediate of the map, so each float32 operation on the way to `pre` errs by at most u*terms:
  * pre: subtraction, fma, addition of the skip (3 roundings; the raw operand's own subtraction and fma make 5; the one-fma form has
    3: the shift, the fma, the skip) - at most 5u*terms, inside the 8u*terms of the either-side rule below;
  * activation (ttk_bn_act): max(., 0) is 1-Lipschitz and exact: |a - ref| <= 4u*terms (3 roundings + 1 for second-order terms);
  * features: the 3 roundings above, an HW-term float32 sum in ANY order ((HW - 1)u of sum|a| <= sum(terms)), the rounded 1/HW and the
    multiplication by it: (HW + 4)u*mean_hw(terms) to first order, (HW + 6)u with the raw operand's two more roundings and the
    second-order terms ((HW + 6)^2 u^2 / 2 < u for HW < 5000);
  * gradient: rounded 1/HW and one product: |g - gfeat/HW| <= 3u*|gfeat/HW| where pre > 0 (2 roundings + 1); exactly 0 where pre <= 0.
    The bf16 pair rounds g to bf16 once more: one bf16 step, 2^-8 relative (the convention of tests/test_bc_kernels_gpu.py), + 3u.
    2^-8 is also the unit roundoff of bf16 (8 significand bits), so round-to-nearest ATTAINS it for values just above a power of two:
    a correct kernel measures close to 1 of this bound, a truncating one reaches 2;
  * no element is left out: where 0 < |pre| <= 8u*terms the float32 sign of pre may differ from the float64 one, so there g may be 0 or
    the unmasked value and nothing else.  Where pre is EXACTLY 0 in float64 the mask must be closed: with the inputs of make_case that
    happens at the planted elements only (y == mean, beta == 0, skip == 0), where every float32 operation is exact as well;
  * the share of elements accepted by the either-side rule is computed from the reference alone and capped at EITHER_CAP;
  * partial sums, against sums of the kernel's OWN stored g (what the consumer reads): the subtraction y - mean, the product (fused or
    not) and at most N - 1 additions in any order, N = B*HW: (N + 8)u * sum|term| per channel and column (8: the three roundings per
    term, the float64 sum of the float32 rows on this side, second-order terms);
  * gmax: equal, as a float, to max|g| of the stored tensor (a maximum rounds nothing)."""
import types

import torch

U = 2.0 ** -24          # unit roundoff of float32
BF16_STEP = 2.0 ** -8   # one bf16 step, relative (tests/test_bc_kernels_gpu.py: _close_bf16)
EITHER_CAP = 1e-3       # largest share of elements that the either-side rule may accept in one case
SCALE, BETA, MEAN, RSTD, GA, GB, GMEAN, AUX = range(8)  # rows of a BatchNorm constant block (include/ttk.h)
AUX_GMAX = 2

# (B, HW, C) of the fp32 pair and ttk_bn_act (rows = B*HW); the last two cap the grid: backward 41*25*256 = 262 400 items, forward
# 1025*256 = 262 400 items against 1024 workgroups of 256
SHAPES = [(3, 25, 32), (5, 81, 128), (2, 1, 64), (7, 9, 1024), (3, 25, 512)]
SHAPE_BWD_CAPPED = (41, 25, 1024)
SHAPE_FWD_CAPPED = (1025, 4, 1024)
SHAPE_ACT_CAPPED = (4097, 1, 1024)  # ttk_bn_act: 4097*256 = 1 048 832 items against 4096 workgroups of 256
SKIPS = ("none", "stored", "raw")
# bf16-compute pair: C = 192, 320, 1536 leave threads of a workgroup idle (256 is no multiple of C/8)
BC_CHANNELS = [64, 192, 320, 1024, 1536, 2048]
BC_PIXELS = [(3, 25), (5, 81)]
BC_BWD_CAPPED = (330, 25, 1024)   # 8250 pixels against 1024 workgroups * 2 slots * 4
BC_FWD_CAPPED = (4097, 2, 2048)   # 4097*256 items against 4096 workgroups of 256


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def bn_block(C, g):
    """A BatchNorm constant block [8][C] (float32) as the other kernel tests draw it; row AUX zero."""
    bn = torch.zeros(8, C)
    bn[SCALE] = torch.rand(C, generator=g) + 0.5
    bn[BETA] = torch.randn(C, generator=g) * 0.2
    bn[MEAN] = torch.randn(C, generator=g) * 0.3
    bn[RSTD] = torch.rand(C, generator=g) + 0.5
    bn[GA] = torch.rand(C, generator=g) + 0.5
    bn[GB] = torch.randn(C, generator=g) * 0.2
    bn[GMEAN] = torch.randn(C, generator=g) * 0.05
    return bn


def make_case(B, HW, C, skip, bf16=False):
    """Inputs of one case (CPU, float32 holders; with bf16 the activation-sized tensors hold bf16 values): y, gfeat, bn and - skip ==
    "stored" - a non-negative stored residual operand or - "raw" - a raw convolution output with its own BatchNorm block.

    Channel z has beta = 0 and PLANTED pixels with y == mean exactly and a residual operand of exactly 0 (stored: 0; raw: raw == mean_s
    with beta_s = 0): there pre = 0 in float32 and in float64, so the strict `> 0` of the mask is decided deterministically (a = 0,
    g = 0).  (One-fma form: scale and mean of channel z are bf16 values, so scale*mean is exact in float32, the shift is its exact
    negative and fma(scale, mean, shift) = 0.)  The planted pixels are every pixel of sample 0 and, for B > 1 and HW > 1, the first
    and last pixel of the last sample; gfeat[0][z] is four times the largest other |gfeat|, so max|g| taken before masking is wrong."""
    assert skip in SKIPS and not (bf16 and skip == "raw")
    g = torch.Generator().manual_seed(1000003 * B + 1009 * HW + C + 17 * SKIPS.index(skip) + (5 if bf16 else 0))
    rnd = lambda *s: torch.randn(*s, generator=g)
    c = types.SimpleNamespace(B=B, HW=HW, C=C, kind=skip, bf16=bf16, skip=None, raw=None, bn_skip=None)
    c.y, c.bn, c.z = rnd(B, HW, C), bn_block(C, g), (7 * B + HW) % C
    c.planted = torch.zeros(B, HW, dtype=torch.bool)
    c.planted[0] = True
    if B > 1 and HW > 1:
        c.planted[B - 1, 0] = c.planted[B - 1, HW - 1] = True
    c.bn[BETA, c.z] = 0.0
    if bf16:
        c.y = bf16_round(c.y)
        c.bn[SCALE, c.z], c.bn[MEAN, c.z] = bf16_round(c.bn[SCALE, c.z]), bf16_round(c.bn[MEAN, c.z])
    c.y[:, :, c.z][c.planted] = c.bn[MEAN, c.z]
    if skip == "stored":
        c.skip = rnd(B, HW, C).abs()
        if bf16:
            c.skip = bf16_round(c.skip)
        c.skip[:, :, c.z][c.planted] = 0.0
    elif skip == "raw":
        c.raw, c.bn_skip = rnd(B, HW, C), bn_block(C, g)
        c.bn_skip[BETA, c.z] = 0.0
        c.raw[:, :, c.z][c.planted] = c.bn_skip[MEAN, c.z]
    c.gfeat = rnd(B, C)
    c.gfeat[0, c.z] = 0.0
    c.gfeat[0, c.z] = -4.0 * c.gfeat.abs().max()
    return c


def reference(c, device="cpu"):
    """Everything the kernels are compared with, float64 on `device`: pre, terms, a, feat, the unmasked gradient g_un, the mask `pos`,
    g = g_un*pos, the either-side set, its share, and the tolerances of the features and the activation."""
    d = lambda t: t.to(device).double()
    y, bn, gfeat = d(c.y), d(c.bn), d(c.gfeat)
    sc, be, mu = bn[SCALE], bn[BETA], bn[MEAN]
    terms = sc.abs() * (y.abs() + mu.abs()) + be.abs()
    skip = 0.0
    if c.raw is not None:
        raw, bs = d(c.raw), d(c.bn_skip)
        skip = (bs[SCALE] * (raw - bs[MEAN]) + bs[BETA]).clamp_min(0.0)
        terms = terms + skip + bs[SCALE].abs() * (raw.abs() + bs[MEAN].abs()) + bs[BETA].abs()
    elif c.skip is not None:
        skip = d(c.skip)
        terms = terms + skip.abs()
    r = types.SimpleNamespace(y=y, mean=mu, terms=terms)
    r.pre = sc * (y - mu) + be + skip
    r.a = r.pre.clamp_min(0.0)
    r.act_tol = 4.0 * U * terms                          # 3 roundings + 1 (module docstring)
    r.feat = r.a.mean(1)
    r.feat_tol = (c.HW + 6) * U * terms.mean(1)          # HW-term sum in any order, the map, the rounded 1/HW (module docstring)
    r.pos = r.pre > 0
    r.either = (r.pre != 0) & (r.pre.abs() <= 8.0 * U * terms)  # at most 5 roundings of at most u*terms each; 8 leaves second order room
    r.share = float(r.either.double().mean())
    r.g_un = (gfeat / c.HW)[:, None, :].expand(c.B, c.HW, c.C)
    r.g = r.g_un * r.pos
    return r


def _worst(err, tol):
    """max err/tol; an error at tolerance 0 is infinitely far out, none is 0.  NaN propagates (and fails every `<= 1`)."""
    inf, zero = torch.full_like(err, float("inf")), torch.zeros_like(err)
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, zero, inf))
    ratio = torch.where(torch.isnan(err), err, ratio)
    return float(ratio.max()) if not torch.isnan(ratio).any() else float("nan")


def ratio_feat(feat, r):
    return _worst((feat.double() - r.feat).abs(), r.feat_tol)


def ratio_act(a, r):
    return _worst((a.double() - r.a).abs(), r.act_tol)


G_REL_FP32 = 3.0 * U               # rounded 1/HW, one product, + 1 (module docstring)
G_REL_BF16 = BF16_STEP + 3.0 * U   # ... and one rounding to bf16: one bf16 step (tests/test_bc_kernels_gpu.py)


def ratio_g(got, r, rel):
    """Worst error/bound of the stored gradient `got` [B][HW][C] (channels-last values): where the mask is open |got - gfeat/HW| against
    rel*|gfeat/HW|; where it is closed anything but 0 is infinitely far out; in the either-side set the better of the two."""
    got = got.double()
    inf, zero = torch.full_like(got, float("inf")), torch.zeros_like(got)
    err, tol = (got - r.g_un).abs(), rel * r.g_un.abs()
    opened = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, zero, inf))
    closed = torch.where(got == 0, zero, inf)
    ratio = torch.where(r.either, torch.minimum(opened, closed), torch.where(r.pos, opened, closed))
    ratio = torch.where(torch.isnan(got), got, ratio)
    return float(ratio.max()) if not torch.isnan(ratio).any() else float("nan")


def ratio_partials(part, g_stored, r):
    """(ratio of column 0, ratio of column 1): the float32 partial rows `part` [rows][2][C], summed in float64, against the sums of
    g and g*(y - mean) of the STORED gradient; bound (N + 8)u * sum|term| per channel, N = B*HW (module docstring)."""
    gs = g_stored.double()
    n = gs.shape[0] * gs.shape[1]
    s = part.double().sum(0)
    out = []
    for k, term in enumerate((gs, gs * (r.y - r.mean))):
        out.append(_worst((s[k] - term.sum((0, 1))).abs(), (n + 8) * U * term.abs().sum((0, 1))))
    return tuple(out)


def gmax_of(g_stored):
    """max|g| of the stored tensor as a float32 value (exact: the maximum of float32 / bf16 values)."""
    return float(g_stored.float().abs().max())
