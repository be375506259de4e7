"""The float64 reference of the pooling / activation tests (tests/pool_ref.py) on its own, without a GPU: it is autograd's pooling, a
correct float32 implementation passes every bound at every shape of tests/test_pool_gpu.py, and the same implementation with ONE
planted error is rejected - so that a failure of tests/test_pool_gpu.py indicts the kernel and a pass means something."""
import functools

import pytest
import torch

import pool_ref as R

FP32_CASES = [(s, k) for s in R.SHAPES + [R.SHAPE_BWD_CAPPED, R.SHAPE_FWD_CAPPED, R.SHAPE_ACT_CAPPED] for k in R.SKIPS]
BC_CASES = [((B, HW, C), k) for C in R.BC_CHANNELS for B, HW in R.BC_PIXELS for k in ("none", "stored")]
BC_CASES += [(R.BC_BWD_CAPPED, "stored"), (R.BC_FWD_CAPPED, "none")]
FAULTS = ("drop_last_pixel", "divisor", "neighbour_bn", "neighbour_gfeat", "mask_ge", "omit_row", "gmax_unmasked")


@functools.lru_cache(maxsize=2)
def _case(shape, kind, bf16):
    c = R.make_case(*shape, kind, bf16=bf16)
    return c, R.reference(c)


def _fma(a, b, c):
    """float32 fma: the product of two float32 values is exact in float64; the sum is rounded to 53 bits and then to 24 (a double
    rounding that differs from the fused one only on a tie of the second)."""
    return (a.double() * b.double() + c.double()).float()


def emulate(c, fault=None, rows=3):
    """The kernels' arithmetic in float32 on the CPU: subtract-first map (fp32 pair, ttk_bn_act) or the one-fma map on bf16 tensors
    (bf16-compute pair), a serial sum over the pixels, the rounded 1/HW, partial sums of the stored gradient in `rows` rows.
    `fault`: one planted error.  -> feat [B][C], a [B][HW][C], g [B][HW][C], part [rows][2][C], gmax."""
    bn, gfeat = c.bn, c.gfeat
    if fault == "neighbour_bn":
        bn = bn.roll(1, dims=1)
    if fault == "neighbour_gfeat":
        gfeat = gfeat.roll(1, dims=0)
    sc, be, mu = bn[R.SCALE], bn[R.BETA], bn[R.MEAN]
    pre = _fma(sc, c.y, _fma(-sc, mu, be)) if c.bf16 else _fma(sc, c.y - mu, be)
    if c.raw is not None:
        bs = c.bn_skip
        pre = pre + _fma(bs[R.SCALE], c.raw - bs[R.MEAN], bs[R.BETA]).clamp_min(0.0)
    elif c.skip is not None:
        pre = pre + c.skip
    a = pre.clamp_min(0.0)
    s = torch.zeros(c.B, c.C)
    for p in range(c.HW - (fault == "drop_last_pixel")):
        s = s + a[:, p]
    inv = torch.tensor(1.0) / torch.tensor(float(c.HW + (fault == "divisor")))
    feat = s * inv
    g_un = (gfeat * inv)[:, None, :].expand(c.B, c.HW, c.C)
    g = torch.where(pre >= 0 if fault == "mask_ge" else pre > 0, g_un, torch.zeros(()))
    if fault == "drop_last_pixel":
        g[:, -1] = 0.0
    if c.bf16:
        g = R.bf16_round(g)
    gmax = float((g_un if fault == "gmax_unmasked" else g).abs().max())
    n = c.B * c.HW
    t1 = g.reshape(n, c.C)
    t2 = t1 * (c.y - mu).reshape(n, c.C)
    part = torch.stack([torch.stack([t1[i].sum(0), t2[i].sum(0)]) for i in torch.tensor_split(torch.arange(n), rows)])
    if fault == "omit_row":
        part = part[1:]
    return feat, a, g, part, gmax


def verdict(c, r, out):
    """{quantity: worst error/bound} of one (emulated or real) set of outputs; gmax: 0 when equal to max|g| of the stored tensor."""
    feat, a, g, part, gmax = out
    p0, p1 = R.ratio_partials(part, g, r)
    return {"feat": R.ratio_feat(feat, r), "act": R.ratio_act(a, r), "g": R.ratio_g(g, r, R.G_REL_BF16 if c.bf16 else R.G_REL_FP32),
            "part0": p0, "part1": p1, "gmax": 0.0 if gmax == R.gmax_of(g) else float("inf")}


@pytest.mark.parametrize("kind", R.SKIPS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_reference_is_autograd_of_the_pooled_activation(shape, kind):
    """(a) feat and g against torch.autograd through AdaptiveAvgPool2d(1) of relu(bn(y) + skip), float64."""
    c, r = _case(shape, kind, False)
    B, HW, C = shape
    f = lambda t: t.double()
    y = f(c.y).requires_grad_()
    bn = f(c.bn)
    # (eval-mode batch_norm with weight = scale, running_var = 1 - eps: exactly scale*(y - mean) + beta up to float64 rounding)
    lin = lambda t, b: (t - b[R.MEAN]) * b[R.SCALE] + b[R.BETA]
    skip = 0.0 if kind == "none" else f(c.skip) if kind == "stored" else torch.relu(lin(f(c.raw), f(c.bn_skip)))
    act = torch.relu(lin(y, bn) + skip)                       # [B][HW][C]
    feat = torch.nn.AdaptiveAvgPool2d(1)(act.permute(0, 2, 1).reshape(B, C, HW, 1)).view(B, C)
    feat.backward(f(c.gfeat))
    # float64 on both sides: 2^-53 per operation, HW + 4 operations, of the same magnitudes as in the float32 bound
    tol = r.feat_tol * 2.0 ** -29
    assert ((feat.detach() - r.feat).abs() <= tol).all()
    # autograd's gradient w.r.t. pre is w.r.t. y divided by scale (scale >= 0.5): the mask and gfeat/HW, one float64 rounding each way
    got = y.grad / bn[R.SCALE]
    assert ((got - r.g).abs() <= 4 * 2.0 ** -53 * r.g_un.abs()).all()
    assert (r.g[0, :, c.z] == 0).all() and (r.a[0, :, c.z] == 0).all() and (r.pre[:, :, c.z][c.planted] == 0).all()
    assert (r.g != 0).any() and r.pos.double().mean() > 0.2


@pytest.mark.parametrize("shape,kind", FP32_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_float32_emulation_passes_every_bound(shape, kind):
    """(b) + (d), fp32 pair and ttk_bn_act: every ratio <= 1, the either-side share under its cap."""
    c, r = _case(shape, kind, False)
    v = verdict(c, r, emulate(c))
    print("RATIO emulation fp32", shape, kind, {k: f"{x:.3f}" for k, x in v.items()}, f"either-side share {r.share:.2e}")
    assert r.share <= R.EITHER_CAP
    assert all(x <= 1.0 for x in v.values()), v


@pytest.mark.parametrize("shape,kind", BC_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_bf16_emulation_passes_every_bound(shape, kind):
    """(b) + (d), bf16-compute pair: bf16 tensors, the one-fma map, g rounded to bf16."""
    c, r = _case(shape, kind, True)
    v = verdict(c, r, emulate(c))
    print("RATIO emulation bf16", shape, kind, {k: f"{x:.3f}" for k, x in v.items()}, f"either-side share {r.share:.2e}")
    assert r.share <= R.EITHER_CAP
    assert all(x <= 1.0 for x in v.values()), v


def test_bf16_gradient_bound_is_round_to_nearest():
    """The bf16 gradient bound is bf16's unit roundoff: rounding to nearest comes close to it (so ratios near 1 are what a correct
    kernel measures), chopping the low 16 bits instead exceeds it."""
    c, r = _case((5, 81, 192), "stored", True)
    g_un = torch.where(r.pos, (c.gfeat * (torch.tensor(1.0) / torch.tensor(float(c.HW))))[:, None, :].expand(c.B, c.HW, c.C), torch.zeros(()))
    nearest = R.ratio_g(R.bf16_round(g_un), r, R.G_REL_BF16)
    chopped = R.ratio_g((g_un.contiguous().view(torch.int32) & -65536).view(torch.float32), r, R.G_REL_BF16)
    assert 0.9 < nearest <= 1.0 < chopped < 2.0, (nearest, chopped)


# which quantity each planted error must push past its bound
BROKEN = {"drop_last_pixel": ("feat", "g"), "divisor": ("feat", "g"), "neighbour_bn": ("feat", "act"), "neighbour_gfeat": ("g",),
          "mask_ge": ("g",), "omit_row": ("part0", "part1"), "gmax_unmasked": ("gmax",)}


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_planted_errors_are_rejected(shape, bf16, fault):
    """(c) One planted error each: the quantities it touches leave their bounds, at every small shape, in both arithmetic forms."""
    if bf16 and shape[2] < 64:
        shape = (shape[0], shape[1], 64)  # (the bf16-compute pair starts at C = 64)
    kind = "stored" if bf16 else R.SKIPS[(R.SHAPES.index(shape) if shape in R.SHAPES else 0) % 3]
    c, r = _case(shape, kind, bf16)
    v = verdict(c, r, emulate(c, fault))
    for q in BROKEN[fault]:
        assert not v[q] <= 1.0, (fault, q, v)
    if fault == "mask_ge":  # only the planted exact zeros tell `>=` from `>`: nothing else moves
        assert v["g"] == float("inf") and v["feat"] <= 1.0 and v["act"] <= 1.0
