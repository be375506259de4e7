"""The kernels between the backbone and the heads against float64 (tests/pool_ref.py: the reference, the derivation of every bound,
the inputs with their planted exact zeros; tests/test_pool_ref.py: the reference on its own):
  * ttk_avgpool_fwd / ttk_avgpool_bwd in their three layouts, ttk_avgpool_fwd_rawskip / ttk_avgpool_bwd_rawskip (csrc/pool.hip);
  * ttk_bc_avgpool_fwd / ttk_bc_avgpool_bwd / ttk_bc_partial_rows_pool (csrc/bc_pool.hip);
  * ttk_bn_act (csrc/bn_act.hip);  ttk_transpose (csrc/pwconv.hip) against torch.
Every output buffer starts as NaN and must be finite afterwards; every call runs twice on fresh buffers and must repeat bit for bit (no
float atomics here: TTK_AUX_GMAX is an integer maximum).  Each case prints its worst error/bound ratio per quantity ("RATIO ...");
the worst seen on the MI355X are recorded in profiles/pool_float64.txt."""
import functools

import pytest
import torch

import pool_ref as R

pytestmark = pytest.mark.gpu

LAYOUT_BLOCKS32, LAYOUT_ROWS, LAYOUT_CB64 = 0, 4, 8  # the layout bits of the pooling pair's flag argument (include/ttk.h)
NAN = float("nan")


def _layout(flag):
    """(channels-last values -> storage order, and back) of one layout flag."""
    import trackertraincode._hip as hip

    if flag == LAYOUT_ROWS:
        return (lambda t: t.contiguous()), (lambda t: t)
    return (hip.to_blocks, hip.from_blocks) if flag == LAYOUT_BLOCKS32 else (hip.to_blocks64, hip.from_blocks64)


@functools.lru_cache(maxsize=2)
def _case(shape, kind, bf16=False):
    """Inputs and float64 reference (on the device) of one case: computed once, shared by the layouts, never written."""
    c = R.make_case(*shape, kind, bf16=bf16)
    r = R.reference(c, "cuda")
    assert r.share <= R.EITHER_CAP  # from the reference alone
    return c, r


def _materialise(raw_blocks, bn_skip, C):
    """x = relu(bn_skip(raw)) through ttk_bn_act (plain rows out) -> channel blocks of 32: the stored form of a raw residual operand."""
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    x = torch.full(raw_blocks.shape, NAN, device="cuda")
    L.call("ttk_bn_act", p(raw_blocks), p(bn_skip), None, p(x), raw_blocks.numel() // C, C)
    torch.cuda.synchronize()
    assert torch.isfinite(x).all()
    return hip.to_blocks(x)


def _bits(t):
    return t.view(torch.int32)


def _report(what, shape, kind, layout, **ratios):
    print("RATIO", what, shape, kind, f"layout {layout}", {k: f"{v:.3f}" for k, v in ratios.items()})
    for k, v in ratios.items():
        assert v <= 1.0, (what, k, v)


# (skip form, layout flag): the raw-skip entry points take no flag (channel blocks of 32)
FORMS = [(k, f) for f in (LAYOUT_BLOCKS32, LAYOUT_ROWS, LAYOUT_CB64) for k in ("none", "stored")] + [("raw", LAYOUT_BLOCKS32)]


def _fp32_cases(shapes):
    return [(s, k, f) for s in shapes for k, f in FORMS if not (f == LAYOUT_CB64 and s[2] < 64)]


_ids = lambda v: str(v).replace(" ", "")


@pytest.mark.parametrize("shape,kind,layout", _fp32_cases(R.SHAPES + [R.SHAPE_FWD_CAPPED]), ids=_ids)
def test_avgpool_forward_against_float64(shape, kind, layout):
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    B, HW, C = shape
    c, r = _case(shape, kind)
    to, _ = _layout(layout)
    d_y, d_bn = to(c.y.cuda()), c.bn.cuda()
    d_sk = to(c.skip.cuda()) if kind == "stored" else to(c.raw.cuda()) if kind == "raw" else None
    d_bs = c.bn_skip.cuda() if kind == "raw" else None
    runs = []
    for _ in range(2):
        feat = torch.full((B, C), NAN, device="cuda")
        if kind == "raw":
            L.call("ttk_avgpool_fwd_rawskip", p(d_y), p(d_bn), p(d_sk), p(d_bs), p(feat), B, HW, C)
        else:
            L.call("ttk_avgpool_fwd", p(d_y), p(d_bn), p(d_sk), p(feat), B, HW, C, layout)
        torch.cuda.synchronize()
        runs.append(feat)
    assert torch.isfinite(feat).all()
    assert torch.equal(_bits(runs[0]), _bits(runs[1])), "the forward does not repeat bit for bit"
    _report("avgpool_fwd", shape, kind, layout, feat=R.ratio_feat(feat, r))
    assert (feat[0, c.z] == 0).all()  # every pixel of (sample 0, channel z) is a planted exact zero
    if kind == "raw":  # ... and the stored form of the same operand, bit for bit
        feat2 = torch.full((B, C), NAN, device="cuda")
        L.call("ttk_avgpool_fwd", p(d_y), p(d_bn), p(_materialise(d_sk, d_bs, C)), p(feat2), B, HW, C, 0)
        torch.cuda.synchronize()
        assert torch.equal(_bits(feat), _bits(feat2)), "raw and stored residual operand differ"


@pytest.mark.parametrize("shape,kind,layout", _fp32_cases(R.SHAPES + [R.SHAPE_BWD_CAPPED]), ids=_ids)
def test_avgpool_backward_against_float64(shape, kind, layout):
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    B, HW, C = shape
    c, r = _case(shape, kind)
    to, back = _layout(layout)
    d_y, d_gf = to(c.y.cuda()), c.gfeat.cuda()
    d_sk = to(c.skip.cuda()) if kind == "stored" else to(c.raw.cuda()) if kind == "raw" else None
    d_bs = c.bn_skip.cuda() if kind == "raw" else None
    bn0 = c.bn.clone()
    bn0[R.AUX] = torch.arange(1, C + 1) * 0.37  # the other slots of row AUX hold something to keep
    bn0 = bn0.cuda()
    rows = L.partial_rows_elementwise(B * HW * (C // 4))
    assert rows == min(-(-B * HW * (C // 4) // 256), 1024)

    def run(start, with_part=True, skip_op=d_sk, raw=(kind == "raw")):
        bn = bn0.clone()
        bn[R.AUX, R.AUX_GMAX] = start
        g = torch.full((B, HW, C), NAN, device="cuda")
        part = torch.full((rows, 2, C), NAN, device="cuda") if with_part else None
        if raw:
            L.call("ttk_avgpool_bwd_rawskip", p(d_gf), p(d_y), p(bn), p(skip_op), p(d_bs), p(g), p(part), B, HW, C)
        else:
            L.call("ttk_avgpool_bwd", p(d_gf), p(d_y), p(bn), p(skip_op), p(g), p(part), B, HW, C, layout)
        torch.cuda.synchronize()
        return g, part, bn

    g, part, bn = run(0.0)
    g2, part2, bn2 = run(0.0)
    assert torch.isfinite(g).all() and torch.isfinite(part).all() and torch.isfinite(bn).all()
    assert all(torch.equal(_bits(u), _bits(v)) for u, v in ((g, g2), (part, part2), (bn, bn2))), "the backward does not repeat bit for bit"
    got = back(g)
    p0, p1 = R.ratio_partials(part, got, r)
    _report("avgpool_bwd", shape, kind, layout, g=R.ratio_g(got, r, R.G_REL_FP32), part0=p0, part1=p1)
    assert (got[:, :, c.z][c.planted.cuda()] == 0).all(), "pre == 0 exactly: the mask is `> 0`"
    # TTK_AUX_GMAX: max|g| of the stored tensor as a float, from a slot that starts at 0, at half of it and at twice it
    true = R.gmax_of(g)
    assert true > 0 and float(bn[R.AUX, R.AUX_GMAX]) == true
    assert true < float(c.gfeat.abs().max()) / HW  # (the largest |gfeat| sits on a masked sample: a maximum taken before masking differs)
    keep = torch.ones(8, C, dtype=torch.bool, device="cuda")
    keep[R.AUX, R.AUX_GMAX] = False
    assert torch.equal(_bits(bn)[keep], _bits(bn0)[keep]), "the backward wrote into bn outside TTK_AUX_GMAX"
    for start in (0.5 * true, 2.0 * true):
        gs, ps, bs = run(start)
        want = torch.tensor(max(start, true), device="cuda")
        assert torch.equal(_bits(bs[R.AUX, R.AUX_GMAX]), _bits(want)), ("GMAX", start, true, float(bs[R.AUX, R.AUX_GMAX]))
        assert torch.equal(_bits(gs), _bits(g)) and torch.equal(_bits(ps), _bits(part)) and torch.equal(_bits(bs)[keep], _bits(bn0)[keep])
    # part = NULL: the same g and GMAX
    gn, _, bnn = run(0.0, with_part=False)
    assert torch.equal(_bits(gn), _bits(g)) and torch.equal(_bits(bnn), _bits(bn)), "part = NULL changes g or bn"
    if kind == "raw":  # the stored form of the same operand, bit for bit
        gs, ps, bs = run(0.0, skip_op=_materialise(d_sk, d_bs, C), raw=False)
        assert torch.equal(_bits(gs), _bits(g)) and torch.equal(_bits(ps), _bits(part)) and torch.equal(_bits(bs), _bits(bn))


@pytest.mark.parametrize("kind", ["none", "stored"])
@pytest.mark.parametrize("shape", R.SHAPES + [R.SHAPE_BWD_CAPPED, R.SHAPE_FWD_CAPPED, R.SHAPE_ACT_CAPPED], ids=_ids)
def test_bn_act_against_float64(shape, kind):
    """ttk_bn_act on rows = B*HW pixels: channel blocks of 32 in, plain channels-last rows out."""
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    B, HW, C = shape
    c, r = _case(shape, kind)
    d_y, d_bn = hip.to_blocks(c.y.cuda()), c.bn.cuda()
    d_sk = hip.to_blocks(c.skip.cuda()) if kind == "stored" else None
    runs = []
    for _ in range(2):
        a = torch.full((B, HW, C), NAN, device="cuda")
        L.call("ttk_bn_act", p(d_y), p(d_bn), p(d_sk), p(a), B * HW, C)
        torch.cuda.synchronize()
        runs.append(a)
    assert torch.isfinite(a).all() and torch.equal(_bits(runs[0]), _bits(runs[1]))
    _report("bn_act", shape, kind, "-", act=R.ratio_act(a, r))
    assert (a[r.pre == 0] == 0).all() and int((r.pre == 0).sum()) >= HW  # the planted exact zeros
    assert (a >= 0).all() and float(a.max()) > 0


BC = [((B, HW, C), k) for C in R.BC_CHANNELS for B, HW in R.BC_PIXELS for k in ("none", "stored")]


def _bc_operands(c):
    import trackertraincode._hip as hip

    blk = lambda t: None if t is None else hip.to_blocks64(t.to(torch.bfloat16).cuda())  # (the values are bf16 already: exact)
    return blk(c.y), blk(c.skip), c.bn.cuda(), c.gfeat.cuda()


@pytest.mark.parametrize("shape,kind", BC + [(R.BC_FWD_CAPPED, "none")], ids=_ids)
def test_bc_avgpool_forward_against_float64(shape, kind):
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    B, HW, C = shape
    c, r = _case(shape, kind, True)
    d_y, d_sk, d_bn, _ = _bc_operands(c)
    runs = []
    for _ in range(2):
        feat = torch.full((B, C), NAN, device="cuda")
        L.call("ttk_bc_avgpool_fwd", p(d_y), p(d_bn), p(d_sk), p(feat), B, HW, C)
        torch.cuda.synchronize()
        runs.append(feat)
    assert torch.isfinite(feat).all() and torch.equal(_bits(runs[0]), _bits(runs[1]))
    _report("bc_avgpool_fwd", shape, kind, "cb64/bf16", feat=R.ratio_feat(feat, r))
    assert (feat[0, c.z] == 0).all()


@pytest.mark.parametrize("shape,kind", BC + [(R.BC_BWD_CAPPED, "stored")], ids=_ids)
def test_bc_avgpool_backward_against_float64(shape, kind):
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    B, HW, C = shape
    c, r = _case(shape, kind, True)
    d_y, d_sk, d_bn, d_gf = _bc_operands(c)
    slots = 256 // (C // 8)
    rows = L.cdll.ttk_bc_partial_rows_pool(B, HW, C)
    assert rows == min(-(-B * HW // (slots * 4)), 1024)
    if shape == R.BC_BWD_CAPPED:
        assert rows == 1024 and B * HW > rows * slots * 4  # the block's pixel loop strides by the whole grid

    def run(with_part=True):
        g = torch.full((B, HW, C), NAN, dtype=torch.bfloat16, device="cuda")
        part = torch.full((rows, 2, C), NAN, device="cuda") if with_part else None
        bn = d_bn.clone()
        L.call("ttk_bc_avgpool_bwd", p(d_gf), p(d_y), p(bn), p(d_sk), p(g), p(part), B, HW, C)
        torch.cuda.synchronize()
        assert torch.equal(_bits(bn), _bits(d_bn))  # const here: GMAX is the fp32 path's business
        return g, part

    g, part = run()
    g2, part2 = run()
    gn, _ = run(with_part=False)
    bits16 = lambda t: t.view(torch.int16)
    assert torch.isfinite(g.float()).all() and torch.isfinite(part).all()
    assert torch.equal(bits16(g), bits16(g2)) and torch.equal(_bits(part), _bits(part2)), "the backward does not repeat bit for bit"
    assert torch.equal(bits16(g), bits16(gn)), "part = NULL changes g"
    got = hip.from_blocks64(g).float()
    p0, p1 = R.ratio_partials(part, got, r)
    _report("bc_avgpool_bwd", shape, kind, "cb64/bf16", g=R.ratio_g(got, r, R.G_REL_BF16), part0=p0, part1=p1)
    assert (got[:, :, c.z][c.planted.cuda()] == 0).all(), "pre == 0 exactly: the mask is `> 0`"


def test_bc_partial_rows_pool_domain():
    import trackertraincode._hip as hip
    rows = hip.lib().cdll.ttk_bc_partial_rows_pool
    for B, HW, C in ((3, 25, 32), (3, 25, 96), (3, 25, 2112), (0, 25, 64)):
        assert rows(B, HW, C) == -1, (B, HW, C)
    assert rows(1, 1, 64) == 1 and rows(3, 25, 2048) == 19 and rows(330, 25, 1024) == 1024


def test_refusals_before_any_launch():
    """Channel counts outside each family's domain and null tensors: RuntimeError from the argument checks, nothing written."""
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    t = torch.zeros(1 << 16, device="cuda")
    out = torch.full((1 << 16,), NAN, device="cuda")
    for C in (48, 2048):
        with pytest.raises(RuntimeError):
            L.call("ttk_avgpool_fwd", p(t), p(t), None, p(out), 2, 4, C, 0)
        with pytest.raises(RuntimeError):
            L.call("ttk_avgpool_bwd", p(t), p(t), p(t), None, p(out), p(out), 2, 4, C, 0)
        with pytest.raises(RuntimeError):
            L.call("ttk_avgpool_fwd_rawskip", p(t), p(t), p(t), p(t), p(out), 2, 4, C)
        with pytest.raises(RuntimeError):
            L.call("ttk_avgpool_bwd_rawskip", p(t), p(t), p(t), p(t), p(t), p(out), p(out), 2, 4, C)
        with pytest.raises(RuntimeError):
            L.call("ttk_bn_act", p(t), p(t), None, p(out), 8, C)
    with pytest.raises(RuntimeError):
        L.call("ttk_bc_avgpool_fwd", p(t), p(t), None, p(out), 2, 4, 32)
    with pytest.raises(RuntimeError):
        L.call("ttk_bc_avgpool_bwd", p(t), p(t), p(t), None, p(out), p(out), 2, 4, 32)
    for null in range(3):  # y, bn, feat / a
        a = [p(t), p(t), p(out)]
        a[null] = None
        with pytest.raises(RuntimeError, match="null pointer"):
            L.call("ttk_avgpool_fwd", a[0], a[1], None, a[2], 2, 4, 64, 0)
        with pytest.raises(RuntimeError, match="null pointer"):
            L.call("ttk_avgpool_fwd_rawskip", a[0], a[1], p(t), p(t), a[2], 2, 4, 64)
        with pytest.raises(RuntimeError, match="null pointer"):
            L.call("ttk_bc_avgpool_fwd", a[0], a[1], None, a[2], 2, 4, 64)
        with pytest.raises(RuntimeError, match="null pointer"):
            L.call("ttk_bn_act", a[0], a[1], None, a[2], 8, 64)
        with pytest.raises(RuntimeError, match="null pointer"):  # backward: y, bn, g
            L.call("ttk_avgpool_bwd", p(t), a[0], a[1], None, a[2], None, 2, 4, 64, 0)
        with pytest.raises(RuntimeError, match="null pointer"):
            L.call("ttk_bc_avgpool_bwd", p(t), a[0], a[1], None, a[2], None, 2, 4, 64)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and (t == 0).all()


@pytest.mark.parametrize("rows,cols", [(1, 1), (31, 33), (32, 32), (1024, 32), (257, 1000)])
def test_transpose_equals_torch(rows, cols):
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    src = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + cols)).cuda()
    out = torch.full((cols, rows), NAN, device="cuda")
    L.call("ttk_transpose", p(src), p(out), rows, cols)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(src.t().contiguous()))
