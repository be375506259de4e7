"""The raw residual operand (include/ttk.h, ABI 32): ttk_dwconv3x3_fwd_rawskip, ttk_dwconv3x3_bwd_data_rawskip, ttk_avgpool_fwd_rawskip and
ttk_avgpool_bwd_rawskip take the residual input of a block as the RAW convolution output that produced it plus that convolution's BatchNorm
block, and form x = relu(bn(s)) on load - the same subtract, fma and max that ttk_bn_act stores.  So every output buffer must be BIT FOR BIT
that of the stored-operand entry point given the materialised x: the cases below assert torch.equal, never a tolerance.  The backbone with
and without stored inputs of the first block of each residual chain (mobilenet_v1._ELIDE_HEAD_INPUT) must agree the same way."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE, BETA, MEAN, RSTD, GA, GB, GMEAN, AUX = range(8)
AUX_GMAX = 2


def _bn(C, g):
    bn = torch.zeros(8, C)
    bn[SCALE] = torch.rand(C, generator=g) + 0.5
    bn[BETA] = torch.randn(C, generator=g) * 0.2
    bn[MEAN] = torch.randn(C, generator=g) * 0.3
    bn[RSTD] = torch.rand(C, generator=g) + 0.5
    bn[GA] = torch.rand(C, generator=g) + 0.5
    bn[GB] = torch.randn(C, generator=g) * 0.2
    bn[GMEAN] = torch.randn(C, generator=g) * 0.05
    return bn.cuda()  # (row AUX zero: the kernels raise it with atomicMax)


def _rnd(g, *shape):
    return torch.randn(*shape, generator=g).cuda()


def _materialise(raw, bn):
    """x = relu(bn(raw)) through ttk_bn_act (raw: channel blocks; the entry point writes plain rows) -> channel blocks again."""
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    C = raw.shape[-1]
    x = torch.full(raw.shape, float("nan"), device="cuda")
    L.call("ttk_bn_act", p(raw), p(bn), None, p(x), raw.numel() // C, C)
    torch.cuda.synchronize()
    assert torch.isfinite(x).all() and float(x.min()) == 0.0 and float(x.max()) > 0.0  # both branches of the relu occur
    return hip.to_blocks(x)


def _same(a, b, what):
    assert torch.isfinite(a).all() and torch.isfinite(b).all(), what
    assert torch.equal(a, b), (what, float((a - b).abs().max()))


# (B, H, W, C, stride, a_out)
FWD = [(3, 33, 33, 32, 1, True),    # bands of one image handed on in LDS (carry mode)
       (5, 9, 9, 64, 1, True),      # several images per tile, ragged last tile, two slabs
       (2, 65, 65, 32, 1, True),    # column tiles
       (3, 33, 33, 64, 2, False),
       (5, 17, 17, 32, 2, False)]


@pytest.mark.parametrize("B,H,W,C,stride,want_a", FWD)
def test_depthwise_forward_raw_equals_stored(B, H, W, C, stride, want_a):
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    g = torch.Generator().manual_seed(7 * B + H + C + stride)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    yprev, raw, w = _rnd(g, B, H, W, C), _rnd(g, B, H, W, C), _rnd(g, C, 1, 3, 3) * 0.3
    bn_prev, bn_skip, pivot = _bn(C, g), _bn(C, g), _rnd(g, C) * 0.5
    x = _materialise(raw, bn_skip)
    rows = L.partial_rows_dwconv(B, H, W, C, stride, False)
    out = []
    for rawskip in (False, True):
        y = torch.full((B, Ho, Wo, C), float("nan"), device="cuda")
        a_out = torch.full((B, H, W, C), float("nan"), device="cuda") if want_a else None
        part = torch.full((rows, 2, C), float("nan"), device="cuda")
        if rawskip:
            L.call("ttk_dwconv3x3_fwd_rawskip", p(yprev), p(bn_prev), p(raw), p(bn_skip), p(a_out), p(w), p(y), p(part), p(pivot), B, H, W, C, stride)
        else:
            L.call("ttk_dwconv3x3_fwd", p(yprev), p(bn_prev), p(x), p(a_out), p(w), p(y), p(part), p(pivot), B, H, W, C, stride, 0)
        torch.cuda.synchronize()
        out.append((y, a_out, part))
    _same(out[0][0], out[1][0], "y")
    _same(out[0][2], out[1][2], "partial sums")
    if want_a:
        _same(out[0][1], out[1][1], "a_out")
        assert float(out[1][1].max()) > 0.0


# the two stride-2 forward shapes, and one stride-1 shape (with the residual gradient); block input recomputed (no a_in) in both forms
# (and a stride-1 image of one band: the instantiation without the ring of LDS rows)
BWD = [(3, 33, 33, 64, 2), (5, 17, 17, 32, 2), (3, 33, 33, 32, 1), (5, 9, 9, 64, 1)]


@pytest.mark.parametrize("B,H,W,C,stride", BWD)
def test_depthwise_backward_raw_equals_stored(B, H, W, C, stride):
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    g = torch.Generator().manual_seed(11 * B + H + C + stride)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    yprev, raw, w = _rnd(g, B, H, W, C), _rnd(g, B, H, W, C), _rnd(g, C, 1, 3, 3) * 0.3
    g_dw, y_dw = _rnd(g, B, Ho, Wo, C), _rnd(g, B, Ho, Wo, C)
    sg = _rnd(g, B, H, W, C) if stride == 1 else None
    bn_prev0, bn_skip, bn_dw = _bn(C, g), _bn(C, g), _bn(C, g)
    x = _materialise(raw, bn_skip)
    rows = L.partial_rows_dwconv(B, H, W, C, stride, True)
    out = []
    for rawskip in (False, True):
        bn_prev = bn_prev0.clone()
        g_prev = torch.full((B, H, W, C), float("nan"), device="cuda")
        part = torch.full((rows, 2, C), float("nan"), device="cuda")
        dw = torch.zeros(C, 9, device="cuda")
        dw_rows = torch.full((rows, C, 9), float("nan"), device="cuda")  # the workgroup-row form (dw_accumulate = 2): order-fixed
        if rawskip:
            L.call("ttk_dwconv3x3_bwd_data_rawskip", p(g_dw), p(y_dw), p(bn_dw), p(w), p(sg), p(yprev), p(bn_prev), p(raw), p(bn_skip), p(g_prev),
                   p(part), p(dw), 2, p(dw_rows), B, H, W, C, stride)
        else:
            L.call("ttk_dwconv3x3_bwd_data", p(g_dw), p(y_dw), p(bn_dw), p(w), p(sg), p(yprev), p(bn_prev), p(x), None, p(g_prev),
                   p(part), p(dw), 2, p(dw_rows), B, H, W, C, stride, 0)
        torch.cuda.synchronize()
        out.append((g_prev, part, bn_prev, dw_rows))
    _same(out[0][0], out[1][0], "g_prev")
    _same(out[0][1], out[1][1], "partial sums")
    _same(out[0][2], out[1][2], "bn_prev (TTK_AUX_GMAX)")
    assert float(out[1][2][AUX, AUX_GMAX]) == float(out[1][0].abs().max()) > 0.0
    _same(out[0][3], out[1][3], "weight-gradient rows")
    assert float((out[1][0] == 0).float().mean()) > 0.05  # the relu mask of the recomputed block input drops gradient


def test_avgpool_raw_equals_stored():
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    B, HW, C = 5, 25, 64
    g = torch.Generator().manual_seed(5)
    y, raw, gfeat = _rnd(g, B, HW, 1, C), _rnd(g, B, HW, 1, C), _rnd(g, B, C)
    bn0, bn_skip = _bn(C, g), _bn(C, g)
    x = _materialise(raw, bn_skip)
    rows = L.partial_rows_elementwise(B * HW * (C // 4))
    out = []
    for rawskip in (False, True):
        bn = bn0.clone()
        feat = torch.full((B, C), float("nan"), device="cuda")
        gy = torch.full((B, HW, 1, C), float("nan"), device="cuda")
        part = torch.full((rows, 2, C), float("nan"), device="cuda")
        if rawskip:
            L.call("ttk_avgpool_fwd_rawskip", p(y), p(bn), p(raw), p(bn_skip), p(feat), B, HW, C)
            L.call("ttk_avgpool_bwd_rawskip", p(gfeat), p(y), p(bn), p(raw), p(bn_skip), p(gy), p(part), B, HW, C)
        else:
            L.call("ttk_avgpool_fwd", p(y), p(bn), p(x), p(feat), B, HW, C, 0)
            L.call("ttk_avgpool_bwd", p(gfeat), p(y), p(bn), p(x), p(gy), p(part), B, HW, C, 0)
        torch.cuda.synchronize()
        out.append((feat, gy, part, bn))
    for a, b, what in zip(out[0], out[1], ("features", "g", "partial sums", "bn (TTK_AUX_GMAX)")):
        _same(a, b, what)
    assert float(out[1][3][AUX, AUX_GMAX]) == float(out[1][1].abs().max()) > 0.0


def test_null_raw_operand_is_refused():
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    t = torch.zeros(8, 32, device="cuda")
    with pytest.raises(RuntimeError, match="null pointer"):
        L.call("ttk_dwconv3x3_fwd_rawskip", p(t), p(t), p(t), None, None, p(t), p(t), None, None, 1, 1, 1, 32, 1)
    with pytest.raises(RuntimeError, match="null pointer"):
        L.call("ttk_avgpool_fwd_rawskip", p(t), p(t), None, p(t), p(t), 1, 1, 32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole backbone
# ---------------------------------------------------------------------------------------------------------------------------------
_B, _HW = 4, 129
_HEADS = [2, 4, 6, 12]  # dw3_1, dw4_1, dw5_1, dw6: the first block of each chain of residual blocks


def _net(blurpool):
    from trackertraincode.backbones.mobilenet_v1 import MobileNet

    torch.manual_seed(0)
    net = MobileNet(num_classes=None, use_blurpool=blurpool).cuda()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for bn in net._bns():
            bn.weight.copy_((torch.rand(bn.weight.shape, generator=g) + 0.5).cuda())
            bn.bias.copy_((torch.randn(bn.bias.shape, generator=g) * 0.3).cuda())
            bn.running_mean.copy_((torch.randn(bn.bias.shape, generator=g) * 0.1).cuda())
            bn.running_var.copy_((torch.rand(bn.bias.shape, generator=g) + 0.5).cuda())
    return net.train()


def _step(net, x, gfeat, frozen):
    """Forward + backward through the launch sequences, from the network's parameters and a COPY of its buffers."""
    from trackertraincode.backbones import mobilenet_v1 as MB

    momentum, eps = net._check(x)
    params = [q.detach() for q in net._flat_params()]
    buffers = [b.clone() for b in net._flat_buffers()]
    feat, ctx = MB._forward_impl(x, params, buffers, momentum, eps, training=not frozen, frozen=frozen, blur=net._blur_weights(), blocks=net._blocks)
    stored = [k for k, (d, a) in enumerate(zip(ctx.dims, ctx.a_in)) if d[7] and a is not None]
    elided = [k for k, (d, a) in enumerate(zip(ctx.dims, ctx.a_in)) if d[7] and a is None]
    grads = MB._backward_impl(ctx, gfeat, params)
    torch.cuda.synchronize()
    return feat, grads, buffers, stored, elided


@pytest.mark.parametrize("blurpool,frozen", [(False, False), (True, False), (False, True)])
def test_backbone_is_bitwise_the_same_without_the_head_inputs(monkeypatch, blurpool, frozen):
    from trackertraincode.backbones import mobilenet_v1 as MB

    monkeypatch.setattr(MB, "_DETERMINISTIC", True)  # every weight-gradient reduction in a fixed order
    net = _net(blurpool)
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(_B, 1, _HW, _HW, generator=g) * 0.5 + 0.2).cuda()
    gfeat = (torch.randn(_B, net.num_features, generator=g) / _B).cuda()
    default = MB._ELIDE_HEAD_INPUT  # the product's setting: a subset of the heads by name
    res = {}
    for elide in (True, False, default):
        monkeypatch.setattr(MB, "_ELIDE_HEAD_INPUT", elide)
        res[elide] = _step(net, x, gfeat, frozen)
    residual = [k for k, (_, cin, cout, stride) in enumerate(net._blocks) if stride == 1 and cin == cout]
    assert res[True][4] == _HEADS and res[True][3] == [k for k in residual if k not in _HEADS]
    assert res[False][4] == [] and res[False][3] == residual
    _same(res[True][0], res[False][0], "features")
    assert len(res[True][1]) == len(res[False][1]) == len(net._flat_params())
    names = ["conv1.weight", "bn1.weight", "bn1.bias"] + [f"{n}.{q}" for n, *_ in net._blocks
                                                          for q in ("dw.weight", "bn_dw.weight", "bn_dw.bias", "pw.weight", "bn_sep.weight", "bn_sep.bias")]
    for name, a, b in zip(names, res[True][1], res[False][1]):
        _same(a, b, name)
    assert any(float(a.abs().max()) > 0 for a in res[True][1])
    for i, (a, b) in enumerate(zip(res[True][2], res[False][2])):
        assert torch.equal(a, b), f"BatchNorm buffer {i}"
    # the product's setting: some of the heads, and the same bits
    names_of = [n for n, *_ in net._blocks]
    assert default is not True and default is not False and set(default) <= {names_of[k] for k in _HEADS}
    assert res[default][4] == [k for k in _HEADS if names_of[k] in default]
    _same(res[default][0], res[False][0], "features (default setting)")
    for name, a, b in zip(names, res[default][1], res[False][1]):
        _same(a, b, name + " (default setting)")
    for i, (a, b) in enumerate(zip(res[default][2], res[False][2])):
        assert torch.equal(a, b), f"BatchNorm buffer {i} (default setting)"


def test_intermediates_are_the_same_without_the_head_inputs(monkeypatch):
    """MobileNet._intermediates materialises a raw residual operand first (dw3_1 and dw6 are heads of a chain)."""
    from trackertraincode.backbones import mobilenet_v1 as MB

    net = _net(False)
    x = (torch.randn(2, 1, _HW, _HW, generator=torch.Generator().manual_seed(3)) * 0.5 + 0.2).cuda()
    outs = {}
    for elide in (True, False):
        monkeypatch.setattr(MB, "_ELIDE_HEAD_INPUT", elide)
        outs[elide] = net._intermediates(x)
        torch.cuda.synchronize()
    assert len(outs[True]) == len(outs[False]) == 5
    for i, (a, b) in enumerate(zip(outs[True], outs[False])):
        _same(a, b, f"intermediate {i}")
