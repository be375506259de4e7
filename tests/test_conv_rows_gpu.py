"""The implicit-GEMM convolutions of the ResNet18 variant through the C ABI, row by row against float64, off the square path
(tests/conv_ref.py: the reference, the yardstick, the criterion and its derivation, the table of cases with the code path each is there
for; tests/test_conv_ref.py: all of that on its own, and the mutations the criterion catches where a whole-tensor norm does not):
  * ttk_conv_weight_repack, ttk_conv_prepare_weights: both operand layouts decoded on the host with the formulas of include/ttk.h;
  * ttk_conv_fwd; ttk_conv_bwd_data raw and masked, from (g, y, bn) and from the planes of ttk_bn_bwd_apply; ttk_conv_bwd_weight with
    atomics, with scratch, and from the planes;
  * the non-GEMM neighbours on non-square and degenerate grids: ttk_stem7_*, ttk_maxpool3x3s2_*, ttk_blur3x3_*.
Every output starts as NaN (a weight gradient: zeros, it accumulates) between two NaN guard bands of 64 elements, must be finite afterwards
and the bands untouched; every call runs twice on fresh buffers and repeats bit for bit (the atomic weight gradient need not).  Where the
float64 scale of an element is zero - every contributing product is zero: zero channels, padding, the odd pixels of a strided 1x1 data
gradient - the device value must be exactly zero.

Each output prints `RATIO <entry> <case> <value>`, value = worst (|x - f64| - floor - 2^-24 s) / (s Y) over its elements (conv_ref.py); the
assertion is value <= MARGIN = 4.  Worst per entry point on the MI355X (profiles/conv_float64.txt has the cases):
    ttk_conv_fwd 1.00 (3x1x43x64x64x3x1)   ttk_conv_bwd_data 0.51 in all four forms (2x10x7x128x256x1x2)
    ttk_conv_bwd_weight 1.03 in all three forms (1x1x1x64x128x3x2)   ttk_stem7_fwd 0.74 (2x20x33)   ttk_stem7_bwd_weight 0.45 (1x7x7)
    ttk_blur3x3_fwd 0.53, _bwd 0.06 (2x2x7x32 stride 2)
Shapes without a kernel are asserted as refusals, outputs still NaN: ttk_conv_bwd_data at Cin = 32 / 96, ttk_bn_bwd_apply at C = 192 (the
planes of those cases are cut on the host), ttk_maxpool3x3s2_* at H = 1, ttk_conv_prepare_weights with 25 tensors or Cin = 48.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 64
_ids = lambda v: "x".join(map(str, v))


class Guard:
    """Output buffers of one launch, each between two guard bands of GUARD elements of its fill value (NaN; 0x7e00 = an fp16 NaN for the
    16-bit operand planes; 0xff for window indices)."""

    def __init__(self):
        self.items = []

    def new(self, *shape, dtype=torch.float32, fill=NAN):
        n = int(np.prod(shape))
        full = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.items.append((full, n, fill))
        return full[GUARD:GUARD + n].view(*shape)

    def zeros(self, *shape):
        v = self.new(*shape)
        v.zero_()
        return v

    def check(self, what):
        torch.cuda.synchronize()
        for full, n, fill in self.items:
            band = torch.cat([full[:GUARD], full[GUARD + n:]])
            ok = band.isnan().all() if fill != fill else (band == fill).all()
            assert bool(ok), f"{what}: written outside a buffer of {n} elements"


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _lib():
    import trackertraincode._hip as hip
    return hip.lib(), hip.ptr


def _judge(entry, case, p, out, masked=False):
    out = np.asarray(out, np.float64)
    assert np.isfinite(out).all(), (entry, case, "NaN left or written")
    ratio, zeros_ok = R.masked_ratio(p, out) if masked else p.ratio(out)
    print("RATIO", entry, _ids(case), f"{ratio:.3f}")
    assert zeros_ok, (entry, case, "an element whose every product is zero (or whose mask is closed) is not exactly zero")
    if not ratio <= R.MARGIN:
        e = (np.abs(out - p.ref) - p.floor - R.U * p.s) / np.where(p.s > 0, p.s * p.Y, np.inf)
        row = int(e.max(1).argmax())
        raise AssertionError((entry, case, f"ratio {ratio:.2f} > {R.MARGIN} in row {row} of {out.shape[0]}", f"Y {p.Y:.2e}"))
    return ratio


def _check_forward_sums(part, y_dev, prod, piv):
    """part[rows][2][C] of a forward kernel: (sum (y - pivot), sum (y - pivot)^2) per channel, as tests/test_conv_gpu.py asserts them -
    against the float64 reference, absolute 3e-5 of the largest channel's sum |y - pivot| and relative 3e-5 - and no NaN left in any row.
    Additionally the second column is held to the squares of the y the kernel STORED (relative 3e-5: the float32 summation alone).
    One exception, derived: with a single row (M = 1, the degenerate strided cases) the "sum" is the one term (y - pivot)^2, and a channel
    whose y lies next to its pivot turns the error e that the row criterion grants y itself (conv_ref.Product.allowed) into the relative
    error 2 e / |y - pivot| of that term, whatever the kernel does.  There - and only on the channels where 2 |y - pivot| e + e^2 alone
    exceeds the 3e-5, which no float32 kernel can meet - that amount is granted on top; all other channels and all cases with more than
    one row keep the assertion as test_conv_gpu.py states it."""
    ps = part.cpu().numpy().astype(np.float64)
    assert np.isfinite(ps).all()  # no NaN left in rows < the partial-row count
    flat = prod.ref - piv.astype(np.float64)
    np.testing.assert_allclose(ps[:, 0].sum(0), flat.sum(0), rtol=0, atol=3e-5 * np.abs(flat).sum(0).max())
    own = np.asarray(y_dev, np.float64) - piv.astype(np.float64)
    np.testing.assert_allclose(ps[:, 1].sum(0), (own ** 2).sum(0), rtol=3e-5)
    want = (flat ** 2).sum(0)
    if flat.shape[0] > 1:
        np.testing.assert_allclose(ps[:, 1].sum(0), want, rtol=3e-5)
        return
    e = prod.allowed()[0]
    moved = 2 * np.abs(flat[0]) * e + e ** 2
    print("SUMS single row: channels granted more than 3e-5:", int((moved > 3e-5 * want).sum()), "of", want.size)
    assert np.all(np.abs(ps[:, 1].sum(0) - want) <= 3e-5 * want + np.where(moved > 3e-5 * want, moved, 0.0))


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=4)
def _operands(case):
    """the case's inputs on the device and its weight operands from ttk_conv_weight_repack (checked by its own test)"""
    L, p = _lib()
    c = R.make_case(case)
    d = dict(a=_t(c.a), w=_t(c.w), a_bound=_t(np.array([c.a_bound], np.float32)), piv=_t(c.piv), g=_t(c.g), y=_t(c.y32), bn=_t(c.bn),
             mask_y=_t(c.mask_y))
    n = c.w.size
    d["wf"], d["wb"] = torch.zeros(3 * n, dtype=torch.int16, device="cuda"), torch.zeros(3 * n, dtype=torch.int16, device="cuda")
    L.call("ttk_conv_weight_repack", p(d["w"]), p(d["wf"]), p(d["wb"]), c.Cout, c.Cin, c.k, c.k)
    G = Guard()
    d["dy"] = G.new(2, c.M, c.Cout, dtype=torch.float16)  # ttk_bn_bwd_apply: the h plane, then the l plane, of dy * 2^s
    if c.Cout & (c.Cout - 1) == 0:
        L.call("ttk_bn_bwd_apply", p(d["g"]), p(d["y"]), p(d["bn"]), p(d["dy"]), c.M, c.Cout)
    else:  # Cout = 192: the elementwise producer takes powers of two only (include/ttk.h) - refused, and the planes are cut on the host
        with pytest.raises(RuntimeError, match="bn_bwd_apply: unsupported shape"):
            L.call("ttk_bn_bwd_apply", p(d["g"]), p(d["y"]), p(d["bn"]), p(d["dy"]), c.M, c.Cout)
        assert bool(d["dy"].isnan().all())
        d["dy"].copy_(torch.from_numpy(np.stack(R.split_f16_bits(c.dy32, R.pow2_scale(c.dy_bound)))))
    G.check("bn_bwd_apply")
    assert bool(torch.isfinite(d["dy"]).all())
    return c, d


def _expected_planes(w, S):
    """(wf[2][T][Cin/32][Cout][32], wb[2][T][Cout/32][Cin][32]) as uint16 bits from w[Cout][Cin][T] (include/ttk.h)"""
    Cout, Cin, T = w.shape
    fwd, bwd = [], []
    for piece in R.split_f16_bits(w, S):
        fwd.append(piece.reshape(Cout, Cin // 32, 32, T).transpose(3, 1, 0, 2))
        bwd.append(piece.reshape(Cout // 32, 32, Cin, T).transpose(3, 0, 2, 1))
    return np.ascontiguousarray(np.stack(fwd)).view(np.uint16), np.ascontiguousarray(np.stack(bwd)).view(np.uint16)


def _check_planes(buf, want, w, what):
    """buf: int16 [3 n] as the device left it; want: the numpy pieces in the buffer's layout; header = max |w|"""
    n = w.size
    got = buf[:2 * n].cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want.reshape(-1)), (what, "pieces differ from numpy's split")
    hdr = buf[2 * n:2 * n + 2].cpu().numpy().view(np.float32)[0]
    assert hdr == np.float32(np.abs(w).max()), (what, "header")


@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_weight_repack_layouts_and_pieces(case):
    L, p = _lib()
    c = R.make_case(case)
    w = c.w.reshape(c.Cout, c.Cin, c.T)
    S = R.pow2_scale(c.w_bound)
    want_f, want_b = _expected_planes(w, S)
    runs = []
    for _ in range(2):
        G = Guard()
        wf, wb = G.new(3 * w.size, dtype=torch.int16, fill=0x7e00), G.new(3 * w.size, dtype=torch.int16, fill=0x7e00)
        d_w = _t(c.w)
        L.call("ttk_conv_weight_repack", p(d_w), p(wf), p(wb), c.Cout, c.Cin, c.k, c.k)
        G.check("conv_weight_repack")
        _check_planes(wf, want_f, w, "w_fwd")
        _check_planes(wb, want_b, w, "w_bwd")
        runs.append((wf[:2 * w.size + 2].clone(), wb[:2 * w.size + 2].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # h + l reproduces w * 2^s to 2^-22 relative (decoded from the device's own planes, layout of include/ttk.h)
    planes = runs[0][0][:2 * w.size].cpu().numpy().view(np.float16).astype(np.float64).reshape(2, c.T, c.Cin // 32, c.Cout, 32)
    back = (planes[0] + planes[1]).transpose(2, 1, 3, 0).reshape(c.Cout, c.Cin, c.T) / S
    assert np.all(np.abs(back - w) <= np.maximum(2.0 ** -22 * np.abs(w), R.floor_abs(w, c.w_bound)))


def test_prepare_weights_equals_repack_per_tensor():
    """One call over a list that mixes k = 1 and k = 3, Cin = 32, an all-zero tensor (scale 1) and a tensor without a data-gradient
    operand; n = 24 is accepted, n = 25 and a Cin of 48 are refused."""
    L, p = _lib()
    rng = np.random.default_rng(11)
    shapes = [(64, 32, 3), (128, 64, 1), (64, 64, 3), (256, 128, 1), (64, 32, 1), (192, 96, 3)]
    ws = [(rng.normal(0, 1, (co, ci, k, k)) * np.sqrt(2.0 / (k * k * co))).astype(np.float32) for co, ci, k in shapes]
    ws[2][:] = 0.0
    no_bwd = 3

    def run(ws, no_bwd):
        G = Guard()
        d_w = [_t(w) for w in ws]
        wf = [G.new(3 * w.size, dtype=torch.int16, fill=0x7e00) for w in ws]
        wb = [None if i == no_bwd else G.new(3 * w.size, dtype=torch.int16, fill=0x7e00) for i, w in enumerate(ws)]
        L.conv_prepare_weights(d_w, wf, wb)
        G.check("conv_prepare_weights")
        return wf, wb

    for ws_, nb in ((ws, no_bwd), ([ws[i % len(ws)] for i in range(24)], None)):
        wf, wb = run(ws_, nb)
        wf2, wb2 = run(ws_, nb)
        for i, w in enumerate(ws_):
            co, ci, k = w.shape[:3]
            n = w.size
            G = Guard()
            rf, rb = G.new(3 * n, dtype=torch.int16, fill=0x7e00), G.new(3 * n, dtype=torch.int16, fill=0x7e00)
            d_w = _t(w)
            L.call("ttk_conv_weight_repack", p(d_w), p(rf), p(rb), co, ci, k, k)
            G.check("conv_weight_repack")
            want_f, want_b = _expected_planes(w.reshape(co, ci, k * k), R.pow2_scale(np.float32(np.abs(w).max())))
            for got, again, ref, want in ((wf[i], wf2[i], rf, want_f), (wb[i], wb2[i], rb, want_b)):
                if got is None:
                    continue
                assert torch.equal(got[:2 * n + 2], ref[:2 * n + 2]), (i, "operand planes or header differ from ttk_conv_weight_repack")
                assert torch.equal(got[:2 * n + 2], again[:2 * n + 2])
                _check_planes(got, want, w, i)
        if nb is not None:
            assert float(wf[2][2 * ws[2].size:2 * ws[2].size + 2].view(torch.float32)[0]) == 0.0 and not bool(wf[2][:2 * ws[2].size].any())
    small = [ws[4]] * 25
    G = Guard()
    bufs = [G.new(3 * ws[4].size, dtype=torch.int16, fill=0x7e00) for _ in range(50)]
    with pytest.raises(RuntimeError, match=r"conv_prepare_weights: bad arguments \(at most 24 tensors\)"):
        L.conv_prepare_weights([_t(w) for w in small], bufs[:25], bufs[25:])
    w48 = np.ones((64, 48, 1, 1), np.float32)
    with pytest.raises(RuntimeError, match="conv_prepare_weights: bad tensor 0"):
        L.conv_prepare_weights([_t(w48)], bufs[:1], bufs[1:2])
    G.check("refused conv_prepare_weights")
    assert all(bool((b == 0x7e00).all()) for b in bufs)


@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_conv_fwd_rows(case):
    L, p = _lib()
    c, d = _operands(case)
    ref = R.forward(case)
    rows = L.partial_rows_gemm(c.M)
    runs = []
    for _ in range(2):
        G = Guard()
        y, part = G.new(c.M, c.Cout), G.new(rows, 2, c.Cout)
        L.call("ttk_conv_fwd", p(d["a"]), p(d["a_bound"]), p(d["wf"]), p(y), p(part), p(d["piv"]), c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.k,
               c.stride, c.pad)
        G.check("conv_fwd")
        runs.append((y, part))
    (y, part), (y2, part2) = runs
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(part), _bits(part2))
    _judge("conv_fwd", case, ref, y.cpu().numpy())
    _check_forward_sums(part, y.cpu().numpy(), ref, c.piv)


@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_conv_bwd_data_rows(case):
    L, p = _lib()
    c, d = _operands(case)
    geo = (c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.stride, c.pad)
    if not R.has_dgrad(case):  # no kernel for Cin = 32, 96: refused before anything is launched
        G = Guard()
        g_in = G.new(c.Min, c.Cin)
        with pytest.raises(RuntimeError, match="conv_bwd_data: unsupported shape"):
            L.call("ttk_conv_bwd_data", p(d["g"]), p(d["y"]), p(d["bn"]), p(d["wb"]), None, None, p(g_in), None, *geo)
        G.check("refused conv_bwd_data")
        assert bool(g_in.isnan().all())
        return
    ref = R.dgrad(case)
    assert ref.share <= R.UNDECIDED_CAP
    # dy as ttk_bn_bwd_apply wrote it: two fp16 planes of dy * 2^s; h + l reproduces it to fp32 rounding (as tests/test_conv_gpu.py)
    S = R.pow2_scale(c.dy_bound)
    planes = d["dy"].double().cpu().numpy()
    np.testing.assert_allclose((planes[0] + planes[1]) / S, c.dy32, rtol=2e-6, atol=1e-6 * float(np.abs(c.dy32).max()))
    rows = L.partial_rows_gemm(c.Min)
    for form, g, y in (("", d["g"], d["y"]), ("_planes", d["dy"], None)):
        runs = []
        for _ in range(2):
            G = Guard()
            raw, masked, part = G.new(c.Min, c.Cin), G.new(c.Min, c.Cin), G.new(rows, 2, c.Cin)
            mbn = _t(c.mbn)
            L.call("ttk_conv_bwd_data", p(g), p(y), p(d["bn"]), p(d["wb"]), None, None, p(raw), None, *geo)
            L.call("ttk_conv_bwd_data", p(g), p(y), p(d["bn"]), p(d["wb"]), p(d["mask_y"]), p(mbn), p(masked), p(part), *geo)
            G.check("conv_bwd_data" + form)
            runs.append((raw, masked, part, mbn))
        for x, x2 in zip(*runs):
            assert torch.equal(_bits(x), _bits(x2)), "conv_bwd_data" + form
        raw, masked, part, mbn = runs[0]
        _judge("conv_bwd_data_raw" + form, case, ref, raw.cpu().numpy())
        out = masked.cpu().numpy()
        _judge("conv_bwd_data_masked" + form, case, ref, out, masked=True)
        assert float(mbn[R.BN_AUX, R.AUX_GMAX]) == float(np.abs(out).max())  # the bound of the next layer's gradient operand
        ps = part.cpu().numpy().astype(np.float64)
        assert np.isfinite(ps).all()
        o64 = out.astype(np.float64)
        np.testing.assert_allclose(ps[:, 0].sum(0), o64.sum(0), rtol=0, atol=3e-5 * np.abs(o64).sum(0).max())
        yc = c.mask_y.astype(np.float64) - c.mbn[R.BN_MEAN]
        np.testing.assert_allclose(ps[:, 1].sum(0), (o64 * yc).sum(0), rtol=0, atol=3e-5 * np.abs(o64 * yc).sum(0).max())


@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_conv_bwd_weight_rows(case):
    L, p = _lib()
    c, d = _operands(case)
    ref = R.wgrad(case)
    geo = (c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.stride, c.pad)
    ncols = c.T * c.Cin
    nb = L.conv_wgrad_partial_bytes(c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.stride)
    assert (nb > 0) == (c.k == 3)  # 1x1 kernels keep the (coalesced) atomics
    if nb:
        assert nb == 4 * c.Cout * ncols * R.wgrad_slices(c.M, c.Cout, ncols)[0]
    if case == R.MULTI_SLICE_CASE:
        assert nb == 4 * c.Cout * ncols * R.MULTI_SLICE_COUNT  # the case cannot silently degrade to one slice
    forms = [("atomic", d["g"], d["y"], False), ("planes", d["dy"], None, bool(nb))] + ([("scratch", d["g"], d["y"], True)] if nb else [])
    for form, g, y, use_scratch in forms:
        runs = []
        for _ in range(2):
            G = Guard()
            dw = G.zeros(c.Cout, c.Cin, c.k, c.k)  # accumulated onto: zeros between the NaN bands
            scratch = G.new(nb // 4) if use_scratch else None
            L.call("ttk_conv_bwd_weight", p(g), p(y), p(d["bn"]), p(d["a"]), p(d["a_bound"]), p(dw), p(scratch), *geo)
            G.check("conv_bwd_weight " + form)
            if use_scratch:
                assert bool(torch.isfinite(scratch).all()), "a slice tile of the scratch was not written"
            runs.append(dw)
        if use_scratch:
            assert torch.equal(_bits(runs[0]), _bits(runs[1])), form  # the slice-wise form is bitwise reproducible
        for dw in runs:
            _judge("conv_bwd_weight_" + form, case, ref, R.wgrad_from_torch(c, dw.cpu().numpy()))


# ---- the non-GEMM neighbours off the square path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(2, 20, 33), (1, 33, 18), (1, 7, 7)])
def test_stem7_rows(B, H, W):
    L, p = _lib()
    c = R.stem_case(B, H, W)
    case = (B, H, W)
    d_x, d_w, d_piv, d_g, d_y, d_bn = _t(c.x), _t(c.w), _t(c.piv), _t(c.g), _t(c.y32), _t(c.bn)
    rows = L.partial_rows_elementwise(c.M * 16)
    runs = []
    for _ in range(2):
        G = Guard()
        y, part = G.new(c.M, 64), G.new(rows, 2, 64)
        L.call("ttk_stem7_fwd", p(d_x), p(d_w), p(y), p(part), p(d_piv), B, H, W)
        G.check("stem7_fwd")
        runs.append((y, part))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
    _judge("stem7_fwd", case, c.fwd, runs[0][0].cpu().numpy())
    _check_forward_sums(runs[0][1], runs[0][0].cpu().numpy(), c.fwd, c.piv)
    nb = L.cdll.ttk_stem7_wgrad_partial_bytes(B, H, W)
    assert nb > 0
    for form in ("atomic", "scratch"):
        runs = []
        for _ in range(2):
            G = Guard()
            dw = G.new(64, 49)  # overwritten
            scratch = G.new(nb // 4) if form == "scratch" else None
            L.call("ttk_stem7_bwd_weight", p(d_g), p(d_y), p(d_bn), p(d_x), p(dw), p(scratch), B, H, W)
            G.check("stem7_bwd_weight " + form)
            runs.append(dw)
            _judge("stem7_bwd_weight_" + form, case, c.wgrad, dw.cpu().numpy())
        if form == "scratch":
            assert torch.equal(_bits(runs[0]), _bits(runs[1]))


def _bn_pre(bn, y):
    return bn[R.BN_SCALE] * (y - bn[R.BN_MEAN]) + bn[R.BN_BETA]


@pytest.mark.parametrize("B,H,W,C", [(2, 6, 9, 64), (1, 2, 2, 32)])
def test_maxpool_rows(B, H, W, C):
    """as tests/test_resnet_kernels_gpu.py::test_maxpool, element by element at the same tolerances, H != W and a single window"""
    L, p = _lib()
    rng = np.random.default_rng(1009 * B + 101 * H + 7 * W + C)
    y = rng.normal(0, 1, (B, H, W, C)).astype(np.float32)
    bn = R.bn_block(C, rng)
    s64 = torch.from_numpy(_bn_pre(bn, y).astype(np.float32)).double().permute(0, 3, 1, 2).requires_grad_(True)
    a64 = F.max_pool2d(torch.relu(s64), 3, 2, 1)
    Ho, Wo = a64.shape[-2:]
    assert (Ho, Wo) == R.out_hw(H, W, 3, 2)
    ga, gb = rng.normal(0, 1, (B, Ho, Wo, C)).astype(np.float32), rng.normal(0, 1, (B, Ho, Wo, C)).astype(np.float32)
    (gs_ref,) = torch.autograd.grad(a64, s64, torch.from_numpy(ga + gb).double().permute(0, 3, 1, 2))
    gs_ref = gs_ref.permute(0, 2, 3, 1).numpy()
    rows = L.partial_rows_elementwise(B * H * W * (C // 4))
    d_y, d_ga, d_gb = _t(y), _t(ga), _t(gb)
    runs = []
    for _ in range(2):
        G = Guard()
        d_bn = _t(bn)
        a, idx = G.new(B, Ho, Wo, C), G.new(B, Ho, Wo, C, dtype=torch.uint8, fill=0xff)
        g, part = G.new(B, H, W, C), G.new(rows, 2, C)
        L.call("ttk_maxpool3x3s2_fwd", p(d_y), p(d_bn), p(a), p(idx), B, H, W, C)
        L.call("ttk_maxpool3x3s2_bwd", p(d_ga), p(d_gb), p(idx), p(d_y), p(d_bn), p(g), p(part), B, H, W, C)
        G.check("maxpool3x3s2")
        runs.append((a, idx, g, part))
        assert float(d_bn[R.BN_AUX, R.AUX_ACT_BOUND]) == float(a.max())
    for x, x2 in zip(*runs):
        assert torch.equal(x.view(torch.uint8), x2.view(torch.uint8))
    a, idx, g, part = runs[0]
    assert int(idx.max()) < 9
    np.testing.assert_allclose(a.cpu().numpy(), a64.detach().permute(0, 2, 3, 1).numpy(), rtol=1e-6, atol=1e-6)
    gv = g.cpu().numpy()
    np.testing.assert_allclose(gv, gs_ref, rtol=1e-5, atol=1e-6)
    ps = part.cpu().numpy().astype(np.float64)
    assert np.isfinite(ps).all()
    v, yc = gv.reshape(-1, C).astype(np.float64), (y - bn[R.BN_MEAN]).reshape(-1, C).astype(np.float64)
    np.testing.assert_allclose(ps[:, 0].sum(0), v.sum(0), rtol=0, atol=3e-5 * np.abs(v).sum(0).max() + 1e-12)
    np.testing.assert_allclose(ps[:, 1].sum(0), (v * yc).sum(0), rtol=0, atol=3e-5 * np.abs(v * yc).sum(0).max() + 1e-12)


def test_maxpool_refuses_a_single_row():
    """H = 1 (or W = 1) is outside what the pooling pair was built for (include/ttk.h): refused, nothing written"""
    L, p = _lib()
    B, H, W, C = 1, 1, 5, 32
    rng = np.random.default_rng(3)
    d_y, d_bn = _t(rng.normal(0, 1, (B, H, W, C)).astype(np.float32)), _t(R.bn_block(C, rng))
    G = Guard()
    a, idx, g = G.new(B, 1, 3, C), G.new(B, 1, 3, C, dtype=torch.uint8, fill=0xff), G.new(B, H, W, C)
    ga = torch.ones(B, 1, 3, C, device="cuda")
    with pytest.raises(RuntimeError, match="maxpool3x3s2_fwd: unsupported shape"):
        L.call("ttk_maxpool3x3s2_fwd", p(d_y), p(d_bn), p(a), p(idx), B, H, W, C)
    with pytest.raises(RuntimeError, match="maxpool3x3s2_bwd: unsupported shape"):
        L.call("ttk_maxpool3x3s2_bwd", p(ga), None, p(idx), p(d_y), p(d_bn), p(g), None, B, H, W, C)
    G.check("refused maxpool3x3s2")
    assert bool(a.isnan().all()) and bool(g.isnan().all()) and bool((idx == 0xff).all())


@pytest.mark.parametrize("B,H,W,C,stride", [(1, 1, 4, 32, 2), (2, 2, 7, 32, 2)])
def test_blur3x3_rows(B, H, W, C, stride):
    L, p = _lib()
    rng = np.random.default_rng(1009 * B + 101 * H + 7 * W + C)
    Ho, Wo = R.out_hw(H, W, 3, stride)
    a = rng.normal(0, 1, (B * H * W, C)).astype(np.float32)
    ga, gb = rng.normal(0, 1, (B * Ho * Wo, C)).astype(np.float32), rng.normal(0, 1, (B * Ho * Wo, C)).astype(np.float32)
    # the reference's own cross-check against torch (float64 depthwise convolution and its autograd)
    kern = torch.from_numpy(R.BLUR_TAPS.reshape(1, 1, 3, 3)).repeat(C, 1, 1, 1)
    a64 = torch.from_numpy(a).double().reshape(B, H, W, C).permute(0, 3, 1, 2).requires_grad_(True)
    t64 = F.conv2d(a64, kern, None, stride=stride, padding=1, groups=C)
    (gin64,) = torch.autograd.grad(t64, a64, torch.from_numpy(ga.astype(np.float64) + gb).reshape(B, Ho, Wo, C).permute(0, 3, 1, 2))
    fwd = R.BlurProduct(a, a.astype(np.float64), np.abs(a).astype(np.float64), R.gather_index(B, H, W, Ho, Wo, 3, stride, False))
    idx_t = R.gather_index(B, Ho, Wo, H, W, 3, stride, True)
    both = R.BlurProduct(ga + gb, ga.astype(np.float64) + gb, np.abs(ga).astype(np.float64) + np.abs(gb), idx_t)
    one = R.BlurProduct(ga, ga.astype(np.float64), np.abs(ga).astype(np.float64), idx_t)
    assert np.abs(fwd.ref - t64.detach().permute(0, 2, 3, 1).reshape(-1, C).numpy()).max() <= 1e-12
    assert np.abs(both.ref - gin64.permute(0, 2, 3, 1).reshape(-1, C).numpy()).max() <= 1e-12
    d_a, d_ga, d_gb = _t(a), _t(ga), _t(gb)
    case = (B, H, W, C, stride)
    runs = []
    for _ in range(2):
        G = Guard()
        t, g2, g1 = G.new(B * Ho * Wo, C), G.new(B * H * W, C), G.new(B * H * W, C)
        L.call("ttk_blur3x3_fwd", p(d_a), p(t), B, H, W, C, stride)
        L.call("ttk_blur3x3_bwd", p(d_ga), p(d_gb), p(g2), B, H, W, C, stride)
        L.call("ttk_blur3x3_bwd", p(d_ga), None, p(g1), B, H, W, C, stride)
        G.check("blur3x3")
        runs.append((t, g2, g1))
    for x, x2 in zip(*runs):
        assert torch.equal(_bits(x), _bits(x2))
    t, g2, g1 = runs[0]
    _judge("blur3x3_fwd", case, fwd, t.cpu().numpy())
    _judge("blur3x3_bwd", case, both, g2.cpu().numpy())
    _judge("blur3x3_bwd_one", case, one, g1.cpu().numpy())
