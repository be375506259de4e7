"""The any-channel-count kernel family (ttk_anyc_*, csrc/anyc_*.hip; include/ttk.h) entry point by entry point against float64, with the
criteria of the tuned siblings' tests (tests/test_pwconv_gpu.py, tests/test_dwconv_gpu.py) - channel counts that are multiples of 8 with a
narrower last channel block, ragged pixel counts - and bitwise repeatability of every weight gradient and partial-sum output (the family
has no float atomics)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BN_SCALE, BN_BETA, BN_MEAN, BN_RSTD, BN_GA, BN_GB, BN_GMEAN, BN_AUX = range(8)
AUX_ACT_BOUND, AUX_DY_BOUND, AUX_GMAX = range(3)


def _bn_block(C, rng):
    bn = np.zeros((8, C), np.float32)
    bn[BN_SCALE] = rng.uniform(0.5, 1.5, C)
    bn[BN_BETA] = rng.normal(0, 0.2, C)
    bn[BN_MEAN] = rng.normal(0, 0.3, C)
    bn[BN_RSTD] = rng.uniform(0.5, 2.0, C)
    bn[BN_GA] = rng.uniform(0.5, 1.5, C)
    bn[BN_GB] = rng.normal(0, 0.2, C)
    bn[BN_GMEAN] = rng.normal(0, 0.05, C)
    return bn


def _chain32(a, b_t):
    """a[M,K] @ b_t[K,N] accumulated k by k in float32: the accuracy class of a GEMM that keeps ONE fp32 accumulator per output."""
    acc = np.zeros((a.shape[0], b_t.shape[1]), np.float32)
    for k in range(a.shape[1]):
        acc += a[:, k:k + 1] * b_t[k:k + 1, :]
    return acc


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# (M, Cin, Cout): ragged in M, a narrower last channel block on either side
PW_SHAPES = [(1234, 8, 16), (140001, 16, 32), (99990, 24, 48), (33, 48, 96), (20736, 96, 96), (4100, 192, 384),
             (648, 384, 384), (300, 768, 768), (648, 1536, 1536), (128, 1024, 2048), (777, 48, 24)]


@pytest.mark.parametrize("M,Cin,Cout", PW_SHAPES)
def test_anyc_pw_fwd_bwd_data_bwd_weight(M, Cin, Cout):
    """Body of tests/test_pwconv_gpu.py::test_pwconv_fwd_bwd_data_bwd_weight on the ttk_anyc_pw_* entry points."""
    import trackertraincode._hip as H
    L, p = H.lib(), H.ptr
    rng = np.random.default_rng(M + Cin + Cout)
    ydw = rng.normal(0, 1, (M, Cin)).astype(np.float32)
    w = (rng.normal(0, 1, (Cout, Cin)) * np.sqrt(2.0 / Cout)).astype(np.float32)
    bn_dw, bn_pw = _bn_block(Cin, rng), _bn_block(Cout, rng)
    dev = "cuda"
    t = lambda a: torch.from_numpy(a).to(dev)
    rows = L.partial_rows_gemm(M)

    # ---- forward
    a32 = np.maximum(bn_dw[BN_SCALE] * (ydw - bn_dw[BN_MEAN]) + bn_dw[BN_BETA], 0).astype(np.float32)
    y64 = a32.astype(np.float64) @ w.astype(np.float64).T
    y32 = _chain32(a32, np.ascontiguousarray(w.T))
    d_ydw, d_w, d_bn = H.to_blocks_any(t(ydw)), t(w), t(bn_dw)
    piv = rng.normal(0, 0.5, Cout).astype(np.float32)
    d_piv = t(piv)
    fw = []
    for _ in range(2):
        y = torch.full((M, Cout), float("nan"), device=dev)
        part = torch.full((rows, 2, Cout), float("nan"), device=dev)
        L.call("ttk_anyc_pw_fwd", p(d_ydw), p(d_bn), p(d_w), p(y), p(part), p(d_piv), M, Cin, Cout)
        torch.cuda.synchronize()
        fw.append((y, part))
    assert torch.equal(fw[0][0], fw[1][0]) and torch.equal(fw[0][1], fw[1][1])
    e_hip, e_f32 = _rel(H.from_blocks_any(y).cpu().numpy(), y64), _rel(y32, y64)
    print(f"fwd   M={M} K={Cin} N={Cout}: hip {e_hip:.2e}  fp32 chain {e_f32:.2e}")
    assert e_hip <= 1.5 * e_f32 + 1e-7, (e_hip, e_f32)
    ps = part.cpu().numpy().astype(np.float64)
    assert np.isfinite(ps).all()
    ys = y64 - piv.astype(np.float64)
    np.testing.assert_allclose(ps[:, 0].sum(0), ys.sum(0), rtol=0, atol=2e-5 * np.abs(ys).sum(0).max())
    np.testing.assert_allclose(ps[:, 1].sum(0), (ys ** 2).sum(0), rtol=2e-5)

    # ---- data gradient
    g = rng.normal(0, 1, (M, Cout)).astype(np.float32)
    yv = H.from_blocks_any(y).cpu().numpy()
    dy32 = (bn_pw[BN_GA] * (g - bn_pw[BN_GMEAN]) + bn_pw[BN_GB] * (yv - bn_pw[BN_MEAN])).astype(np.float32)
    pre = bn_dw[BN_SCALE] * (ydw - bn_dw[BN_MEAN]) + bn_dw[BN_BETA]
    mask = pre > 0
    safe = np.abs(pre) > 1e-4  # entries whose mask could flip with rounding are left out of the comparison
    excluded = 1.0 - safe.mean()
    print(f"dgrad excluded share {excluded:.2e}")
    assert excluded <= 1e-3, excluded  # (density of pre <= 0.8 with ydw ~ N(0,1), scale >= 0.5: at most 1.6e-4 expected)
    gd64 = (dy32.astype(np.float64) @ w.astype(np.float64)) * mask
    gd32 = _chain32(dy32, w) * mask
    d_g, d_bnpw = H.to_blocks_any(t(g)), t(bn_pw)
    bw = []
    for _ in range(2):
        g_dw = torch.full((M, Cin), float("nan"), device=dev)
        part2 = torch.full((rows, 2, Cin), float("nan"), device=dev)
        d_bn2 = d_bn.clone()
        L.call("ttk_anyc_pw_bwd_data", p(d_g), p(y), p(d_bnpw), p(d_w), p(d_ydw), p(d_bn2), p(g_dw), p(part2), M, Cin, Cout)
        torch.cuda.synchronize()
        bw.append((g_dw, part2, d_bn2))
    assert all(torch.equal(a, b) for a, b in zip(*bw))
    out = H.from_blocks_any(g_dw).cpu().numpy()
    assert np.isfinite(out).all()
    e_hip, e_f32 = _rel(out * safe, gd64 * safe), _rel(gd32 * safe, gd64 * safe)
    print(f"dgrad M={M} K={Cout} N={Cin}: hip {e_hip:.2e}  fp32 chain {e_f32:.2e}")
    assert e_hip <= 1.5 * e_f32 + 1e-7, (e_hip, e_f32)
    ps = part2.cpu().numpy().astype(np.float64)
    assert np.isfinite(ps).all()
    o64 = out.astype(np.float64)
    np.testing.assert_allclose(ps[:, 0].sum(0), o64.sum(0), rtol=0, atol=2e-5 * np.abs(o64).sum(0).max())
    s2 = (o64 * (ydw.astype(np.float64) - bn_dw[BN_MEAN])).sum(0)
    np.testing.assert_allclose(ps[:, 1].sum(0), s2, rtol=0, atol=2e-5 * np.abs(o64 * (ydw - bn_dw[BN_MEAN])).sum(0).max())
    # TTK_AUX_GMAX of the producer's block: max |g_dw| (a maximum is exact), nothing else of the block touched
    got_bn = d_bn2.cpu().numpy()
    assert got_bn[BN_AUX, AUX_GMAX] == np.abs(out).max()
    got_bn[BN_AUX, AUX_GMAX] = 0
    assert np.array_equal(got_bn, bn_dw)

    # ---- weight gradient (slice rows + fixed-order fold): overwrite and accumulate forms, bitwise repeatable
    dw64 = dy32.astype(np.float64).T @ a32.astype(np.float64)
    dw32 = _chain32(np.ascontiguousarray(dy32.T), a32)
    nbytes = L.anyc_wgrad_scratch_bytes("pw", M, Cin, Cout)
    assert nbytes > 0
    runs = []
    for _ in range(2):
        scratch = torch.full((nbytes // 4,), float("nan"), device=dev)
        dW = torch.full((Cout, Cin), float("nan"), device=dev)
        L.call("ttk_anyc_pw_bwd_weight", p(d_g), p(y), p(d_bnpw), p(d_ydw), p(d_bn), p(dW), 0, p(scratch), M, Cin, Cout)
        torch.cuda.synchronize()
        runs.append(dW)
    assert torch.equal(runs[0], runs[1])
    e_hip, e_f32 = _rel(runs[0].cpu().numpy(), dw64), _rel(dw32, dw64)
    print(f"wgrad M={M} Cout={Cout} Cin={Cin}: hip {e_hip:.2e}  fp32 chain {e_f32:.2e}")
    assert e_hip <= 1.5 * e_f32 + 1e-7, (e_hip, e_f32)
    acc = torch.ones(Cout, Cin, device=dev)
    L.call("ttk_anyc_pw_bwd_weight", p(d_g), p(y), p(d_bnpw), p(d_ydw), p(d_bn), p(acc), 1, p(scratch), M, Cin, Cout)
    torch.cuda.synchronize()
    # (the fold starts from the buffer's value: same sum, another rounding order than 1 + folded sum)
    assert torch.allclose(acc, 1.0 + runs[0], rtol=1e-5, atol=1e-5 * float(runs[0].abs().max()))


SCALE, BETA, MEAN, RSTD, GA, GB, GMEAN = range(7)


def _bn(C, g):
    bn = torch.zeros(8, C, dtype=torch.float64)
    bn[SCALE] = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    bn[BETA] = torch.randn(C, generator=g, dtype=torch.float64) * 0.2
    bn[MEAN] = torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    bn[RSTD] = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    bn[GA] = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    bn[GB] = torch.randn(C, generator=g, dtype=torch.float64) * 0.2
    bn[GMEAN] = torch.randn(C, generator=g, dtype=torch.float64) * 0.05
    return bn


def _nchw(t):  # [B,H,W,C] -> [B,C,H,W]
    return t.permute(0, 3, 1, 2)


# (B, H = W, C, stride, skip): every C in {8, 16, 24, 48, 96, 192, 768, 2048} at both strides, the network's spatial sizes 65, 33, 17, 9, 5,
# B in {3, 64}; each channel count at the sizes it meets in a width-scaled network (and one size up)
DW_SHAPES = [(3, 65, 8, 1, True), (64, 65, 8, 2, False), (64, 65, 16, 1, True), (3, 65, 16, 2, False),
             (3, 65, 24, 1, True), (64, 33, 24, 2, False), (64, 33, 48, 1, True), (3, 65, 48, 2, False),
             (3, 33, 96, 1, True), (64, 33, 96, 2, False), (64, 17, 192, 1, True), (3, 33, 192, 2, False),
             (3, 9, 768, 1, True), (64, 9, 768, 2, False), (64, 5, 768, 1, False), (3, 17, 768, 2, False),
             (3, 5, 2048, 1, True), (64, 5, 2048, 2, False), (3, 9, 2048, 2, False), (3, 17, 96, 1, False)]


@pytest.mark.parametrize("B,H,C,stride,skip", DW_SHAPES)
def test_anyc_dw_fwd_and_bwd_against_float64(B, H, C, stride, skip):
    """Body of tests/test_dwconv_gpu.py::test_dwconv_fwd_and_bwd_against_float64 on ttk_anyc_dw_fwd / ttk_anyc_dw_bwd_data: skip input,
    materialised a_out, residual gradient, fused weight gradient, TTK_AUX_GMAX."""
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    W = H
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W + C + stride)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    yprev, skp = rnd(B, H, W, C), (rnd(B, H, W, C).abs() if skip else None)
    w = rnd(C, 1, 3, 3) * 0.3
    bn_prev, bn_dw = _bn(C, g), _bn(C, g)
    f32 = lambda t: None if t is None else t.to(torch.float32).cuda().contiguous()
    yprev, w, bn_prev, bn_dw = (t.to(torch.float32).double() for t in (yprev, w, bn_prev, bn_dw))
    skp = None if skp is None else skp.to(torch.float32).double()

    # ---------------- forward
    pre = bn_prev[SCALE] * (yprev - bn_prev[MEAN]) + bn_prev[BETA] + (skp if skip else 0.0)
    a_in = pre.clamp_min(0.0)
    y_ref = F.conv2d(_nchw(a_in), w, stride=stride, padding=1, groups=C).permute(0, 2, 3, 1)
    blk = lambda t: None if t is None else hip.to_blocks_any(f32(t))
    unblk = lambda t: hip.from_blocks_any(t).cpu().double()
    d_yprev, d_skip, d_w, d_bnp = blk(yprev), blk(skp), f32(w), f32(bn_prev)
    want_a = skip and stride == 1
    rows = L.anyc_partial_rows(B * Ho * Wo)
    piv = (torch.randn(C, generator=torch.Generator().manual_seed(C)) * 0.5).float()
    d_piv = piv.cuda()
    fw = []
    for _ in range(2):
        a_out = torch.full((B, H, W, C), float("nan"), device="cuda") if want_a else None
        y = torch.full((B, Ho, Wo, C), float("nan"), device="cuda")
        part = torch.full((rows, 2, C), float("nan"), device="cuda")
        L.call("ttk_anyc_dw_fwd", p(d_yprev), p(d_bnp), p(d_skip), p(a_out), p(d_w), p(y), p(part), p(d_piv), B, H, W, C, stride)
        torch.cuda.synchronize()
        fw.append((y, part))
    assert torch.equal(fw[0][0], fw[1][0]) and torch.equal(fw[0][1], fw[1][1])
    assert torch.isfinite(y).all() and torch.isfinite(part).all()
    scale = y_ref.abs().max().item()
    assert (unblk(y) - y_ref).abs().max().item() <= 3e-6 * scale
    if want_a:
        assert (unblk(a_out) - a_in).abs().max().item() <= 1e-6 * max(a_in.abs().max().item(), 1.0)
    ps = part.cpu().double().sum(0)
    ys = y_ref - piv.double()
    assert torch.allclose(ps[0], ys.sum((0, 1, 2)), rtol=0, atol=2e-5 * ys.abs().sum((0, 1, 2)).max().item())
    assert torch.allclose(ps[1], (ys ** 2).sum((0, 1, 2)), rtol=2e-5, atol=1e-12)

    # ---------------- data gradient (+ fused weight gradient), block input recomputed and materialised
    g_dw, y_dw = rnd(B, Ho, Wo, C).to(torch.float32).double(), unblk(y)
    sg = rnd(B, H, W, C).to(torch.float32).double() if (skip and stride == 1) else None
    dy = bn_dw[GA] * (g_dw - bn_dw[GMEAN]) + bn_dw[GB] * (y_dw - bn_dw[MEAN])
    a_leaf = a_in.clone().requires_grad_(True)
    w_leaf = w.clone().requires_grad_(True)
    out = F.conv2d(_nchw(a_leaf), w_leaf, stride=stride, padding=1, groups=C)
    out.backward(_nchw(dy).contiguous())
    G = a_leaf.grad + (sg if sg is not None else 0.0)
    margin = pre.abs() > 1e-4  # entries whose relu mask could flip with rounding are left out
    gp_ref = G * (pre > 0)
    dw_ref = w_leaf.grad.reshape(C, 9)
    d_g, d_y, d_bnd, d_sg = blk(g_dw), y, f32(bn_dw), blk(sg)
    rows_b = L.anyc_partial_rows(B * H * W)
    nbytes = L.anyc_wgrad_scratch_bytes("dw", B, H, W, C)
    for materialised in ((False, True) if want_a else (False,)):
        det = []
        for _ in range(2):
            scratch = torch.full((nbytes // 4,), float("nan"), device="cuda")
            g_prev = torch.full((B, H, W, C), float("nan"), device="cuda")
            part_b = torch.full((rows_b, 2, C), float("nan"), device="cuda")
            dwg = torch.full((C, 9), float("nan"), device="cuda")
            bnp = d_bnp.clone()
            L.call("ttk_anyc_dw_bwd_data", p(d_g), p(d_y), p(d_bnd), p(d_w), p(d_sg), p(d_yprev), p(bnp), p(d_skip),
                   p(a_out) if materialised else None, p(g_prev), p(part_b), p(dwg), 0, p(scratch), B, H, W, C, stride)
            torch.cuda.synchronize()
            det.append((dwg, g_prev, part_b, bnp))
        assert all(torch.equal(a, b) for a, b in zip(*det))
        got = unblk(g_prev)
        assert torch.isfinite(got).all() and torch.isfinite(part_b).all()
        sc = gp_ref.abs().max().item()
        assert ((got - gp_ref) * margin).abs().max().item() <= 5e-6 * sc, (materialised,)
        assert (dwg.cpu().double() - dw_ref).abs().max().item() <= 3e-5 * dw_ref.abs().max().item()
        pb = part_b.cpu().double().sum(0)
        assert torch.allclose(pb[0], got.sum((0, 1, 2)), rtol=0, atol=3e-5 * got.abs().sum((0, 1, 2)).max().item())
        s2 = (got * (yprev - bn_prev[MEAN])).sum((0, 1, 2))
        assert torch.allclose(pb[1], s2, rtol=0, atol=3e-5 * (got * (yprev - bn_prev[MEAN])).abs().sum((0, 1, 2)).max().item())
        assert bnp[BN_AUX, AUX_GMAX].item() == g_prev.abs().max().item()  # TTK_AUX_GMAX raised to max |g_prev|
        # without the weight gradient (the blur step of a BlurPool block): the same data gradient
        gp2, pb2 = torch.empty_like(g_prev), torch.empty_like(part_b)
        L.call("ttk_anyc_dw_bwd_data", p(d_g), p(d_y), p(d_bnd), p(d_w), p(d_sg), p(d_yprev), p(d_bnp.clone()), p(d_skip),
               p(a_out) if materialised else None, p(gp2), p(pb2), None, 0, None, B, H, W, C, stride)
        torch.cuda.synchronize()
        assert torch.equal(gp2, g_prev) and torch.equal(pb2, part_b)


@pytest.mark.parametrize("Cout", [8, 16, 24, 48, 64])
@pytest.mark.parametrize("B,H,W", [(2, 129, 129), (3, 33, 33), (2, 40, 50), (5, 7, 9)])
def test_anyc_stem_fwd_and_weight_gradient_against_float64(B, H, W, Cout):
    """Body of tests/test_dwconv_gpu.py::test_stem_fwd_and_weight_gradient_against_float64 with a Cout argument."""
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    g = torch.Generator().manual_seed(B + H + W + Cout)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    x = (torch.rand(B, 1, H, W, generator=g) - 0.5).double()
    w = (torch.randn(Cout, 1, 5, 5, generator=g) * 0.2).float().double()
    x = x.float().double()
    y_ref = F.conv2d(x, w, stride=2, padding=2).permute(0, 2, 3, 1)
    d_x, d_w = x.float().cuda(), w.float().cuda()
    rows = L.anyc_partial_rows(B * Ho * Wo)
    piv = (torch.randn(Cout, generator=g) * 0.1).float()
    d_piv = piv.cuda()
    fw = []
    for _ in range(2):
        y = torch.full((B, Ho, Wo, Cout), float("nan"), device="cuda")
        part = torch.full((rows, 2, Cout), float("nan"), device="cuda")
        L.call("ttk_anyc_stem_fwd", p(d_x), p(d_w), p(y), p(part), p(d_piv), B, H, W, Cout)
        torch.cuda.synchronize()
        fw.append((y, part))
    assert torch.equal(fw[0][0], fw[1][0]) and torch.equal(fw[0][1], fw[1][1])
    yv = hip.from_blocks_any(y).cpu().double()
    assert (yv - y_ref).abs().max().item() <= 3e-6 * y_ref.abs().max().item()
    ps = part.cpu().double().sum(0)
    ys = y_ref - piv.double()
    assert torch.allclose(ps[0], ys.sum((0, 1, 2)), rtol=0, atol=2e-5 * ys.abs().sum((0, 1, 2)).max().item())
    assert torch.allclose(ps[1], (ys ** 2).sum((0, 1, 2)), rtol=2e-5)
    bn = _bn(Cout, g).float().double()
    gr = torch.randn(B, Ho, Wo, Cout, generator=g).float().double()
    dy = bn[GA] * (gr - bn[GMEAN]) + bn[GB] * (yv - bn[MEAN])
    wl = w.clone().requires_grad_(True)
    F.conv2d(x, wl, stride=2, padding=2).backward(_nchw(dy).contiguous())
    d_g, d_bn = hip.to_blocks_any(gr.float().cuda()), bn.float().cuda()
    ref = wl.grad.reshape(Cout, 25)
    det = []
    for _ in range(2):
        scratch = torch.full((L.anyc_wgrad_scratch_bytes("stem", B, H, W, Cout) // 4,), float("nan"), device="cuda")
        dwd = torch.full((Cout, 25), float("nan"), device="cuda")
        L.call("ttk_anyc_stem_bwd_weight", p(d_g), p(y), p(d_bn), p(d_x), p(dwd), 0, p(scratch), B, H, W, Cout)
        torch.cuda.synchronize()
        det.append(dwd)
    assert torch.equal(det[0], det[1])
    assert (det[0].cpu().double() - ref).abs().max().item() <= 3e-5 * ref.abs().max().item()


@pytest.mark.parametrize("C", [8, 48, 256, 768, 1536])
@pytest.mark.parametrize("B,HW,skip", [(3, 25, True), (64, 25, False), (5, 81, True)])
def test_anyc_pool_and_bn_act_against_float64(B, HW, C, skip):
    """ttk_anyc_avgpool_fwd / _bwd and ttk_anyc_bn_act against float64: features, masked gradient, partial sums, TTK_AUX_GMAX."""
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    g = torch.Generator().manual_seed(B + HW + C)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()
    y, sk, bn = rnd(B, HW, C), (rnd(B, HW, C).abs() if skip else None), _bn(C, g).float().double()
    pre = bn[SCALE] * (y - bn[MEAN]) + bn[BETA] + (sk if skip else 0.0)
    a = pre.clamp_min(0.0)
    d_y, d_sk, d_bn = hip.to_blocks_any(y.float().cuda()), (hip.to_blocks_any(sk.float().cuda()) if skip else None), bn.float().cuda()
    feat = torch.full((B, C), float("nan"), device="cuda")
    L.call("ttk_anyc_avgpool_fwd", p(d_y), p(d_bn), p(d_sk), p(feat), B, HW, C)
    act = torch.full((B, HW, C), float("nan"), device="cuda")
    L.call("ttk_anyc_bn_act", p(d_y), p(d_bn), p(d_sk), p(act), B * HW, C)
    torch.cuda.synchronize()
    assert (feat.cpu().double() - a.mean(1)).abs().max().item() <= 3e-6 * max(a.mean(1).abs().max().item(), 1.0)
    assert (act.cpu().double() - a).abs().max().item() <= 1e-6 * max(a.abs().max().item(), 1.0)  # plain channels-last rows
    gfeat = rnd(B, C)
    g_ref = (gfeat[:, None, :] / HW) * (pre > 0)
    margin = pre.abs() > 1e-4
    rows = L.anyc_partial_rows(B * HW)
    d_gf = gfeat.float().cuda()
    runs = []
    for _ in range(2):
        gout = torch.full((B, HW, C), float("nan"), device="cuda")
        part = torch.full((rows, 2, C), float("nan"), device="cuda")
        bnc = d_bn.clone()
        L.call("ttk_anyc_avgpool_bwd", p(d_gf), p(d_y), p(bnc), p(d_sk), p(gout), p(part), B, HW, C)
        torch.cuda.synchronize()
        runs.append((gout, part, bnc))
    assert all(torch.equal(u, v) for u, v in zip(*runs))
    got = hip.from_blocks_any(gout).cpu().double()
    assert ((got - g_ref) * margin).abs().max().item() <= 1e-6 * g_ref.abs().max().item()
    pb = part.cpu().double().sum(0)
    assert torch.allclose(pb[0], got.sum((0, 1)), rtol=0, atol=3e-5 * got.abs().sum((0, 1)).max().item())
    s2 = got * (y - bn[MEAN])
    assert torch.allclose(pb[1], s2.sum((0, 1)), rtol=0, atol=3e-5 * s2.abs().sum((0, 1)).max().item())
    assert bnc[BN_AUX, AUX_GMAX].item() == gout.abs().max().item()


def test_anyc_entry_points_reject_bad_arguments():
    """Channel counts outside the family's domain (multiples of 8 in 8..2048) and a_out at stride 2 are refused before any launch; the
    tuned entry points keep their own domain (48 channels: refused there, accepted here)."""
    import trackertraincode._hip as hip
    L, p = hip.lib(), hip.ptr
    t = torch.zeros(1 << 16, device="cuda")
    for C in (4, 12, 2056):
        with pytest.raises(RuntimeError, match="unsupported shape"):
            L.call("ttk_anyc_pw_fwd", p(t), p(t), p(t), p(t), p(t), None, 16, C, 16)
        with pytest.raises(RuntimeError, match="unsupported shape"):
            L.call("ttk_anyc_dw_fwd", p(t), p(t), None, None, p(t), p(t), p(t), None, 1, 5, 5, C, 1)
    with pytest.raises(RuntimeError, match="stride 1"):
        L.call("ttk_anyc_dw_fwd", p(t), p(t), None, p(t), p(t), p(t), p(t), None, 1, 5, 5, 16, 2)
    with pytest.raises(RuntimeError):
        L.call("ttk_pwconv1x1_fwd", p(t), p(t), p(t), p(t), p(t), None, 16, 48, 48, p(t), 0)
