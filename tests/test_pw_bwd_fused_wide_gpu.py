"""ttk_pwconv1x1_bwd_fused on the layers with 256 output channels (csrc/pw_bwd_fused.hip, pw_bwd_fused16w_k): weight and data
gradient of a pointwise convolution from one read of g, y and ydw, against float64 numpy and against the two kernels it replaces.

Set up as test_fused_bwd_matches_fp64_and_the_two_kernels of test_pwconv_gpu.py: the same float64 reference, prepared weight block,
1.7x-loose operand bounds and `safe` mask.  The bound of the data gradient and of dW is max(3e-6, 1.5 * err2): 3e-6 is what that
test holds the fp16-split fused kernels to, err2 is the error of ttk_pwconv1x1_bwd_data + ttk_pwconv1x1_bwd_weight on the same inputs
against the same reference, and 1.5 covers another summation order of the same arithmetic (two fp16 pieces, three products, fp32
accumulation)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BN_SCALE, BN_BETA, BN_MEAN, BN_RSTD, BN_GA, BN_GB, BN_GMEAN, BN_AUX = range(8)
AUX_ACT_BOUND, AUX_DY_BOUND, AUX_GMAX = range(3)

# shapes that ship a fused form (the record profiles/pw_bwd_fused_wide.txt has the measurements behind the list)
SHIPPED = [(128, 256), (256, 256)]
# M: less than one 32-row stage | a few workgroups and a ragged last stage | more tiles than the persistent grid (at most 256 walkers):
# every workgroup walks several stages, both LDS buffers are reused
MS = [20, 32 * 8 + 31, 32 * 600 + 9]


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


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@functools.lru_cache(maxsize=None)
def _case(M, Cin, Cout):
    """Inputs, the float64 reference and the results of the two stand-alone kernels: computed once per shape, read-only afterwards."""
    import trackertraincode._hip as Hh
    L, p = Hh.lib(), Hh.ptr
    rng = np.random.default_rng(M + Cin)
    g = (rng.normal(0, 1, (M, Cout)) * 1e-2).astype(np.float32)
    y = rng.normal(0, 1, (M, Cout)).astype(np.float32)
    ydw = rng.normal(0, 1, (M, Cin)).astype(np.float32)
    w = (rng.normal(0, 1, (Cout, Cin)) * np.sqrt(2.0 / Cout)).astype(np.float32)
    bn_pw, bn_dw = _bn_block(Cout, rng), _bn_block(Cin, rng)
    dy = bn_pw[BN_GA].astype(np.float64) * (g - bn_pw[BN_GMEAN]) + bn_pw[BN_GB].astype(np.float64) * (y - bn_pw[BN_MEAN])
    yc = ydw.astype(np.float64) - bn_dw[BN_MEAN]
    pre = bn_dw[BN_SCALE] * yc + bn_dw[BN_BETA]
    c = dict(yc=yc, pre=pre, gdw_ref=(dy @ w.astype(np.float64)) * (pre > 0), dw_ref=dy.T @ np.maximum(pre, 0),
             safe=np.abs(pre) > 1e-4)  # a pre-activation within rounding of zero may fall on either side of the ReLU
    dev = "cuda"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c["g"], c["y"], c["ydw"], c["w"], c["bn_pw"], c["bn_dw"] = Hh.to_blocks(t(g)), Hh.to_blocks(t(y)), Hh.to_blocks(t(ydw)), t(w), t(bn_pw), t(bn_dw)
    c["prep"] = torch.empty(L.pwconv_prepared_bytes(Cin, Cout), dtype=torch.uint8, device=dev)
    L.pwconv_prepare_weights([c["w"].view(Cout, Cin, 1, 1)], [c["prep"]])
    c["bn_pw"][BN_AUX, AUX_DY_BOUND] = 1.7 * float(np.abs(dy).max())  # 1.7x loose, as the step's bounds are
    c["bn_dw"][BN_AUX, AUX_ACT_BOUND] = 1.7 * float(np.maximum(pre, 0).max())
    # the two kernels the fused one replaces, on the same inputs: their error against the same reference is the yardstick
    g_dw2 = torch.empty(M, Cin, device=dev)
    part2 = torch.empty(L.partial_rows_gemm(M, Cout, Cin, True), 2, Cin, device=dev)
    dw2 = torch.zeros(Cout, Cin, device=dev)
    wt = c["w"].t().contiguous()
    wq2 = torch.empty(L.pwconv_prepared_bytes(Cin, Cout), dtype=torch.uint8, device=dev)
    L.call("ttk_pwconv1x1_bwd_data", p(c["g"]), p(c["y"]), p(c["bn_pw"]), p(wt), p(c["ydw"]), p(c["bn_dw"]), p(g_dw2), p(part2), M, Cin, Cout, p(wq2), 0)
    L.call("ttk_pwconv1x1_bwd_weight", p(c["g"]), p(c["y"]), p(c["bn_pw"]), p(c["ydw"]), p(c["bn_dw"]), p(dw2), None, M, Cin, Cout, 0)
    torch.cuda.synchronize()
    c["err2_gdw"] = _rel(Hh.from_blocks(g_dw2).cpu().numpy() * c["safe"], c["gdw_ref"] * c["safe"])
    c["err2_dw"] = _rel(dw2.cpu().numpy(), c["dw_ref"])
    return c


def _run(c, M, Cin, Cout, scratch):
    import trackertraincode._hip as Hh
    L, p = Hh.lib(), Hh.ptr
    rows = L.cdll.ttk_pwconv1x1_bwd_fused_rows(M, Cin, Cout)
    assert rows > 0
    g_dw = torch.full((M, Cin), float("nan"), device="cuda")
    part = torch.full((rows, 2, Cin), float("nan"), device="cuda")
    dw = torch.zeros(Cout, Cin, device="cuda")
    L.call("ttk_pwconv1x1_bwd_fused", p(c["g"]), p(c["y"]), p(c["bn_pw"]), p(c["w"]), p(c["prep"]), p(c["ydw"]), p(c["bn_dw"]), p(g_dw), p(dw),
           p(scratch), p(part), M, Cin, Cout)
    torch.cuda.synchronize()
    return g_dw, dw, part


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("Cin,Cout", SHIPPED)
def test_wide_fused_bwd_matches_fp64_and_the_two_kernels(M, Cin, Cout):
    """Data gradient, dW and the BatchNorm-backward partial rows; rows past M contribute nothing; every element of g_dw is written."""
    import trackertraincode._hip as Hh
    c = _case(M, Cin, Cout)
    g_dw, dw, part = _run(c, M, Cin, Cout, None)
    out = Hh.from_blocks(g_dw).cpu().numpy()
    assert np.isfinite(out).all()  # the NaN pre-fill is overwritten everywhere
    e_gdw, e_dw = _rel(out * c["safe"], c["gdw_ref"] * c["safe"]), _rel(dw.cpu().numpy(), c["dw_ref"])
    print(f"M={M} {Cin}->{Cout}: g_dw fused {e_gdw:.3e} pair {c['err2_gdw']:.3e} | dW fused {e_dw:.3e} pair {c['err2_dw']:.3e}")
    assert e_gdw <= max(3e-6, 1.5 * c["err2_gdw"]), (e_gdw, c["err2_gdw"])
    assert e_dw <= max(3e-6, 1.5 * c["err2_dw"]), (e_dw, c["err2_dw"])
    ps = part.cpu().numpy().astype(np.float64)
    assert np.isfinite(ps).all()
    o64 = out.astype(np.float64)
    np.testing.assert_allclose(ps[:, 0].sum(0), o64.sum(0), rtol=0, atol=3e-5 * np.abs(o64).sum(0).max())
    np.testing.assert_allclose(ps[:, 1].sum(0), (o64 * c["yc"]).sum(0), rtol=0, atol=3e-5 * np.abs(o64 * c["yc"]).sum(0).max())


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("Cin,Cout", SHIPPED)
def test_wide_fused_bwd_deterministic_form(M, Cin, Cout):
    """With the scratch buffer the weight gradient is folded from slice tiles in a fixed order: two calls agree bit for bit."""
    import trackertraincode._hip as Hh
    L = Hh.lib()
    c = _case(M, Cin, Cout)
    nb = L.cdll.ttk_pwconv1x1_bwd_fused_partial_bytes(M, Cin, Cout)
    assert nb == L.cdll.ttk_pwconv1x1_bwd_fused_rows(M, Cin, Cout) * Cin * Cout * 4
    scratch = torch.full((nb // 4,), float("nan"), device="cuda")
    res = [_run(c, M, Cin, Cout, scratch) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))
    e_dw = _rel(res[0][1].cpu().numpy(), c["dw_ref"])
    print(f"M={M} {Cin}->{Cout}: dW folded {e_dw:.3e} pair {c['err2_dw']:.3e}")
    assert e_dw <= max(3e-6, 1.5 * c["err2_dw"]), (e_dw, c["err2_dw"])


def test_fused_rows_exactly_for_the_shipped_shapes():
    import trackertraincode._hip as Hh
    L = Hh.lib()
    M = 512 * 17 * 17
    for cin, cout in [(128, 256), (256, 256), (256, 512), (512, 512), (512, 1024), (1024, 1024), (256, 128), (512, 256)]:
        rows = L.cdll.ttk_pwconv1x1_bwd_fused_rows(M, cin, cout)
        assert (rows > 0) == ((cin, cout) in SHIPPED), (cin, cout, rows)
        assert (L.cdll.ttk_pwconv1x1_bwd_fused_partial_bytes(M, cin, cout) > 0) == ((cin, cout) in SHIPPED)
    for cin, cout in SHIPPED:
        assert 0 < L.cdll.ttk_pwconv1x1_bwd_fused_rows(M, cin, cout) <= 256  # the persistent grid
        assert L.cdll.ttk_pwconv1x1_bwd_fused_rows(20, cin, cout) == 1
