"""tests/conv_ref.py on its own, without a GPU: the im2col reference against torch's float64 convolution and its autograd; the yardstick
(fp32 fma chain, three-product split model) inside the criterion that tests/test_conv_rows_gpu.py holds the kernels to; four mutations of
the numpy model - the errors that file exists to catch - each more than 10x outside it; the cap on undecided mask elements."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

_ids = lambda v: "x".join(map(str, v))
SENSITIVITY = 10.0  # every mutation must land this far outside what the criterion allows
WHOLE_TENSOR_TOL = 1.5e-6  # what tests/test_conv_gpu.py allows for |out - ref| / |ref| over the whole tensor


def _outside(p, x):
    """worst |x - f64| / allowed over the elements: > 1 fails the criterion"""
    allowed = p.allowed()
    err = np.abs(np.asarray(x, np.float64) - p.ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(allowed > 0, err / np.where(allowed > 0, allowed, 1.0), np.where(err == 0, 0.0, np.inf)).max())


def test_case_table_covers_what_it_claims():
    seen = set()
    for B, H, W, Cin, Cout, k, stride in R.CASES:
        Ho, Wo = R.out_hw(H, W, k, stride)
        assert B * Ho * Wo <= 600 and B * H * W <= 600 and k * k * Cin * Cout <= 2.4e6
        for what, nout, m in (("fwd", Cout, B * Ho * Wo),) + ((("dgrad", Cin, B * H * W),) if Cin % 64 == 0 else ()):
            bm = 128 if nout % 128 else (256 if nout % 256 else 128)
            form = "128x64" if nout % 128 else ("256x128" if nout % 256 else "128x256")
            seen.add((what, form, "below" if m < bm else "exact" if m == bm else "plus1" if m == bm + 1 else "other"))
        ncols = k * k * Cin
        seen.add(("wgrad", "64x192" if Cout == 64 and ncols == 576 else "64x256" if Cout == 64 else "128x256"))
        if stride == 2:
            seen.add(("s2", k, H % 2, W % 2, H != W))
            seen.add(("s2small", k, H, W))
    for what in ("fwd", "dgrad"):
        for form in ("128x64", "256x128", "128x256"):
            for m in ("below", "exact", "plus1"):
                assert (what, form, m) in seen, (what, form, m)
    for form in ("64x192", "64x256", "128x256"):
        assert ("wgrad", form) in seen
    for k in (1, 3):
        for ph in (0, 1):
            for pw in (0, 1):
                assert ("s2", k, ph, pw, True) in seen
        for hw in ((1, 1), (1, 6), (6, 1), (2, 2), (2, 3)):
            assert ("s2small", k) + hw in seen
    assert {c[3] for c in R.CASES} >= {32, 64, 96, 128, 256, 512} and {c[4] for c in R.CASES} >= {64, 128, 192, 256, 512}
    assert len(set(R.CASES)) == len(R.CASES)
    B, H, W, Cin, Cout, k, stride = R.MULTI_SLICE_CASE
    M = B * H * W
    slices, rows = R.wgrad_slices(M, Cout, k * k * Cin)
    assert R.MULTI_SLICE_CASE in R.CASES and slices == R.MULTI_SLICE_COUNT and M % rows != 0  # ragged last slice
    assert R.wgrad_slices(M - 1, Cout, k * k * Cin)[0] == 1  # ... and no smaller M has two


@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_im2col_reference_equals_torch_float64(case):
    c = R.make_case(case)
    nchw = lambda x, h, w: torch.from_numpy(np.ascontiguousarray(x)).double().reshape(c.B, h, w, -1).permute(0, 3, 1, 2)
    a64 = nchw(c.a, c.H, c.W).requires_grad_(True)
    w64 = torch.from_numpy(c.w).double().requires_grad_(True)
    y64 = F.conv2d(a64, w64, stride=c.stride, padding=c.pad)
    assert tuple(y64.shape[-2:]) == (c.Ho, c.Wo)
    dy64, D = R.dy_terms(c)
    ga, gw = torch.autograd.grad(y64, (a64, w64), nchw(dy64, c.Ho, c.Wo))
    close = lambda x, ref: np.abs(x - ref).max() <= 1e-12 * np.abs(ref).max()
    assert close(c.y64, y64.detach().permute(0, 2, 3, 1).reshape(c.M, c.Cout).numpy())
    g_in = R.im2col(dy64, c.idx_t) @ c.Wb.astype(np.float64)
    assert close(g_in, ga.permute(0, 2, 3, 1).reshape(c.Min, c.Cin).numpy())
    dw = dy64.T @ c.A.astype(np.float64)
    assert close(dw, R.wgrad_from_torch(c, gw.numpy()))
    assert np.all(D >= np.abs(dy64)) and np.all(np.abs(c.dy32) <= c.dy_bound) and float(c.a.max()) <= c.a_bound
    # exact zeros are where the case says: the zero channels' weight-gradient columns, the odd pixels of a strided 1x1 data gradient
    s_w = (D.T @ np.abs(c.A).astype(np.float64)).reshape(c.Cout, c.T, c.Cin)
    assert np.all(s_w[:, :, c.zero_channels] == 0)
    if c.k == 1 and c.stride == 2:
        s_in = (R.im2col(D, c.idx_t) @ np.abs(c.Wb).astype(np.float64)).reshape(c.B, c.H, c.W, c.Cin)
        assert np.all(s_in[:, 1::2] == 0) and np.all(s_in[:, :, 1::2] == 0) and np.all(s_in[:, ::2, ::2] > 0)


@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_yardstick_satisfies_the_criterion_and_undecided_share_is_capped(case):
    prods = [("fwd", R.forward(case)), ("wgrad", R.wgrad(case))] + ([("dgrad", R.dgrad(case))] if R.has_dgrad(case) else [])
    for name, p in prods:
        assert np.isfinite(p.Y) and 0 < p.Y < 64 * R.U, (name, p.Y)  # an fp32 chain's class: a few ulp of the scale, at every K here
        for x in (p.chain, p.model):
            ratio, zeros_ok = p.ratio(x)
            assert zeros_ok and ratio <= 1.0 and _outside(p, x) <= 1.0, (name, ratio)
        print(f"YARDSTICK {name} {_ids(case)} chain {p.E_chain:.2e} model {p.E_model:.2e}")
    if R.has_dgrad(case):
        p = R.dgrad(case)
        assert p.share <= R.UNDECIDED_CAP, p.share
        # the reference's own masked value passes the masked rule; opening a closed element or closing an open one does not
        out = p.ref * p.open
        ratio, zeros_ok = R.masked_ratio(p, out)
        assert zeros_ok and ratio <= 0.0
        closed, opened = np.argwhere(~p.open & ~p.undecided), np.argwhere(p.open & ~p.undecided & (p.s > 0))
        if len(closed):
            bad = out.copy()
            bad[tuple(closed[0])] = 1e-30
            assert not R.masked_ratio(p, bad)[1]
        if len(opened):
            bad = out.copy()
            bad[tuple(opened[len(opened) // 2])] = 0.0
            assert R.masked_ratio(p, bad)[0] > R.MARGIN


# ---- sensitivity: what a whole-tensor norm lets through and the per-row criterion does not -----------------------------------------------
CASE_LOW_PIECE = (2, 12, 17, 32, 64, 3, 1)   # (a) forward, K = 288, M = 408
CASE_EVEN_H = (3, 8, 6, 64, 64, 3, 2)        # (b) even-H stride-2 data gradient
CASE_NON_SQUARE = (2, 7, 10, 64, 128, 3, 2)  # (c) H != W, forward gather and transposed gather
CASE_PADDED_DY = (2, 4, 16, 64, 64, 3, 1)    # (d) padded taps of the dy-forming operand


def _drop_low_piece(case):
    """(worst |x - f64| / allowed, whole-tensor figure) of the forward split model with the low fp16 piece of the activation operand
    lost over one k32 step (the first of the centre tap: never padded) of one row (an interior pixel of image 0)"""
    c, p = R.make_case(case), R.forward(case)
    row = (c.Ho // 2) * c.Wo + c.Wo // 2
    k0 = 4 * c.Cin
    bad = R.split_model(p.A32, p.B32, p.bound_a, p.bound_b, drop_low=(row, k0, k0 + 32))
    assert np.array_equal(np.delete(bad, row, 0), np.delete(p.model, row, 0))
    out, rel = _outside(p, bad), p.rel(bad)
    print(f"MUTATION a {_ids(case)}: outside {out:.1f}x  E {p.E(bad):.2e} (Y {p.Y:.2e})  whole-tensor {rel:.2e} (unmutated {p.rel(p.model):.2e})")
    return out, rel


def test_mutation_low_piece_of_one_k32_step_of_one_row():
    """(a) The row's own figure leaves the criterion by more than 10x - on the case named for it and on the first shape of
    tests/test_conv_gpu.py, (3, 33, 64, 64, 3, 1), M = 3267, where the whole-tensor figure that test asserts does not notice: a local
    error is diluted by the square root of its share of the elements, which is why tests/test_conv_rows_gpu.py judges row by row."""
    out, _ = _drop_low_piece(CASE_LOW_PIECE)
    assert out > SENSITIVITY
    out, rel = _drop_low_piece((3, 33, 33, 64, 64, 3, 1))
    assert out > SENSITIVITY
    assert rel < WHOLE_TENSOR_TOL


def test_mutation_even_side_reads_the_wrapped_pixel():
    """(b) The transposed gather without its upper-bound test: with H = 8 the tap kh = 0 of row gh = 7 has sh = 4 = Ho and reads the next
    image's row 0 (the last image: its own last row) instead of zero."""
    c, p = R.make_case(CASE_EVEN_H), R.dgrad(CASE_EVEN_H)
    idx = R.gather_index(c.B, c.Ho, c.Wo, c.H, c.W, c.k, c.stride, True, mutate="wrap")
    touched = (idx != c.idx_t).any(1).reshape(c.B, c.H, c.W)
    assert touched[:, c.H - 1].all() and not touched[:, :c.H - 1].any()  # the last grid row of every image, nothing else
    dy64, _ = R.dy_terms(c)
    bad = R.im2col(dy64, idx) @ c.Wb.astype(np.float64)
    out = _outside(p, bad)
    print(f"MUTATION b: outside {out:.1f}x  whole-tensor {p.rel(bad):.2e}")
    assert out > SENSITIVITY


def test_mutation_height_and_width_exchanged():
    """(c) Hs and Ws exchanged in the gather of a non-square case: forward (source 7 x 10) and transposed (source 4 x 5)."""
    c = R.make_case(CASE_NON_SQUARE)
    idx = R.gather_index(c.B, c.H, c.W, c.Ho, c.Wo, c.k, c.stride, False, mutate="swap")
    p = R.forward(CASE_NON_SQUARE)
    bad = R.im2col(c.a.reshape(c.Min, c.Cin).astype(np.float64), idx) @ c.Wf.astype(np.float64)
    out_f = _outside(p, bad)
    p = R.dgrad(CASE_NON_SQUARE)
    dy64, _ = R.dy_terms(c)
    idx = R.gather_index(c.B, c.Ho, c.Wo, c.H, c.W, c.k, c.stride, True, mutate="swap")
    bad = R.im2col(dy64, idx) @ c.Wb.astype(np.float64)
    out_t = _outside(p, bad)
    print(f"MUTATION c: outside {out_f:.1f}x forward, {out_t:.1f}x transposed")
    assert out_f > SENSITIVITY and out_t > SENSITIVITY


def test_mutation_padded_tap_formed_as_minus_ga_gmean():
    """(d) A padded tap of the operand formed as dy on load contributes ga*(0 - gmean) + gb*(0 - 0) instead of 0 (data gradient), and
    likewise a row past the pixel range in the weight gradient would: the BatchNorm blocks of make_case have GMEAN != 0."""
    c, p = R.make_case(CASE_PADDED_DY), R.dgrad(CASE_PADDED_DY)
    dy64, _ = R.dy_terms(c)
    fill = -(c.bn[R.BN_GA].astype(np.float64) * c.bn[R.BN_GMEAN].astype(np.float64))
    assert np.abs(fill).min() > 0
    bad = R.im2col(dy64, c.idx_t, fill=fill) @ c.Wb.astype(np.float64)
    border = np.zeros((c.B, c.H, c.W), bool)
    border[:, [0, -1]], border[:, :, [0, -1]] = True, True
    assert np.array_equal((bad != p.ref).any(1).reshape(c.B, c.H, c.W), border)  # only the border pixels see a padded tap
    out = _outside(p, bad)
    print(f"MUTATION d: outside {out:.1f}x  whole-tensor {p.rel(bad):.2e}")
    assert out > SENSITIVITY


def test_split_pieces_reproduce_the_scaled_value():
    """h + l = x * 2^s to 2^-22 relative for elements down to 2^-17 of the bound, an absolute 2^-25 below (floor_abs)."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(4096) * np.exp(3.0 * rng.standard_normal(4096))).astype(np.float32)
    bound = np.float32(np.abs(x).max())
    S = R.pow2_scale(bound)
    assert 2.0 ** 14 <= float(bound) * S < 2.0 ** 15 and R.pow2_scale(0.0) == 1.0 and R.pow2_scale(2.0) == 2.0 ** 13
    h, l = R.split_f16(x, S)
    err = np.abs((h + l) / S - x.astype(np.float64))
    assert np.all(err <= np.maximum(2.0 ** -22 * np.abs(x), R.floor_abs(x, bound)))
