"""tests/stem_ref.py on its own, without a GPU: the im2col reference of the 5x5 stem against torch's float64 convolution and its autograd;
rne_bf16 against torch's conversion; the restated launch arithmetic against what every case of the table claims to reach; the yardstick
inside the criterion; and eight mutations of the reference's OWN float32 result (the fma chain), each of which must land outside the
criterion that tests/test_stem_rows_gpu.py holds the kernels to.  Every mutation prints by how much it is outside, and what the only
earlier kernel-level test (tests/test_dwconv_gpu.py: max |err| <= 3e-6 max |y|, 3e-5 max |dw| for the gradient, sums to 2e-5, fp32 storage
only) makes of it as `old`:
  * the old norm PASSES (g) and (h) by construction - it never ran bf16 storage - and (h) also numerically: the sums of the unrounded
    values differ from those of the stored ones by less than its 2e-5;
  * (a) - (f) change elements by far more than 3e-6 of the maximum: the old norm would catch them AT A SHAPE THAT RUNS THE PATH, but of
    its four shapes (all B <= 4, W <= 129, height-6 gradient bands, one band per workgroup) none stages a second band (c), and it calls
    the gradient one way only.  What the per-element criterion adds for them is the location (the assertion names the element) and exact
    zeros where every product is zero."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stem_ref as S

_ids = lambda v: "x".join(map(str, v))
OLD_FWD, OLD_WGRAD, OLD_SUMS = 3e-6, 3e-5, 2e-5  # tests/test_dwconv_gpu.py


def _outside(p, x):
    """worst |x - f64| / allowed over the elements: > 1 fails the criterion"""
    allowed = p.allowed()
    err = np.abs(np.asarray(x, np.float64) - p.ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(allowed > 0, err / np.where(allowed > 0, allowed, 1.0), np.where(err == 0, 0.0, np.inf)).max())


def _old(p, x, tol):
    """the whole-tensor maximum of the old test over its tolerance: > 1 fails it"""
    return float(np.abs(np.asarray(x, np.float64) - p.ref).max() / (tol * np.abs(p.ref).max()))


def _report(name, out, old):
    print(f"MUTATION {name}: outside {out:.3g}x  old {old:.3g}x")
    assert out > 1.0, name


# ---- the table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,claim", S.CASES, ids=[_ids(s) for s in S.SHAPES])
def test_case_reaches_its_stated_path(shape, claim):
    f = S.facts(*shape)
    for k, v in claim.items():
        assert f.get(k) == v, (shape, k, f.get(k), v)
    assert min(shape[1:]) >= 5  # admitted by both entry points


def test_table_covers_every_form_edge_and_loop():
    fs = {s: S.facts(*s) for s in S.SHAPES}
    assert len(set(S.SHAPES)) == len(S.SHAPES) and set(S.BF16_SHAPES) <= set(S.SHAPES)
    assert {f["fwd_form"] for f in fs.values()} == {"band", "gather"}
    assert any(f.get("fwd_second_band", 0) > 0 and f["fwd_grid"] > 1 for f in fs.values())      # forward persistent loop
    assert any(f.get("fwd_second_tile", 0) > 0 for f in fs.values())                             # gather: a wave's second tile
    assert any(f.get("wgrad_second_tile", 0) > 0 and f["wgrad_rows"] > 6 for f in fs.values())   # gradient persistent loop above 6
    assert {f["wgrad_rows"] for f in fs.values() if f["wgrad_fits"]} >= {3, 4, 5, 6, 7, 11, 13}
    assert any(len(set(f.get("fwd_band_heights", ()))) > 1 for f in fs.values())                 # a short band behind a full one
    assert any(f.get("fwd_idle", 0) > 0 for f in fs.values())                                    # idle workgroups write zero sums
    # the bf16 subset keeps one case of each: both forward kernels, both persistent loops
    bf = [fs[s] for s in S.BF16_SHAPES]
    assert {f["fwd_form"] for f in bf} == {"band", "gather"}
    assert any(f.get("fwd_second_band", 0) > 0 for f in bf) and any(f.get("wgrad_second_tile", 0) > 0 for f in bf)
    # the edges of the two LDS tests
    assert S.wgrad_fits(313) and not S.wgrad_fits(314) and S.REFUSED_WIDTH == (1, 5, 314)
    assert S.fwd_dynamic_lds(393) + S.FWD_STATIC_LDS <= S.LDS_LIMIT < S.fwd_dynamic_lds(394) + S.FWD_STATIC_LDS
    assert S.fwd_form(402) == "band" and S.fwd_form(403) == "gather"
    assert all(s in S.SHAPES for s in ((1, 5, 313), (1, 5, 393), (1, 5, 402), (1, 5, 403)))
    # no forward case is past the 32-bit pixel index the host checks, and the gradient's scratch has a row per workgroup
    assert all(f["P"] < 2 ** 31 and f.get("wgrad_grid", 0) <= 1024 for f in fs.values())


def test_band_rows_search_and_small_batches():
    found = S.heights_search()
    assert set(range(6, 14)) <= set(found)  # every height is reachable under B <= 1600, Ho <= 26
    for h, shape in S.HEIGHT_CASES.items():
        assert found[h] == shape and shape in S.SHAPES
    # what the issue states of the old test's shapes, and of training
    for B, Ho in ((2, 65), (3, 17), (4, 10), (1, 6), (768 // 11, 65)):
        assert S.wgrad_band_rows(B, Ho) == 6
    assert S.wgrad_band_rows(512, 65) == 11 and S.wgrad_band_rows(769, 13) == 7
    assert [S.wgrad_band_rows(1, Ho) for Ho in range(1, 8)] == [1, 2, 3, 4, 5, 6, 6]


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 6, 5), (5, 7, 9), (3, 33, 33)], ids=_ids)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_reference_equals_torch_float64(shape, bf16):
    c = S.stem5_case(*shape, bf16=bf16)
    x64 = torch.from_numpy(c.x).double().unsqueeze(1)
    w64 = torch.from_numpy(c.w).double().reshape(S.C, 1, 5, 5).requires_grad_(True)
    y64 = F.conv2d(x64, w64, stride=2, padding=2)
    assert tuple(y64.shape[-2:]) == (c.Ho, c.Wo)
    close = lambda a, ref: np.abs(a - ref).max() <= 1e-12 * np.abs(ref).max()
    assert close(c.fwd.ref, y64.detach().permute(0, 2, 3, 1).reshape(c.M, S.C).numpy())
    dy64, D = S.dy_terms(c)  # of the (g, y32) the gradient is given
    (gw,) = torch.autograd.grad(y64, w64, torch.from_numpy(dy64).reshape(c.B, c.Ho, c.Wo, S.C).permute(0, 3, 1, 2))
    assert close(c.wgrad.ref, gw.reshape(S.C, S.TAPS).numpy())
    assert np.all(D >= np.abs(dy64)) and np.abs(c.bn[S.BN_GMEAN]).min() > 0
    # exact zeros where the case says: the zero image's outputs; no weight-gradient element is without a product
    zero_px = np.zeros((c.B, c.Ho, c.Wo), bool)
    zero_px[c.B // 2] = True
    assert np.all(c.fwd.s[zero_px.reshape(-1)] == 0) and (c.fwd.s > 0).any(1)[~zero_px.reshape(-1)].all() and np.all(c.wgrad.s > 0)
    if bf16:
        for v in (c.y32, c.g):
            assert np.array_equal(S.rne_bf16(v), v)  # already bf16 values
        assert not np.array_equal(c.y32, c.fwd.ref.astype(np.float32))


def test_rne_bf16_equals_torch_and_is_monotone():
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(1 << 16) * np.exp(4.0 * rng.standard_normal(1 << 16))).astype(np.float32)
    ties = ((rng.integers(0x3f00, 0x4100, 4096).astype(np.uint32) << 16) | 0x8000).view(np.float32)  # exactly between two bf16 values
    x = np.concatenate([x, ties, -ties, np.float32([0.0, -0.0, 1.0, 2.0 ** -126, 2.0 ** -133])])
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    assert np.array_equal(S.rne_bf16(x).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(S.bf16_widen(S.bf16_bits(x)), S.rne_bf16(x))
    xs = np.sort(x)
    assert np.all(np.diff(S.rne_bf16(xs).astype(np.float64)) >= 0)
    assert (S.trunc_bf16(x) != S.rne_bf16(x)).mean() > 0.3


@pytest.mark.parametrize("shape", [(5, 7, 9), (40, 9, 9), (1, 5, 313)], ids=_ids)
def test_yardstick_satisfies_the_criterion(shape):
    for bf16 in (False, True):
        c = S.stem5_case(*shape, bf16=bf16)
        for name, p in (("fwd", c.fwd), ("wgrad", c.wgrad)):
            assert np.isfinite(p.Y) and 0 < p.Y < 64 * S.U, (name, p.Y)
            ratio, zeros_ok = p.ratio(p.chain)
            assert zeros_ok and ratio <= 1.0 and _outside(p, p.chain) <= 1.0
        q = S.onto(c.wgrad, c.dw0)
        ratio, zeros_ok = q.ratio((c.dw0.astype(np.float64) + c.wgrad.chain).astype(np.float32))
        assert zeros_ok and ratio <= 1.0
    # the bf16 forward: the rounded chain is inside the bracket, its sums pass, and the figure printed for it is small
    stored = S.rne_bf16(c.fwd.chain)
    assert S.bracket_outside(c.fwd, stored) == 0 and S.bracket_ratio(c.fwd, stored) <= S.MARGIN
    own = stored.astype(np.float64) - c.piv
    assert S.sums_outside(own.sum(0), (own ** 2).sum(0), own, own) <= 1e-9
    # ... and -0 where +0 is due is not
    if (c.fwd.s == 0).any():
        bad = stored.copy()
        bad[np.argwhere(c.fwd.s == 0)[0][0]] = -0.0
        assert S.bracket_outside(c.fwd, bad) == S.C


# ---- mutations of the reference's own float32 result -------------------------------------------------------------------------------
def test_mutation_a_tap_25_of_the_upper_half_wave():
    """The 13th k-pair of the upper half-wave is tap 25, which does not exist: its LDS offset is 0 (the patch's first pixel), its weight
    index runs into the next channel's tap 0.  Neither zeroed: every pixel gains x[first pixel of the patch] * w[c + 1][0]."""
    c = S.stem5_case(3, 33, 33)
    w_next = np.append(c.w.reshape(-1)[S.TAPS::S.TAPS], 0.0)  # w[c * 25 + 25]; past the array for c = 31: taken as 0
    bad = c.fwd.chain + c.X[:, :1].astype(np.float64) * w_next
    _report("a", _outside(c.fwd, bad), _old(c.fwd, bad, OLD_FWD))


def test_mutation_b_halo_row_dropped_from_a_band():
    """The last of the 2 * 13 + 3 staged rows of the first band of (1, 60, 9) is missing (zeros): the taps kh = 4 of output row 12."""
    c = S.stem5_case(1, 60, 9)
    rows = np.arange(12 * c.Wo, 13 * c.Wo)
    Xb = c.X[rows].copy()
    Xb[:, 20:] = 0.0
    bad = c.fwd.chain.copy()
    bad[rows] = S.chain32(Xb, c.fwd.B32)
    assert np.array_equal(np.delete(bad, rows, 0), np.delete(c.fwd.chain, rows, 0))
    _report("b", _outside(c.fwd, bad), _old(c.fwd, bad, OLD_FWD))


def test_mutation_c_last_row_from_the_previous_bands_staging():
    """(40, 9, 9): workgroup 0 takes the bands of images 0 and 32.  Without the barrier in front of the re-staging a wave still reads
    image 0's rows for the last output row of image 32."""
    c = S.stem5_case(40, 9, 9)
    f = S.facts(40, 9, 9)
    first, second = 0, f["fwd_grid"]  # bt = blockIdx.x, then += gridDim.x; one band per image
    assert second < f["fwd_bands"] and first != c.B // 2 != second
    per = c.Ho * c.Wo
    row = lambda n: np.arange(n * per + (c.Ho - 1) * c.Wo, (n + 1) * per)
    bad = c.fwd.chain.copy()
    bad[row(second)] = c.fwd.chain[row(first)]
    _report("c", _outside(c.fwd, bad), _old(c.fwd, bad, OLD_FWD))


def test_mutation_d_left_pad_of_one_column():
    """The band staged with one zero column on the left instead of two: every tap reads the pixel one column to the right."""
    c = S.stem5_case(2, 5, 6)
    xs = np.zeros_like(c.x)
    xs[:, :, :-1] = c.x[:, :, 1:]
    bad = S.chain32(S.patches(xs), c.fwd.B32)
    _report("d", _outside(c.fwd, bad), _old(c.fwd, bad, OLD_FWD))


def test_mutation_e_gmean_not_subtracted_at_padded_taps():
    """Weight gradient of (5, 7, 9): a band is 20 pixels, a wave's chunk 32.  The 12 lanes past the band load the band's pixel 0 again
    (the clamped address); they must contribute 0.  Formed as dy = ga*(0 - gmean) + gb*(0 - mean) against that pixel's patch instead -
    the padded k-steps of the contraction, where GMEAN != 0 shows - every band adds 12 such terms."""
    c = S.stem5_case(5, 7, 9)
    bn = c.bn.astype(np.float64)
    ghost = -(bn[S.BN_GA] * bn[S.BN_GMEAN] + bn[S.BN_GB] * bn[S.BN_MEAN])
    per = c.Ho * c.Wo
    assert S.facts(5, 7, 9)["wgrad_rows"] == c.Ho and per == 20
    bad = c.wgrad.chain + sum((32 - per) * np.outer(ghost, c.X[n * per].astype(np.float64)) for n in range(c.B))
    _report("e", _outside(c.wgrad, bad), _old(c.wgrad, bad, OLD_WGRAD))


def test_mutation_f_sums_of_y_instead_of_y_minus_pivot():
    c = S.stem5_case(5, 7, 9)
    flat = c.fwd.ref - c.piv
    y = c.fwd.chain
    out = S.sums_outside(y.sum(0), (y ** 2).sum(0), flat, y - c.piv)
    old = max(np.abs(y.sum(0) - flat.sum(0)).max() / (OLD_SUMS * np.abs(flat).sum(0).max()),
              (np.abs((y ** 2).sum(0) - (flat ** 2).sum(0)) / (OLD_SUMS * (flat ** 2).sum(0))).max())
    assert S.sums_outside((y - c.piv).sum(0), ((y - c.piv) ** 2).sum(0), flat, y - c.piv) <= 1.0
    _report("f", out, old)


def test_mutation_g_bf16_by_truncation():
    """must fall outside the bracket on some element"""
    c = S.stem5_case(5, 7, 9, bf16=True)
    acc = c.fwd.chain.astype(np.float32)
    assert S.bracket_outside(c.fwd, S.rne_bf16(acc)) == 0
    n = S.bracket_outside(c.fwd, S.trunc_bf16(acc))
    print(f"MUTATION g: {n} of {acc.size} elements outside the bracket  old: never ran bf16 storage")
    assert n > 0


def test_mutation_h_statistics_of_the_unrounded_value():
    """bf16 storage: the sums must be those of the values as stored.  The sums of the unrounded accumulators leave the 3e-5 of the squares
    at 100 pixels and still at 8450 (the rounding errors of 2^-9 average out with the square root of the count only)."""
    for shape in ((5, 7, 9), (2, 129, 129)):
        c = S.stem5_case(*shape, bf16=True)
        acc = c.fwd.chain.astype(np.float32).astype(np.float64)
        own = S.rne_bf16(acc).astype(np.float64) - c.piv
        S1, S2 = (acc - c.piv).sum(0), ((acc - c.piv) ** 2).sum(0)
        out = S.sums_outside(S1, S2, own, own)
        flat = c.fwd.ref - c.piv
        old = max(np.abs(S1 - flat.sum(0)).max() / (OLD_SUMS * np.abs(flat).sum(0).max()),
                  (np.abs(S2 - (flat ** 2).sum(0)) / (OLD_SUMS * (flat ** 2).sum(0))).max())
        print(f"MUTATION h {_ids(shape)}: outside {out:.3g}x  old {old:.3g}x")
        assert out > 1.0
