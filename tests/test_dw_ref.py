"""tests/dw_ref.py on its own, without a GPU: the reference against torch float64 (conv2d and its autograd), the yardstick inside a band,
the case table against the tiling it claims (every kernel instantiation, every seam), `expected_path` at known points, the LDS bytes of
every admitted shape - and the mutations of the numpy model the criterion has to catch.

Mutations, each more than 10x outside the criterion in every case it applies to (the `MUTATION` lines of a run with -s have the figures),
and what the whole-tensor tolerances of tests/test_dwconv_gpu.py make of the SAME arrays (3e-6 max |y|, 5e-6 max |g| outside |pre| <= 1e-4,
3e-5 max |dW|, 2e-5 of the largest channel's sum |y - pivot| and 2e-5 relative on the squares) - computed here, not assumed:
  pad    a padding column of the staged dy formed from zero loads, ga (0 - gmean) + gb (0 - mean), instead of 0 (stride 1; 12 cases,
         2e5 to 3e6 x outside).
  seam   a forward band that opens an image inside a workgroup's run takes its shared rows from the band before it - the last rows of the
         PREVIOUS image (the carry without its `same image` test).  Applies where a run crosses an image boundary (7x8x78, 7x7x78 and
         the stride-2 13x10x33: an element whose every product is zero becomes non-zero, infinitely far outside).  At stride 2 with H odd
         the one row handed on is the zero row below the image and the mutation changes nothing (13x9x33: asserted as a no-op - which is
         why the table has 13x10x33 beside it).
  halo   the right halo column of the column tile next to the last one read as zero (the right halo of the last tile itself lies outside
         the image: zero in the reference too; 5 cases, 1e6 x).
  drop   one pixel left out of dW (every case, 7e2 to 2e6 x), and one pixel left out of the statistics (7e3 to 2e7 x).
  upper  the stride-2 bound test `ho > Ho - 1` removed on an even side: the tap reads row 0 of the next image (4 cases, 2e8 x or more).
  mask   the relu mask taken from bn(yprev) without the residual (14 cases, 1e6 x).
The old tolerances REJECT every one of these arrays as well, in every case above - none is accepted: with random inputs each mutation moves
some element by 1e-2 or more of its tensor's maximum, and one pixel of at most 4 368 is above 2e-5 of a channel's sum.  So what
tests/test_dwconv_gpu.py lacked against these defects is not the tolerance but the CASES - the seams at W = 78 | 79, ragged tiles, even sides
and single rows, a workgroup that walks at small B - and every check it does not make at all: the guards, the accumulation modes, the null
pointers, the rest of bn_prev.  The element-wise criterion adds what a maximum norm cannot see: an error confined to elements that are
small against their tensor's maximum, and exact zeros where every product is zero."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dw_ref as R
from conv_ref import BN_MEAN

_ids = lambda v: "x".join(map(str, v))
BOTH = [c for c in R.CASES if c not in R.FORWARD_ONLY]
U = R.U


def _channels(C):
    """a few channel blocks of a wide case: the first, the one with the second zero channel, the last"""
    if C <= 96:
        return np.arange(C)
    mid = (C // 2 + 3) // 32 * 32
    return np.concatenate([np.arange(32), np.arange(mid, mid + 32), np.arange(C - 32, C)])


def _nchw(x):
    return torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", R.CASES, ids=_ids, scope="module")  # grouped by case: dw_ref caches two
def test_reference_equals_torch_float64(case):
    c = R.make_case(case)
    ch = _channels(c.C)
    bn = c.bn_prev.astype(np.float64)[:, ch]
    pre = torch.from_numpy(bn[R.BN_SCALE] * (c.yprev[..., ch].astype(np.float64) - bn[R.BN_MEAN]) + bn[R.BN_BETA])
    if c.form == "stored":
        pre = pre + torch.from_numpy(c.x[..., ch].astype(np.float64))
    elif c.form == "raw":
        bs = c.bn_skip.astype(np.float64)[:, ch]
        pre = pre + torch.relu(torch.from_numpy(bs[R.BN_SCALE] * (c.raw[..., ch].astype(np.float64) - bs[R.BN_MEAN]) + bs[R.BN_BETA]))
    a = torch.relu(pre).requires_grad_(True)
    w = torch.from_numpy(c.w[ch].astype(np.float64)).reshape(len(ch), 1, 3, 3).requires_grad_(True)
    y = F.conv2d(a.permute(0, 3, 1, 2), w, stride=c.stride, padding=1, groups=len(ch))
    assert tuple(y.shape[-2:]) == (c.Ho, c.Wo)
    assert np.abs(y.detach().permute(0, 2, 3, 1).numpy() - c.y64[..., ch]).max() <= 1e-12
    assert np.array_equal(c.a64[..., ch], a.detach().numpy())
    if case in R.FORWARD_ONLY:
        return
    dy64, _ = R.dy_terms(c)
    y.backward(_nchw(dy64[..., ch]))
    G = a.grad.numpy() + (c.sg[..., ch].astype(np.float64) if c.sg is not None else 0.0)
    q = R.dgrad(case)
    assert np.abs(G - q.ref[..., ch]).max() <= 1e-12
    assert np.abs(G * (pre.numpy() > 0) - R.gprev_ref(case)[..., ch]).max() <= 1e-12
    dw = R.wgrad(case)
    assert np.abs(w.grad.reshape(len(ch), 9).numpy() - dw.ref[ch]).max() <= 1e-10 * max(1.0, np.abs(dw.ref).max())


@pytest.mark.parametrize("case", R.CASES, ids=_ids, scope="module")  # grouped by case: dw_ref caches two
def test_yardstick_band_and_planted_zeros(case):
    """Y between 0.1 U and 16 U for every quantity; at most UNDECIDED_CAP undecided mask elements; the planted zeros are where they
    should be: a_in of the zero pixels, s of y in the zero-weight channels."""
    c = R.make_case(case)
    y, a = R.forward(case)
    qs = {"y": y, "a_out": a}
    if case not in R.FORWARD_ONLY:
        dw = R.wgrad(case)
        qs.update(G=R.dgrad(case), dW=dw)
        print("YARD", _ids(case), f"dW serial {dw.E_serial / U:.2f} U blocked {dw.E_blocked / U:.2f} U")
        assert 0.1 * U <= min(dw.E_serial, dw.E_blocked)
    for name, q in qs.items():
        print("YARD", _ids(case), name, f"{q.Y / U:.2f} U")
        assert 0.1 * U <= q.Y <= 16 * U, (name, q.Y / U)
    assert c.share <= R.UNDECIDED_CAP
    assert np.all(y.s[..., c.zero_channels] == 0) and np.all(c.y64[..., c.zero_channels] == 0)
    assert (y.s > 0).mean() > 0.2  # (a single-pixel image without residual: half the channels are closed)
    for pix in c.zero_pixels:
        assert np.all(c.a64.reshape(-1, c.C)[pix] == 0) and np.all(c.Aabs.reshape(-1, c.C)[pix] == 0)
    assert np.any(c.bn_dw[R.BN_GMEAN] != 0)
    if c.form != "none":
        assert 0.05 < (c.a64 == 0).mean() < 0.95
    assert (c.sg is not None) == (c.form != "none" and c.stride == 1)


def _paths(case):
    return R.expected_path(*case[:5], False), R.expected_path(*case[:5], True)


def test_case_table_reaches_every_instantiation_and_seam():
    fwd = {R.fwd_instance(c) for c in R.CASES}
    assert fwd == {(s, f, k) for s in (1, 2) for f in R.FORMS for k in (False, True)}  # the launcher reaches all twelve
    bwd = {R.bwd_instance(c) for c in BOTH}
    assert bwd == {(1, f, k) for f in ("lean", "full", "raw") for k in (False, True)} | {(2, f, False) for f in ("lean", "full", "raw")}
    P = {c: _paths(c) for c in R.CASES}
    for case in R.CASES:
        assert case[0] * case[1] * case[2] * case[3] <= 10e6, case
        assert R.fwd_admitted(*case[:5])
    # H one below, at and one past a multiple of the band height, carried (R = 2 at W = 78, walking) and in column tiles (R = 18 at W = 79)
    for bwd_ in (0, 1):
        carried = {c[1] % 2 for c, p in P.items() if p[bwd_].carry and p[bwd_].walks and c[2] == 78}
        assert carried == {0, 1} and {c[1] for c, p in P.items() if p[bwd_].carry and c[2] == 78} >= {7, 8, 9}
        assert {c[1] for c, p in P.items() if p[bwd_].NCT > 1 and c[2] == 79} >= {17, 18, 19}
        assert any(p[bwd_].NCT > 1 and c[2] % p[bwd_].TW for c, p in P.items())            # a last column tile narrower than TW
        assert any(p[bwd_].NCT > 1 and p[bwd_].nbands > 1 for p in P.values())            # column tiles and bands at once
        assert any(p[bwd_].carry and p[bwd_].run_crosses for p in P.values())              # a run across an image boundary
        assert any(p[bwd_].carry and p[bwd_].run_inside for p in P.values())
        assert any(p[bwd_].carry and p[bwd_].run_midstart for p in P.values())
        assert any(p[bwd_].NI > 1 and c[0] % p[bwd_].NI and c[0] >= 30 for c, p in P.items())  # B large, not a multiple of the images per tile
        assert any(p[bwd_].NI == 1 and p[bwd_].nbands == 1 and p[bwd_].NCT == 1 and c[3] == 1024 for c, p in P.items())
    assert any(p[0].carry and p[0].run_crosses and c[4] == 2 for c, p in P.items())        # ... in the stride-2 forward carry too
    s2 = {(c[1] % 2, c[2] % 2) for c in BOTH if c[4] == 2}
    assert s2 == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(c[1], c[2]) for c in BOTH} >= {(1, 40), (40, 1), (1, 1), (2, 2)}
    assert {c[3] for c in BOTH} >= {32, 64, 512, 1024}
    assert set(R.POSITION_CASES) <= set(BOTH)
    forms = {(p[0].carry, p[0].NCT > 1, p[0].NI > 1) for c, p in P.items() if c in R.POSITION_CASES}
    assert forms >= {(True, False, False), (False, True, False), (False, False, True), (False, False, False)}


@pytest.mark.parametrize("case", R.CASES, ids=_ids, scope="module")  # grouped by case: dw_ref caches two
def test_tiles_partition_the_grid(case):
    """every pixel of the iterated grid belongs to exactly one tile of exactly one workgroup"""
    for P in _paths(case):
        seen = np.concatenate([R.tile_pixels(P, t) for wg in range(P.rows) for t in R.wg_tiles(P, wg)])
        assert np.array_equal(np.sort(seen), np.arange(P.B * P.Hg * P.Wg))


def test_expected_path_at_known_points():
    def chk(shape, bwd, **want):
        P = R.expected_path(*shape, bwd)
        assert {k: getattr(P, k) for k in want} == want, (shape, bwd)
    for bwd in (False, True):
        chk((7, 8, 78, 1024, 1), bwd, carry=True, NCT=1, R=2, nbands=4, NI=1, tiles=28, rows=24, walks=True, run_crosses=True)
        chk((3, 6, 79, 1024, 1), bwd, carry=False, NCT=5, TW=16, rows=15)
        chk((2, 3, 256, 32, 1), bwd, carry=False, NCT=16, TW=16, rows=32)
        chk((30, 5, 5, 1024, 1), bwd, NI=7, tiles=5, rows=5)
        chk((5, 17, 17, 1024, 1), bwd, NI=1, nbands=1, NCT=1, rows=5)
    chk((13, 9, 33, 1024, 2), False, carry=True, R=4, nbands=2, tiles=26, rows=24, run_crosses=True, lds=42368)
    chk((13, 9, 33, 1024, 2), True, carry=False, NI=3, nbands=1)
    chk((2, 5, 158, 32, 2), False, carry=True, R=1, nbands=3, lds=63488)
    chk((2, 5, 159, 32, 2), False, carry=False, R=1, nbands=3, lds=63872)
    chk((2, 5, 158, 32, 2), True, R=4, nbands=2)
    chk((2, 5, 159, 32, 2), True, R=4, nbands=2)
    chk((9, 9, 9, 512, 2), False, NI=3)
    chk((9, 9, 9, 512, 2), True, NI=8)
    chk((7, 8, 78, 1024, 1), False, lds=43008)
    chk((2, 65, 65, 32, 1), False, carry=True, R=3, nbands=22)     # the network's first layer: 3-row carried bands
    chk((2, 65, 65, 32, 2), False, carry=True, R=2)
    chk((2, 65, 65, 32, 2), True, carry=False, R=16)
    # the stale claims of tests/test_dwconv_gpu.py: 50 and 70 wide take carried full-width bands in both directions; column tiles from 79
    for W in (50, 70, 78):
        assert R.expected_path(2, 40, W, 32, 1, False).carry and R.expected_path(2, 40, W, 32, 1, True).carry
    for W in (79, 90, 100):
        assert R.expected_path(2, 40, W, 32, 1, False).NCT > 1 and R.expected_path(2, 40, W, 32, 1, True).NCT > 1
    chk((1, 3, 163, 32, 2), False, lds=65408)
    chk((1, 3, 164, 32, 2), False, lds=65792)
    chk((1, 3, 256, 32, 2), False, lds=101120)


def test_lds_bytes_over_the_admitted_range():
    """forward: over 64 KiB exactly for stride 2 and W >= 164 (refused by the launcher: include/ttk.h); backward: never above 52 KiB"""
    worst_b = 0
    for s in (1, 2):
        for W in range(1, 257):
            for H in (1, 2, 3, 5, 8, 19, 40, 300):
                for B in (1, 9):
                    f, b = R.expected_path(B, H, W, 32, s, False), R.expected_path(B, H, W, 32, s, True)
                    assert (f.lds > R.MAX_DYN_LDS) == (s == 2 and W >= 164), (B, H, W, s, f.lds)
                    assert R.fwd_admitted(B, H, W, 32, s) == (not (s == 2 and W >= 164))
                    worst_b = max(worst_b, b.lds)
    assert worst_b <= 52 * 1024
    assert R.fwd_admitted(1, 3, 163, 32, 2) and not any(R.fwd_admitted(*c) for c in R.OVERWIDE_FWD)
    assert not R.shape_ok(1, 4, 4, 32, 3) and not R.shape_ok(1, 4, 4, 48, 1) and not R.shape_ok(1, 4, 4, 2048, 1) and not R.shape_ok(1, 1, 257, 32, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# mutations
# ---------------------------------------------------------------------------------------------------------------------------------
def _report(name, case, outside, old_accepts):
    print("MUTATION", name, _ids(case), f"outside {outside:.3g}x", "old tolerance:", "ACCEPTS" if old_accepts else "rejects")
    assert outside > 10, (name, case, outside)


def _old_g(c, mut, ref):
    margin = np.abs(c.pre64) > 1e-4
    return np.abs((mut - ref) * margin).max() <= 5e-6 * np.abs(ref).max()


def _mut_pad(case):
    c, q = R.make_case(case), R.dgrad(case)
    dy64, _ = R.dy_terms(c)
    G = R.conv_bwd(dy64, c.w, 1, c.H, c.W, colfill=R.dy_fill(c)) + (c.sg if c.sg is not None else 0.0)
    _report("pad", case, R.masked_outside(q, G * c.open), _old_g(c, G * c.open, R.gprev_ref(case)))


def _seam(case):
    """y with every band that opens an image INSIDE a workgroup's run staged over the previous band's last rows"""
    c, P = R.make_case(case), R.expected_path(*case[:5], False)
    S, y = c.stride, c.y64.copy()
    for wg in range(P.rows):
        ts = R.wg_tiles(P, wg)
        for t in ts[1:]:
            n, _, band, r0, r1, _, _ = R.tile_geom(P, t)
            if band != 0:
                continue
            ap = np.pad(c.a64[n], ((1, 1), (1, 1), (0, 0)))
            prev = np.pad(c.a64[n - 1], ((1, 1), (1, 1), (0, 0)))  # padded rows: index r + 1
            last = 2 * c.Ho - 1 if S == 2 else c.H                 # the last staged row of the previous image's last band
            for k in range(3 - S):                                 # rows -1 .. of this band := the last 3 - S staged rows before it
                ap[k] = prev[last - (3 - S) + 1 + k + 1]
            y[n, r0:r1] = _conv_padded(ap, c.w, S, c.Ho, c.Wo)[r0:r1]
    return y


def _conv_padded(ap, w, S, Ho, Wo):
    """depthwise 3x3 of ONE image given with its border: ap[H + 2][W + 2][C]"""
    acc = np.zeros((Ho, Wo, ap.shape[2]))
    for kh in range(3):
        for kw in range(3):
            acc += ap[kh:kh + S * (Ho - 1) + 1:S, kw:kw + S * (Wo - 1) + 1:S] * w[:, kh * 3 + kw].astype(np.float64)
    return acc


def _mut_seam(case):
    c, (q, _) = R.make_case(case), R.forward(case)
    y = _seam(case)
    if c.stride == 2 and c.H % 2 == 1:  # the row handed on is the zero row below the image: the mutation changes nothing
        assert np.array_equal(y, c.y64)
        return
    _report("seam", case, q.outside(y), np.abs(y - c.y64).max() <= 3e-6 * np.abs(c.y64).max())


def _mut_halo(case):
    c, (q, _) = R.make_case(case), R.forward(case)
    P = R.expected_path(*case[:5], False)
    cx = (P.NCT - 1) * P.TW  # first column of the last tile = right halo of the tile before it
    a = c.a64.copy()
    a[:, :, cx] = 0.0
    y = c.y64.copy()
    y[:, :, cx - 1] = R.conv_fwd(a[:, :, cx - 2:cx + 1], c.w, 1, c.Ho, 3)[:, :, 1]
    _report("halo", case, q.outside(y), np.abs(y - c.y64).max() <= 3e-6 * np.abs(c.y64).max())


def _mut_drop(case):
    c, q = R.make_case(case), R.wgrad(case)
    dy64, _ = R.dy_terms(c)
    npix = c.B * c.H * c.W
    pix = next(p for p in range(npix // 2, npix) if np.any(c.a64.reshape(npix, c.C)[p] != 0))
    dw = q.ref - R.wgrad_pixel(c, dy64, c.a64, pix)
    _report("drop dW", case, q.outside(dw), np.abs(dw - q.ref).max() <= 3e-5 * np.abs(q.ref).max())
    # the statistics: one workgroup row holding the exact sums less one pixel, rounded once as the kernel rounds a row
    v = (c.y32.astype(np.float64) - c.piv).reshape(-1, c.C)
    k = v.shape[0] // 2
    part = np.stack([v.sum(0) - v[k], (v * v).sum(0) - v[k] ** 2]).astype(np.float32)[None]
    r = R.stat_ratios(part, v, v, True)
    whole = R.stat_ratios(np.stack([v.sum(0), (v * v).sum(0)]).astype(np.float32)[None], v, v, True)
    assert max(whole) <= 1.0  # ... and the same row with nothing left out is inside
    old0 = np.abs(v[k]).max() <= 2e-5 * np.abs(v).sum(0).max()
    old1 = np.all(v[k] ** 2 <= 2e-5 * (v * v).sum(0) + 1e-12)
    print("MUTATION drop stats", _ids(case), f"sum {r[0]:.3g}x squares {r[1]:.3g}x old tolerance: sum", "ACCEPTS" if old0 else "rejects",
          "squares", "ACCEPTS" if old1 else "rejects")
    assert r[0] > 10 and r[1] > 10
    g = R.gprev_ref(case).astype(np.float32).astype(np.float64).reshape(npix, c.C)
    d = (c.yprev.astype(np.float64) - c.bn_prev[BN_MEAN]).reshape(npix, c.C)
    live = np.abs(g).sum(0) > 0
    part = np.stack([g.sum(0) - g[pix], (g * d).sum(0) - (g * d)[pix]]).astype(np.float32)[None]
    if np.any(g[pix] != 0):
        assert min(R.stat_ratios(part[:, :, live], g[:, live], d[:, live], False)) > 10


def _mut_upper(case):
    c, q = R.make_case(case), R.dgrad(case)
    dy64, _ = R.dy_terms(c)
    G = R.conv_bwd(dy64, c.w, 2, c.H, c.W, wrap=True)
    _report("upper", case, R.masked_outside(q, G * c.open), _old_g(c, G * c.open, R.gprev_ref(case)))


def _mut_mask(case):
    c, q = R.make_case(case), R.dgrad(case)
    bn = c.bn_prev.astype(np.float64)
    bare = bn[R.BN_SCALE] * (c.yprev.astype(np.float64) - bn[R.BN_MEAN]) + bn[R.BN_BETA]
    gp = q.ref * (bare > 0)
    _report("mask", case, R.masked_outside(q, gp), _old_g(c, gp, R.gprev_ref(case)))


# name -> (the cases it applies to, the mutation); one test per case runs every mutation that applies to it
MUTATIONS = {
    "pad": (lambda c: c in BOTH and c[4] == 1, _mut_pad),
    "seam": (lambda c: _paths(c)[0].carry and _paths(c)[0].run_crosses, _mut_seam),
    "halo": (lambda c: _paths(c)[0].NCT > 1, _mut_halo),
    "drop": (lambda c: c in BOTH, _mut_drop),
    "upper": (lambda c: c in BOTH and c[4] == 2 and c[1] % 2 == 0, _mut_upper),
    "mask": (lambda c: c in BOTH and c[5] != "none", _mut_mask),
}


def test_every_mutation_applies_to_several_cases():
    n = {name: sum(bool(applies(c)) for c in R.CASES) for name, (applies, _) in MUTATIONS.items()}
    assert n == {"pad": 12, "seam": 4, "halo": 5, "drop": len(BOTH), "upper": 4, "mask": 14}, n
    # the seam changes the result in three of its four cases (13x9x33 stride 2: H odd, the row handed on is the zero row)
    assert sum(1 for c in R.CASES if MUTATIONS["seam"][0](c) and not (c[4] == 2 and c[1] % 2)) == 3


@pytest.mark.parametrize("case", R.CASES, ids=_ids, scope="module")
def test_mutations_land_outside_the_criterion(case):
    for name, (applies, run) in MUTATIONS.items():
        if applies(case):
            run(case)
