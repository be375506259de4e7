"""tests/anyc_ref.py on its own, without a GPU: the reference against torch float64 (matmul, conv2d and their autograd), the restated
layout against `_hip.to_blocks_any`, every yardstick inside the band (0, 2^-20) of tests/test_pw_ref.py, the planted zeros, the cap on
undecided mask elements, the case tables against the host logic they claim to reach (`wgrad_slices`, `fold_form`, `pix_rows`, `grid_1d`),
the fold model against a float64 sum, the derived statistics bound against a float32 model of the kernels' summation - and ten mutations of the numpy model, each more than 10x outside the criterion in every case it
applies to and asserted as a no-op where it truly is one (the `MUTATION` lines of a run with -s have the figures):
   1 stride32      the narrow last block of ydw addressed with row stride 32 instead of blk_w (no-op: M = 1, no narrow block)
   2 drop8         the last 8-group of K in the narrow block dropped (no-op: no narrow block)
   3 pad_rows      a row past a slice's end enters the weight gradient as ga (0 - gmean) (no-op: every slice a multiple of 8 rows)
   4 overlap       the rows between a slice's end and the next multiple of 8 counted in both slices (no-op: one slice, slices of 8 k rows)
   5 swap          H and W exchanged in the depthwise input index (no-op: H = W)
   6 wrapcol       the depthwise border read wraps to the neighbouring row (never a no-op: every case has a tap left of column 0)
   7 upper         the stride-2 backward `oh >= Ho` test dropped at even H: the tap is read from the next image (no-op: H odd, stride 1)
   8 acc_row       the accumulator-to-row map with h and r >> 2 exchanged (no-op: M = 1)
   9 taps_swapped  the stem tap with kh and kw exchanged
  10 mask          the pooled gradient's mask sign taken from the pre-activation without the residual (no-op: no residual)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import anyc_ref as R
import dw_ref
from conv_ref import dy_terms, BN_SCALE, BN_BETA, BN_MEAN, BN_GMEAN

_ids = lambda v: "x".join(map(str, v))
U = R.U
BAND = 2.0 ** -20
FAR = 10.0


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _close(got, ref, what):
    """to 1e-12 of scale"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, what
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), what


# ---------------------------------------------------------------------------------------------------------------------------------
# reference against torch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.PW_CASES + [R.SIDE_PW], ids=_ids)
def test_pointwise_reference_equals_torch_float64(case):
    c = R.pw_case(case)
    bn = c.bn_dw.astype(np.float64)
    a = torch.relu(_t(bn[BN_SCALE] * (c.ydw.astype(np.float64) - bn[BN_MEAN]) + bn[BN_BETA])).requires_grad_(True)
    w = _t(c.w.astype(np.float64)).requires_grad_(True)
    y = a @ w.T
    _close(y.detach().numpy(), c.y64, "y")
    assert np.array_equal(a.detach().numpy(), c.a64)
    dy64, _ = dy_terms(c)
    y.backward(_t(dy64))
    wg = R.pw_wgrad(case)
    _close(w.grad.numpy(), wg.ref, "dW")
    _close(R.pw_wgrad_model(c), wg.ref, "dW slice by slice")
    if "f" in R.PW_ENTRIES.get(case, "f"):
        _close(R.pw_forward(case).ref, c.y64, "forward")
        _close(R.pw_forward_model(c), c.y64, "forward model")
        _close(a.grad.numpy(), R.pw_dgrad(case).ref, "data gradient")


@pytest.mark.parametrize("case", R.DW_CASES + [R.SIDE_DW], ids=_ids)
def test_depthwise_reference_equals_torch_float64(case):
    c = R.dw_case(case)
    ch = np.arange(c.C) if c.C <= 96 else np.r_[0:32, c.C // 2:c.C // 2 + 32, c.C - 32:c.C]
    bn = c.bn_prev.astype(np.float64)[:, ch]
    pre = _t(bn[BN_SCALE] * (c.yprev[..., ch].astype(np.float64) - bn[BN_MEAN]) + bn[BN_BETA])
    if c.x is not None:
        pre = pre + _t(c.x[..., ch].astype(np.float64))
    a = torch.relu(pre).requires_grad_(True)
    w = _t(c.w[ch].astype(np.float64)).reshape(len(ch), 1, 3, 3).requires_grad_(True)
    y = F.conv2d(a.permute(0, 3, 1, 2), w, stride=c.stride, padding=1, groups=len(ch))
    assert tuple(y.shape[-2:]) == (c.Ho, c.Wo)
    qy, qa = R.dw_forward(case)
    _close(y.detach().permute(0, 2, 3, 1).numpy(), qy.ref[..., ch], "y")
    _close(R.dw_forward_model(c)[..., ch], qy.ref[..., ch], "y from the gathered taps")
    assert np.array_equal(qa.ref[..., ch], a.detach().numpy())
    dy64, _ = dw_ref.dy_terms(c)
    y.backward(_t(dy64[..., ch]).permute(0, 3, 1, 2))
    G = a.grad.numpy() + (c.sg[..., ch].astype(np.float64) if c.sg is not None else 0.0)
    _close(G, R.dw_dgrad(case).ref[..., ch], "G")
    _close(w.grad.reshape(len(ch), 9).numpy(), R.dw_wgrad(case).ref[ch], "dW")
    assert (c.sg is not None) == (case[5] == "skip" and c.stride == 1) == c.want_a


@pytest.mark.parametrize("case", R.STEM_CASES, ids=_ids)
def test_stem_reference_equals_torch_float64(case):
    c = R.stem_case(case)
    x = _t(c.x.astype(np.float64)).reshape(c.B, 1, c.H, c.W)
    w = _t(c.w.astype(np.float64)).reshape(c.C, 1, 5, 5).requires_grad_(True)
    y = F.conv2d(x, w, stride=2, padding=2)
    assert tuple(y.shape[-2:]) == (c.Ho, c.Wo)
    _close(y.detach().permute(0, 2, 3, 1).reshape(c.M, c.C).numpy(), c.fwd.ref, "y")
    _close(R.stem_forward_model(c), c.fwd.ref, "y model")
    dy64, _ = dy_terms(c)
    y.backward(_t(dy64.reshape(c.B, c.Ho, c.Wo, c.C)).permute(0, 3, 1, 2))
    _close(w.grad.reshape(c.C, 25).numpy(), c.wgrad.ref, "dW")


@pytest.mark.parametrize("case", R.POOL_CASES + [R.SIDE_POOL], ids=_ids)
def test_pool_reference_equals_torch_float64(case):
    c = R.pool_case(case)
    bn = c.bn.astype(np.float64)
    pre = _t(bn[BN_SCALE] * (c.y.astype(np.float64) - bn[BN_MEAN]) + bn[BN_BETA])
    if c.skip is not None:
        pre = pre + _t(c.skip.astype(np.float64))
    pre.requires_grad_(True)
    a = torch.relu(pre)
    feat = a.mean(1)
    assert np.array_equal(a.detach().numpy(), c.act.ref)
    _close(feat.detach().numpy(), c.feat.ref, "feat")
    feat.backward(_t(c.gfeat.astype(np.float64)))
    _close(pre.grad.numpy(), R.pool_bwd_model(c), "g")
    _close(R.pool_bwd_model(c), c.gin.ref * c.open, "g model")


# ---------------------------------------------------------------------------------------------------------------------------------
# layout and host logic
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", [(1, 8), (5, 16), (7, 24), (3, 32), (9, 40), (4, 64), (6, 72), (2, 104), (3, 2048), (130, 520)])
def test_layout_round_trips_with_to_blocks_any(M, C):
    import trackertraincode._hip as hip

    x = np.random.default_rng(M * 10000 + C).normal(0, 1, (M, C)).astype(np.float32)
    flat = R.to_blocks(x)
    assert np.array_equal(flat, hip.to_blocks_any(_t(x)).reshape(-1).numpy())
    assert np.array_equal(R.from_blocks(flat, M, C), x)
    assert np.array_equal(hip.from_blocks_any(_t(flat).view(M, C)).numpy(), x)
    if C % 32 == 0:
        assert np.array_equal(flat, hip.to_blocks(_t(x)).reshape(-1).numpy())
    assert R.n_blk(C) == -(-C // 32) and sum(R.blk_w(C, b) for b in range(R.n_blk(C))) == C
    assert sorted(R.off(m, c, M, C) for m in range(M) for c in range(C)) == list(range(M * C))  # a bijection onto the buffer


def test_channel_domain():
    assert [C for C in range(0, 2100) if R.c_ok(C)] == list(range(8, 2049, 8))


def test_slice_plans_of_the_table():
    for case, (slices, rows) in R.PW_SLICE_PLANS.items():
        assert (R.wgrad_slices(*case), R.rows_per(*case)) == (slices, rows), case
    plan = lambda c: [me - mb for mb, me in R.slice_plan(*c)]
    assert plan((129, 40, 72)) == [48, 48, 33]
    assert plan((65, 24, 48)) == [40, 25]
    assert plan((4033, 8, 8)) == [64] * 63 + [1]
    assert plan((4032, 8, 8)) == [64] * 63
    assert R.slice_plan(*R.EMPTY_SLICE_CASE)[9] == (648, 641)  # the tenth slice starts past M
    assert all(me > mb for mb, me in R.slice_plan(*R.EMPTY_SLICE_CASE)[:9])
    # the smallest such shape: no M below 641 at these channel counts, and no case of the table beside it, has an empty slice
    assert all(me > mb for M in range(1, 641) for mb, me in R.slice_plan(M, 520, 680))
    assert [c for c in R.PW_CASES if any(me <= mb for mb, me in R.slice_plan(*c))] == [R.EMPTY_SLICE_CASE]
    for c in R.PW_CASES:  # the slices tile [0, M) exactly
        live = [(mb, me) for mb, me in R.slice_plan(*c) if me > mb]
        assert live[0][0] == 0 and live[-1][1] == c[0] and all(a[1] == b[0] for a, b in zip(live, live[1:]))


def test_case_tables_reach_every_feature():
    pw = R.PW_CASES
    narrow = lambda C: C % 32
    for side, idx in (("K", 1), ("N", 2)):
        assert {8, 16, 24} <= {narrow(c[idx]) for c in R.pw_cases_of("f")}, side   # forward: K = Cin, N = Cout (data gradient: exchanged)
        assert {8, 16, 24} <= {narrow(c[idx]) for c in pw}, side
    # a 64-column workgroup tile whose second 32-column half is absent / narrow (forward N = Cout, data gradient N = Cin)
    half = lambda N: (N - 1) % 64 + 1  # columns of the last workgroup tile
    for idx in (1, 2):
        assert any(half(c[idx]) <= 32 for c in R.pw_cases_of("f")) and any(32 < half(c[idx]) < 64 for c in R.pw_cases_of("f"))
    assert {c[0] for c in R.pw_cases_of("f")} >= {1, 31, 32, 33, 127, 128, 129}
    folds = {R.fold_form(R.wgrad_slices(*c), c[1] * c[2]) for c in pw}
    assert folds == {"plain", "wide"}
    assert R.fold_form(63, 64) == "plain" and R.fold_form(64, 64) == "wide" and R.fold_form(64, 65537) == "plain"
    assert {1, 2, 3, 63, 64} <= {R.wgrad_slices(*c) for c in pw}
    assert {c[0] % 8 for c in pw if R.wgrad_slices(*c) == 1} >= {7, 1, 0}  # below, past and at an 8-row step in a single slice
    assert any(c[0] % 8 in (1, 2, 3) for c in pw) and any(c[0] % 8 in (5, 6, 7) for c in pw)  # a step that ends in either 4-row half
    assert any(R.n_blk(c[1]) * R.n_blk(c[2]) == 4096 for c in pw)
    for c in pw:
        zero, closed = R.pw_planted(c[1])
        assert len({*zero, closed}) == 3 and max(*zero, closed) < c[1]
        if c[1] % 32:
            assert any(z >= c[1] // 32 * 32 for z in zero), c  # one planted channel inside the narrow last block
    dw = R.DW_CASES
    s2 = [c for c in dw if c[4] == 2]
    assert {c[1] % 2 for c in s2} == {0, 1} and {c[2] % 2 for c in s2} == {0, 1}  # both parities of H and of W at stride 2
    assert {(c[1] % 2, c[2] % 2) for c in s2} >= {(1, 1), (0, 1), (1, 0), (0, 0)}
    assert any(c[1] < c[2] for c in dw) and any(c[1] > c[2] for c in dw)
    assert any(c[1] == 1 and c[2] > 1 for c in dw) and any(c[2] == 1 and c[1] > 1 for c in dw) and any(c[1] == c[2] == 1 for c in dw)
    assert {narrow(c[3]) for c in dw} >= {8, 16, 24, 0}
    assert any(R.n_blk(c[3]) == 64 for c in dw)
    pix = lambda c: c[0] * c[1] * c[2]
    rows = {R.pix_rows(pix(c)) for c in dw}
    assert 1 in rows and 2 in rows and R.MAX_ROWS in rows
    assert any(pix(c) > 4 * R.PIX_LANES * R.MAX_ROWS for c in dw)  # past the cap: a thread takes more pixels than the 4 the grid is sized for
    assert any(R.pix_rows(pix(c)) == 1 and pix(c) % 32 for c in dw)  # ragged pixel lanes
    assert any(c[5] == "skip" and c[4] == 1 for c in dw) and any(c[5] == "none" for c in dw)
    assert set(R.DW_POSITION_CASES) <= set(dw) and all(c[0] > 1 for c in R.DW_POSITION_CASES)
    st = R.STEM_CASES
    assert {(c[1] % 2, c[2] % 2) for c in st} == {(1, 1), (0, 1), (1, 0), (0, 0)} and {narrow(c[3]) for c in st} >= {8, 16, 24, 0}
    assert any(R.pix_rows(R.stem_case(c).M) > 1 for c in st) and any(c[1] != c[2] for c in st)
    pl = R.POOL_CASES
    assert {narrow(c[2]) for c in pl} >= {8, 24, 0} and {c[3] for c in pl} == {"skip", "none"}
    big = [c for c in pl if c[0] * c[1] * (c[2] // 4) > R.MAX_GRID_1D * R.BLOCK]  # bn_act's items
    assert big and all(c[0] * (c[2] // 4) > R.MAX_GRID_1D * R.BLOCK for c in big)  # ... and avgpool_fwd's: a second grid-stride step
    assert R.grid_1d(2100 * 512) == R.MAX_GRID_1D and R.grid_1d(4096 * 256) == 4096 and R.grid_1d(1) == 1
    assert [R.pix_rows(m) for m in (1, 128, 129, 131072, 131073, 10 ** 7)] == [1, 1, 2, 1024, 1024, 1024]
    # both families take the side-by-side shapes
    import pw_ref
    assert pw_ref.shape_ok(*R.SIDE_PW) and dw_ref.shape_ok(*R.SIDE_DW[:5]) and R.c_ok(R.SIDE_POOL[2]) and R.SIDE_POOL[2] % 32 == 0
    assert all(R.c_ok(C) for C in R.SIDE_PW[1:]) and R.c_ok(R.SIDE_DW[3])


@pytest.mark.parametrize("rows,n", [(1, 5), (3, 64), (63, 64), (64, 64), (70, 33), (64, 65537)])
def test_fold_model(rows, n):
    rng = np.random.default_rng(rows * 100 + n)
    part, base = rng.normal(0, 1, (rows, n)).astype(np.float32), rng.normal(0, 1, n).astype(np.float32)
    for b in (None, base):
        got = R.fold(part, b)
        assert got.dtype == np.float32
        ref = part.astype(np.float64).sum(0) + (0.0 if b is None else b.astype(np.float64))
        mag = np.abs(part.astype(np.float64)).sum(0) + (0.0 if b is None else np.abs(b))
        assert np.all(np.abs(got - ref) <= (rows + 8) * U * mag)
    if R.fold_form(rows, n) == "wide" and rows > 8:
        assert not np.array_equal(R.fold(part, form="wide"), R.fold(part, form="plain"))  # the two orders are told apart bit for bit


# ---------------------------------------------------------------------------------------------------------------------------------
# yardsticks, planted zeros, undecided share
# ---------------------------------------------------------------------------------------------------------------------------------
def _band(name, q, exact=False):
    print("YARD", name, f"{q.Y / U:.2f} U")
    if exact:
        assert q.Y == 0, name
    else:
        assert np.isfinite(q.Y) and 0 < q.Y < BAND, (name, q.Y)


@pytest.mark.parametrize("case", R.PW_CASES + [R.SIDE_PW], ids=_ids)
def test_pointwise_yardsticks_zeros_and_undecided_share(case):
    c = R.pw_case(case)
    w = R.pw_wgrad(case)
    _band(f"pw wgrad {_ids(case)}", w)
    assert np.all(w.s[:, c.zero_channels] == 0) and np.all(w.ref[:, c.zero_channels] == 0)
    assert (w.s > 0).any()
    assert np.any(c.bn[BN_GMEAN] != 0)
    if "f" not in R.PW_ENTRIES.get(case, "f"):
        return
    f, d = R.pw_forward(case), R.pw_dgrad(case)
    _band(f"pw fwd {_ids(case)}", f)
    _band(f"pw dgrad {_ids(case)}", d)
    assert np.all(f.s > 0)
    assert d.share <= R.UNDECIDED_CAP
    assert not c.open[:, c.closed_channel].any() and not c.undecided[:, c.closed_channel].any()  # its data-gradient column: exactly 0
    assert not c.open[:, c.zero_channels].any() and not c.undecided[:, c.zero_channels].any()
    assert np.all(c.aabs[:, c.zero_channels] == 0) and np.all(c.aabs[:, c.closed_channel] == 0)


@pytest.mark.parametrize("case", R.DW_CASES + [R.SIDE_DW], ids=_ids)
def test_depthwise_yardsticks_zeros_and_undecided_share(case):
    c = R.dw_case(case)
    y, a = R.dw_forward(case)
    g, w = R.dw_dgrad(case), R.dw_wgrad(case)
    for name, q in (("y", y), ("a_out", a), ("G", g), ("dW", w)):
        _band(f"dw {name} {_ids(case)}", q)
    print("YARD dw dW", _ids(case), f"serial {w.E_serial / U:.2f} U blocked {w.E_blocked / U:.2f} U")
    assert min(w.E_serial, w.E_blocked) > 0
    assert c.share <= R.UNDECIDED_CAP and g.share == c.share
    assert np.all(y.s[..., c.zero_channels] == 0)  # the zero weight channels
    assert np.all(g.s[..., c.zero_channels] == (0 if c.sg is None else np.abs(c.sg[..., c.zero_channels])))
    assert len(c.zero_pixels) == (2 if c.B * c.H * c.W >= 8 else 0)
    for pix in c.zero_pixels:
        assert np.all(c.a64.reshape(-1, c.C)[pix] == 0) and np.all(c.Aabs.reshape(-1, c.C)[pix] == 0)


@pytest.mark.parametrize("case", R.STEM_CASES, ids=_ids)
def test_stem_yardsticks(case):
    c = R.stem_case(case)
    _band(f"stem y {_ids(case)}", c.fwd)
    _band(f"stem dW {_ids(case)}", c.wgrad)
    assert min(c.wgrad.E_serial, c.wgrad.E_blocked) > 0 and np.all(c.fwd.s > 0)
    assert np.all((c.wgrad.s == 0) == (np.abs(c.X).sum(0) == 0)[None, :])  # a tap that only ever reads padding: an exact zero


@pytest.mark.parametrize("case", R.POOL_CASES + [R.SIDE_POOL], ids=_ids)
def test_pool_yardsticks_zeros_and_undecided_share(case):
    c = R.pool_case(case)
    _band(f"pool feat {_ids(case)}", c.feat)
    _band(f"pool act {_ids(case)}", c.act)
    # HW = 1: 1 / HW = 1 and gfeat * 1 is exact - Y is 0 and the criterion is the final rounding alone
    _band(f"pool g {_ids(case)}", c.gin, exact=c.HW & (c.HW - 1) == 0)
    assert c.share <= R.UNDECIDED_CAP
    if c.M >= 8:
        flat = c.Aabs.reshape(c.M, c.C)
        assert np.all(flat[[1, c.M - 2]] == 0)


@pytest.mark.parametrize("case", R.DW_CASES, ids=_ids)
def test_statistics_bound_holds_for_the_family_order_and_catches_a_dropped_pixel(case):
    """the float32 sums of the given y - pivot in the kernels' order meet the derived bound; with one pixel left out they do not"""
    c = R.dw_case(case)
    M = c.B * c.Ho * c.Wo
    v = (c.y32 - c.piv).reshape(M, c.C)  # float32: rounded once
    v64, L = v.astype(np.float64), R.pix_stat_length(M)
    assert L == -(-M // (32 * R.pix_rows(M))) + 32
    r = R.stat_ratios(R.stat_rows_model(v, v64), v64, v64, True, L)
    print("STATMODEL", _ids(case), f"{r[0]:.3f} {r[1]:.3f}")
    assert max(r) <= 1.0
    live = np.abs(v64).max(1)
    if live.max() > 0:
        r = R.stat_ratios(R.stat_rows_model(v, v64, drop=int(live.argmax())), v64, v64, True, L)
        assert min(r) > 1.0, r
    assert R.GEMM_STAT_LENGTH == 21


# ---------------------------------------------------------------------------------------------------------------------------------
# mutations
# ---------------------------------------------------------------------------------------------------------------------------------
def _mutation(name, case, q, x, noop, masked=False):
    r = R.outside(q, x, masked)
    print("MUTATION", name, _ids(case), "no-op" if noop else f"{r:.3g}")
    if noop:
        assert r <= 1e-3, (name, case, r)  # the float64 model itself: far inside
    else:
        assert r > FAR, (name, case, r)


@pytest.mark.parametrize("case", R.pw_cases_of("f"), ids=_ids)
def test_mutations_of_the_pointwise_forward(case):
    c, q = R.pw_case(case), R.pw_forward(case)
    M, Cin, _ = case
    assert R.outside(q, R.pw_forward_model(c)) <= 1e-3
    _mutation("stride32", case, q, R.pw_forward_model(c, "stride32"), noop=M == 1 or Cin % 32 == 0)
    _mutation("drop8", case, q, R.pw_forward_model(c, "drop8"), noop=Cin % 32 == 0)
    _mutation("acc_row", case, q, R.pw_forward_model(c, "acc_row"), noop=M == 1)


@pytest.mark.parametrize("case", R.PW_CASES, ids=_ids)
def test_mutations_of_the_pointwise_weight_gradient(case):
    c, q = R.pw_case(case), R.pw_wgrad(case)
    assert R.outside(q, R.pw_wgrad_model(c)) <= 1e-3
    _mutation("pad_rows", case, q, R.pw_wgrad_model(c, "pad_rows"), noop=R.pad_rows(*case) == 0)
    _mutation("overlap", case, q, R.pw_wgrad_model(c, "overlap"), noop=R.overlap_rows(*case) == 0)


def test_the_weight_gradient_mutations_apply_where_the_table_says():
    assert [c for c in R.PW_CASES if R.pad_rows(*c) == 0] == [(32, 16, 24), (128, 48, 96), (200, 2048, 8), (64, 72, 24), (4032, 8, 8)]
    assert [c for c in R.PW_CASES if R.overlap_rows(*c)] == [(129, 40, 72), (161, 104, 136), (200, 2048, 8), (65, 24, 48), (641, 520, 680)]


@pytest.mark.parametrize("case", R.DW_CASES, ids=_ids)
def test_mutations_of_the_depthwise_pair(case):
    c = R.dw_case(case)
    B, H, W, C, S, _ = case
    qy, _ = R.dw_forward(case)
    assert R.outside(qy, R.dw_forward_model(c)) <= 1e-3
    _mutation("swap", case, qy, R.dw_forward_model(c, "swap"), noop=H == W)
    # the tap left of column 0 exists in every case; it reads the pixel before (the first pixel of the tensor: itself) - never a no-op
    _mutation("wrapcol", case, qy, R.dw_forward_model(c, "wrapcol"), noop=False)
    qg = R.dw_dgrad(case)
    dy64, _ = dw_ref.dy_terms(c)
    G = R.conv_bwd(dy64, c.w, S, H, W, wrap=True) + (c.sg if c.sg is not None else 0.0)
    _mutation("upper", case, qg, G * c.open, noop=S == 1 or H % 2 == 1, masked=True)


@pytest.mark.parametrize("case", R.STEM_CASES, ids=_ids)
def test_mutation_of_the_stem_taps(case):
    c = R.stem_case(case)
    _mutation("taps_swapped", case, c.fwd, R.stem_forward_model(c, "taps_swapped"), noop=False)


@pytest.mark.parametrize("case", [c for c in R.POOL_CASES if c not in R.POOL_FWD_ONLY], ids=_ids)
def test_mutation_of_the_pooled_gradient_mask(case):
    c = R.pool_case(case)
    assert R.outside(c.gin, R.pool_bwd_model(c), masked=True) <= 1e-3
    _mutation("mask", case, c.gin, R.pool_bwd_model(c, "mask_without_skip"), noop=c.skip is None, masked=True)
