"""tests/bc_ref.py on its own, without a GPU: the reference against torch float64 at 1e-12, the restated layout against
`_hip.to_blocks64`, the exact float32 helpers against float32 arithmetic, `expected_path` against the C ABI's queries where the library
loads, the caps on undecided operands and widened outputs for every case of the table (zero undecided for the short constants), the
coverage of the table, a numpy emulation of the kernels' arithmetic inside every bound - and planted errors in that emulation, each in a
named case and each more than 10x outside the criterion (the `MUTATION` lines of a run with -s have the figures):
    trunc_operand        the operand truncated to bf16 instead of rounded to nearest even
    trunc_weights        the weight image rounded by truncation
    shift_plus_mean      the forward shift formed as beta + scale * mean
    gmean_mean_swapped   c0 from the two means exchanged
    drop_last_k16        the last k16 step of the contraction dropped (K = 32: half of a short chunk)
    block_stride_64      the second 64-channel block of the operand read one pixel row off
    tile_starts_late     a row tile that starts one pixel late
    mask_other_chunk     the mask taken from the next 8-channel chunk
    mask_ge              the mask ignored (every element open)
    second_sum_beta      the second partial sum of the data gradient against beta instead of mean
    padding_counted      the clamped copies of the last pixel counted in the partial sums
and in the weight gradient (its section at the end): slice_starts_late (a slice that starts one pixel late), drop_last_k16 (the last k16
step of the last slice), skip_fold_row (one slice left out of the fold, fast and wide), trunc_operand;
in the depthwise forward: halo_wraps (a halo column that wraps to the previous row), swap_hw (H and W exchanged), skip_before_rounding
(`skip` added before the first rounding: shows in a_out at pixels the case plants), trunc_operand, and relu before the rounding (a no-op
on values, asserted: test_relu_before_the_rounding_is_the_same_operand); in the depthwise backward: a stride-2 parity class exchanged.
The caps hold by selection: every case takes the first of up to bc_ref.SALTS seeded draws whose reference meets them (`draw N` in the
CAPS lines) - the shares printed are those of the selected draws, not typical ones."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bc_ref as R
from conv_ref import BN_BETA, BN_GA, BN_GB, BN_GMEAN, BN_MEAN, BN_SCALE

_ids = R.case_id


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers of the reference
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", [(1, 32), (5, 32), (1, 64), (7, 64), (3, 128), (9, 256), (2, 1024)])
def test_layout_is_to_blocks64(M, C):
    import trackertraincode._hip as hip

    x = np.random.default_rng(M * 10000 + C).normal(0, 1, (M, C)).astype(np.float32)
    flat = R.to_blocks(x)
    assert np.array_equal(flat, hip.to_blocks64(_t(x)).reshape(-1).numpy())
    assert np.array_equal(R.from_blocks(flat, M, C), x)
    assert np.array_equal(hip.from_blocks64(_t(flat).view(M, C)).numpy(), x)
    for m, c in ((0, 0), (M - 1, C - 1), (M // 2, C // 2 + 1)):
        assert flat[R.off64(m, c, M, C)] == x[m, c]


def test_f32_of_rounds_to_nearest_even():
    F = R.Fr
    one, eps = F(1), F(1, 2 ** 23)
    assert R.f32_of(one + eps / 2) == np.float32(1.0)                       # a tie: to the even neighbour
    assert R.f32_of(one + eps + eps / 2) == np.float32(1.0 + 2.0 ** -22)    # a tie: up to the even neighbour
    assert R.f32_of(one + eps / 2 + F(1, 2 ** 80)) == np.float32(1.0 + 2.0 ** -23)  # just past a tie, below float64's resolution
    rng = np.random.default_rng(5)
    a, b, c = (rng.normal(0, 1, 200).astype(np.float32) for _ in range(3))
    for x, y, z in zip(a, b, c):
        assert R.f32_of(F(float(x)) * F(float(y))) == np.float32(x) * np.float32(y)
        assert R.f32_of(F(float(x)) + F(float(z))) == np.float32(x) + np.float32(z)


def test_fma32_is_the_exact_fma():
    """against exact rational arithmetic: where fma32 calls the sum exact its value is the correctly rounded fma; elsewhere lo and hi
    enclose it"""
    rng = np.random.default_rng(11)
    x = R.rne_bf16(rng.normal(0, 1, (64, 8)))
    k = rng.normal(0, 1, 8).astype(np.float32)
    c = (rng.normal(0, 1, (64, 8)) * 10.0 ** rng.integers(-9, 3, (64, 8))).astype(np.float32)
    lo, hi, inexact = R.fma32(x, k, c)
    assert inexact.any() and not inexact.all()
    for i in range(64):
        for j in range(8):
            want = R.f32_of(R.Fr(float(x[i, j])) * R.Fr(float(k[j])) + R.Fr(float(c[i, j])))
            assert lo[i, j] <= want <= hi[i, j]
            if not inexact[i, j]:
                assert lo[i, j] == hi[i, j] == want


@pytest.mark.parametrize("family", R.FAMILIES)
def test_constants(family):
    rng = np.random.default_rng(3)
    bn = (R.bn_full if family == "full" else R.bn_short)(1024, rng)
    c0 = R.c0_candidates(bn)
    sh = R.shift_of(bn)
    if family == "short":
        assert R.significant_bits(bn[[BN_SCALE, BN_BETA, BN_MEAN, BN_GA, BN_GB, BN_GMEAN]]).max() <= 8
        assert np.array_equal(c0[0], c0[1]) and np.array_equal(c0[0], c0[2])
        b = bn.astype(np.float64)
        assert np.array_equal(sh.astype(np.float64), b[BN_BETA] - b[BN_SCALE] * b[BN_MEAN])  # exact in every evaluation order
        assert np.array_equal(c0[0].astype(np.float64), -b[BN_GA] * b[BN_GMEAN] - b[BN_GB] * b[BN_MEAN])
    else:
        differ = (c0[0] != c0[1]) | (c0[0] != c0[2])
        print(f"c0 candidates differ in {differ.mean():.3f} of the channels")
        assert 0.2 < differ.mean() < 0.7                                      # the candidates matter: the reference must carry them
        assert np.abs(c0[1:].astype(np.float64) - c0[0]).max() <= 2.0 ** -23  # ... and are one rounding apart
        assert np.array_equal(c0[0], -bn[BN_GA] * bn[BN_GMEAN] - bn[BN_GB] * bn[BN_MEAN])  # numpy's float32: no contraction


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference against torch, the caps, the emulation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", R.SMALL_CASES, ids=_ids)
def test_reference_equals_torch_float64(case, family):
    c = R.pw_case(*case, family)
    d = lambda x: _t(np.asarray(x, np.float64))
    wb = d(c.wb)
    if c.mode == "fwd":
        bn = c.bn_dw.astype(np.float64)
        sh = R.shift_of(c.bn_dw).astype(np.float64)
        pre = d(bn[BN_SCALE]) * d(c.ydw) + d(sh)
        a = torch.relu(pre.to(torch.float32).to(torch.bfloat16).double())
        ref = torch.nn.functional.conv2d(a.T.reshape(1, c.cin, c.M, 1), wb.reshape(c.cout, c.cin, 1, 1)).reshape(c.cout, c.M).T
        decided = ~c.op.undecided
        assert np.array_equal(a.numpy()[decided], c.op.v.astype(np.float64)[decided])
    else:
        bn = c.bn_pw.astype(np.float64)
        c0 = R.c0_candidates(c.bn_pw)[0].astype(np.float64)
        inner = (d(bn[BN_GB]) * d(c.y) + d(c0)).to(torch.float32).double()
        dy = (d(bn[BN_GA]) * d(c.g) + inner).to(torch.float32).to(torch.bfloat16).double()
        ref = dy @ wb
        decided = ~c.op.inexact
        assert np.array_equal(dy.numpy()[decided], c.op.v.astype(np.float64)[decided])
    clean = ~(c.op.undecided | c.op.inexact).any(1)
    err = np.abs(ref.numpy() - c.p.ref)[clean]
    assert err.max() <= 1e-12 * max(np.abs(c.p.ref).max(), 1.0)
    assert 0 < c.p.Y < 2.0 ** -20


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_caps(case, family):
    c = R.pw_case(*case, family)
    share, widened = float(c.op.undecided.mean()), c.p.widened_share
    mask_u = 0 if c.open is None else int(c.mask_undecided.sum())
    print(f"CAPS {_ids(case)} {family} (draw {c.salt}): undecided {share:.2e} (inexact sums {c.op.inexact.mean():.2e}), widened {widened:.2e}, "
          f"undecided mask elements {mask_u}, Y {c.p.Y:.2e}, lds {c.path.lds}")
    if family == "short":
        assert not c.op.undecided.any() and not c.op.inexact.any() and mask_u == 0 and widened == 0
    else:
        assert share <= R.UNDECIDED_CAP and widened <= R.WIDENED_CAP
    assert c.path.lds <= R.LDS_LIMIT
    if c.M >= 3 and c.mode == "fwd":
        assert (c.p.s[1] == 0).all()          # the planted zero row
    if c.mode == "dgrad" and c.M >= 3:
        assert not c.open[1].any() and c.open.any()


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", R.SMALL_CASES, ids=_ids)
def test_emulation_meets_every_bound(case, family):
    c = R.pw_case(*case, family)
    v = R.model(c)
    assert R.outside(c.p, v, c.open, c.mask_undecided) == 0
    assert R.excess(c.p, v, None if c.open is None else c.open | c.mask_undecided) == 0
    if c.M >= 2:
        assert np.array_equal(v[0], v[-1])
    part = R.model_part(c, v)
    d, q = R.stat_terms(c, v.astype(np.float64))
    assert R.stats_outside(part, c.rows_of, d, q, c.L) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------------------
def test_tables_reach_every_instantiation_and_seam():
    paths = {case: R.expected_path(*case) for case in R.CASES}
    assert all(p is not None for p in paths.values())
    e = {(case[0],) + p.inst for case, p in paths.items() if p.kernel == "e"}
    assert e >= {("fwd", 2, 1), ("fwd", 4, 2), ("fwd", 4, 4), ("dgrad", 1, 2), ("dgrad", 2, 4), ("dgrad", 4, 4)}    # the network's six
    assert e == {(m, nb, kh) for m in ("fwd", "dgrad") for nb, kh in R.E_INSTANCES.values()}                        # and the other four
    l = {(case[0],) + p.inst for case, p in paths.items() if p.kernel == "l"}
    assert l == {("fwd", 128), ("dgrad", 128), ("fwd", 256), ("dgrad", 256)}
    for mode, (cin, cout) in [("fwd", s) for s in R.E_LAYERS] + [("dgrad", s) for s in R.E_LAYERS]:
        assert {c[1] for c in R.CASES if c[0] == mode and c[2:] == (cin, cout)} >= set(R.E_M)
    big = [p for case, p in paths.items() if p.kernel == "e" and case[1] == R.E_BIG_M]
    assert len(big) == 2 and all(p.grid == 256 and p.second_group == 9 for p in big)
    assert R.expected_path("fwd", 65536, 32, 64).second_group == 0
    assert {(c[2], c[3]) for c, p in paths.items() if p.kernel == "l" and c[0] == "fwd" and p.inst == (256,)} >= set(R.L_FWD_LAYERS)
    assert {(c[2], c[3]) for c, p in paths.items() if p.kernel == "l" and c[0] == "dgrad" and p.inst == (256,)} >= set(R.L_DGRAD_LAYERS)
    assert paths[("dgrad", 257, 128, 256)].inst == (128,) and paths[("fwd", 263, 256, 128)].inst == (128,)
    L = [(case, p) for case, p in paths.items() if p.kernel == "l" and p.inst == (256,)]
    rts = {p.RT for _, p in L}
    assert rts >= {8, 16, 24, 32, 40, 256} and any(128 <= rt <= 248 and rt % 32 for rt in rts)
    assert {p.ncol for _, p in L} == {1, 2, 4}
    assert any(p.RT == 256 and p.ncol == 1 and case[1] > 63488 for case, p in L) and any(p.RT == 256 and p.ncol == 4 and case[1] > 15872 for case, p in L)
    assert R.l_plan(63488, 256).RT < 256 and R.l_plan(15872, 1024).RT < 256
    assert any(p.rounds == 2 and p.ncol == 1 for _, p in L) and R.l_plan(65536, 256).rounds == 1
    assert any(p.nrt % 8 and p.idle > 0 for _, p in L)
    ms = {case[1] for case, p in L if p.RT == 16 and case[2:] == (128, 1024)}
    assert any(m % 16 == 0 and m - 1 in ms and m + 1 in ms for m in ms)        # one below, at and one past a multiple of RT
    assert any(p.nrt > 1 and case[1] % p.RT == 1 for case, p in L)              # a last row tile of one pixel
    assert any(case[0] == "dgrad" and p.ncol == 2 and p.RT == 16 for case, p in L)
    # every case the GPU test allocates stays in the tens of MB
    assert max(c[1] * max(c[2], c[3]) for c in R.CASES) * 2 <= 64 << 20


def _cdll():
    import trackertraincode._hip as hip
    if not os.path.exists(hip.LIB_PATH):
        return None
    lib = ctypes.CDLL(hip.LIB_PATH)    # (a library that is there and does not load is an error)
    lib.ttk_bc_partial_rows_pw.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    lib.ttk_bc_partial_rows_pw.restype = ctypes.c_int
    return lib


POW2 = [32, 64, 128, 256, 512, 1024]


def test_expected_path_is_the_query_of_the_library():
    """where libttk_hip.so loads without a GPU (the query launches nothing); tests/test_bc_rows_gpu.py repeats it on the device"""
    lib = _cdll()
    if lib is None:
        pytest.skip("libttk_hip.so is not built here: tests/test_bc_rows_gpu.py holds the query")
    check_query(lib.ttk_bc_partial_rows_pw)


def check_query(query):
    ms = [1, 31, 32, 33, 255, 256, 257, 2049, 8193, 15872, 15873, 63488, 63489, 65536, 65537, R.E_BIG_M]
    for K in POW2:
        for N in POW2:
            for M in ms:
                p = R.expected_path("fwd", M, K, N)
                assert query(M, K, N) == (-1 if p is None else p.rows), (M, K, N)
    for bad in ((0, 32, 64), (5, 48, 64), (5, 32, 2048), (5, 16, 64)):
        assert query(*bad) == -1
    for cin, cout in R.REFUSED_FWD:
        assert R.expected_path("fwd", 5, cin, cout) is None
    for cin, cout in R.REFUSED_DGRAD:
        assert R.expected_path("dgrad", 5, cin, cout) is None


# ---------------------------------------------------------------------------------------------------------------------------------
# planted errors
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = [
    ("trunc_operand", ("fwd", 33, 32, 64)),
    ("trunc_operand", ("dgrad", 257, 128, 128)),
    ("trunc_weights", ("fwd", 257, 64, 128)),
    ("trunc_weights", ("dgrad", 257, 256, 256)),
    ("shift_plus_mean", ("fwd", 33, 128, 128)),
    ("gmean_mean_swapped", ("dgrad", 33, 32, 64)),
    ("drop_last_k16", ("fwd", 33, 32, 64)),
    ("drop_last_k16", ("dgrad", 257, 512, 512)),
    ("block_stride_64", ("fwd", 257, 128, 256)),
    ("tile_starts_late", ("fwd", 257, 256, 512)),
    ("mask_other_chunk", ("dgrad", 33, 64, 128)),
    ("mask_ge", ("dgrad", 257, 128, 256)),
]


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name,case", MUTATIONS, ids=[f"{n}-{_ids(c)}" for n, c in MUTATIONS])
def test_planted_error_is_far_outside(name, case, family):
    assert case in R.CASES
    c = R.pw_case(*case, family)
    v = R.model(c, name)
    judged = None if c.open is None else c.open | c.mask_undecided
    x, n = R.excess(c.p, v, judged), R.outside(c.p, v, c.open, c.mask_undecided)
    print(f"MUTATION {name} {_ids(case)} {family}: {n} of {v.size} elements outside, worst {x:.3g}x the allowed error")
    assert n > 0 and x > 10


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name,case", [("second_sum_beta", ("dgrad", 33, 32, 64)), ("second_sum_beta", ("dgrad", 257, 512, 512)),
                                       ("padding_counted", ("fwd", 33, 64, 128)), ("padding_counted", ("dgrad", 257, 256, 256))])
def test_planted_error_in_the_sums_is_far_outside(name, case, family):
    assert case in R.CASES
    c = R.pw_case(*case, family)
    v = R.model(c)
    d, q = R.stat_terms(c, v.astype(np.float64))
    x = R.stats_outside(R.model_part(c, v, name), c.rows_of, d, q, c.L)
    print(f"MUTATION {name} {_ids(case)} {family}: {x:.3g}x the bound")
    assert x > 10


# ---------------------------------------------------------------------------------------------------------------------------------
# pointwise weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
WG_SMALL = [c for c in R.WG_CASES if c[0] <= 4096]


def _wg_emulated(c, dw0=None, mutate=None, skip_row=None, D=None):
    tiles = R.wg_model(c.plan, c.D if D is None else D, c.A, c.M, mutate).reshape(c.plan.slices, -1)
    out = np.zeros(c.cin * c.cout, np.float32) if dw0 is None else dw0.reshape(-1)
    return R.fold(tiles, out, c.plan.fold == "fast", True, skip_row).reshape(c.cout, c.cin)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", R.WG_CASES, ids=R.wg_id)
def test_wgrad_reference_caps_and_emulation(case, family):
    c = R.wg_case(*case, family)
    ref = (_t(c.opD.v.astype(np.float64)).T @ _t(c.opA.v.astype(np.float64))).numpy()
    assert np.abs(ref - c.p.ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)
    und = max(float(c.opD.undecided.mean()), float(c.opA.undecided.mean()))
    print(f"CAPS wgrad {R.wg_id(case)} {family} (draw {c.salt}): undecided {und:.2e}, widened {c.p.widened_share:.2e}, Y chain {c.p.Y_chain:.2e} own {c.p.Y_own:.2e}, "
          f"slices {c.plan.slices} x {c.plan.rows}, fold {c.plan.fold}, lds {c.plan.lds}")
    if family == "short":
        assert und == 0 and c.p.widened_share == 0 and not c.opD.inexact.any() and not c.opA.inexact.any()
    else:
        assert und <= R.UNDECIDED_CAP and c.p.widened_share <= R.WG_WIDENED_CAP
    assert c.plan.lds <= R.LDS_LIMIT and (c.p.Y > 0 or c.M == 1)   # one pixel: a single exact product
    if case in WG_SMALL:
        assert R.wg_ratio(c.p, _wg_emulated(c))[0] <= 1.0
        assert R.wg_ratio(R.wg_onto(c.p, c.dw0), _wg_emulated(c, c.dw0))[0] <= 1.0


def test_wgrad_table_reaches_every_instantiation_and_seam():
    plans = {case: R.wgrad_plan(*case) for case in R.WG_CASES}
    assert {p.inst for p in plans.values()} == set(R.WG_INSTANCES.values()) and len(R.WG_INSTANCES) == 5
    for (TN, TK), inst in R.WG_INSTANCES.items():
        mine = {case[0]: p for case, p in plans.items() if p.inst == inst and case[1] == TK and case[2] == TN}
        CP = inst[2]
        assert set(mine) >= {1, CP - 1, CP, CP + 1, 2 * CP, 2 * CP + 1}
        assert mine[2 * CP].slices == 1 and mine[2 * CP + 1].slices == 2 and (2 * CP + 1) % mine[2 * CP + 1].rows == 1   # a last slice of one pixel
        assert {15, 16} <= {p.slices for p in mine.values()} and mine[30 * CP].fold == "wide" and mine[32 * CP].fold == "fast"
        assert any(p.slices == p.cap == 256 for p in mine.values())
    assert plans[(16321, 256, 256)].fold == "fast" and plans[(8129, 256, 512)].fold == "wide"      # n = 65 536 | 131 072
    assert plans[(1985, 512, 1024)].slices == 32 == 256 // plans[(1985, 512, 1024)].tiles
    assert plans[(961, 1024, 1024)].slices == 16 == 256 // plans[(961, 1024, 1024)].tiles
    assert all(R.wgrad_plan(5, cin, cout) is None for cin, cout in R.WG_REFUSED)


def check_wgrad_queries(slices, scratch_bytes):
    for cin in POW2:
        for cout in POW2:
            for M in (1, 31, 32, 33, 64, 65, 127, 128, 129, 256, 257, 960, 1024, 4096, 16321, 65281, 70000):
                p = R.wgrad_plan(M, cin, cout)
                assert slices(M, cin, cout) == (0 if p is None else p.slices), (M, cin, cout)
                assert scratch_bytes(M, cin, cout) == (0 if p is None else p.scratch_bytes), (M, cin, cout)


def test_wgrad_plan_is_the_query_of_the_library():
    lib = _cdll()
    if lib is None:
        pytest.skip("libttk_hip.so is not built here: tests/test_bc_rows_gpu.py holds the query")
    for f, res in ((lib.ttk_bc_pw_wgrad_slices, ctypes.c_int), (lib.ttk_bc_pw_wgrad_scratch_bytes, ctypes.c_size_t)):
        f.argtypes, f.restype = [ctypes.c_int64, ctypes.c_int, ctypes.c_int], res
    check_wgrad_queries(lib.ttk_bc_pw_wgrad_slices, lib.ttk_bc_pw_wgrad_scratch_bytes)


WG_MUTATIONS = [
    ("slice_starts_late", (257, 32, 64)),     # the second slice has one pixel: it is lost
    ("slice_starts_late", (960, 256, 256)),
    ("drop_last_k16", (129, 64, 128)),
    ("drop_last_k16", (65, 128, 256)),
    ("skip_fold_row", (4096, 32, 64)),        # fast fold
    ("skip_fold_row", (960, 128, 256)),       # wide fold
    ("trunc_operand", (128, 128, 128)),
    ("trunc_operand", (1024, 256, 256)),
]


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name,case", WG_MUTATIONS, ids=[f"{n}-{R.wg_id(c)}" for n, c in WG_MUTATIONS])
def test_wgrad_planted_error_is_far_outside(name, case, family):
    assert case in R.WG_CASES
    c = R.wg_case(*case, family)
    if name == "skip_fold_row":
        x = _wg_emulated(c, skip_row=c.plan.slices - 2)
    elif name == "trunc_operand":
        x = _wg_emulated(c, D=R.dy_operand(c.g, c.y, c.bn_pw, R.trunc_bf16).v.astype(np.float64).T)
    else:
        x = _wg_emulated(c, mutate=name)
    r = R.wg_ratio(c.p, x)[0]
    print(f"MUTATION wgrad {name} {R.wg_id(case)} {family}: {r:.3g}x the allowed error")
    assert r > 10


# ---------------------------------------------------------------------------------------------------------------------------------
# depthwise forward
# ---------------------------------------------------------------------------------------------------------------------------------
def check_dw_query(query):
    for backward in (0, 1):
        for C in (32, 64, 128, 1024):
            for stride in (1, 2):
                for B, H in ((1, 1), (3, 9), (7, 40), (40, 65)):
                    for W in (1, 9, 47, 48, 50, 52, 78, 79, 158, 159, 185, 256):
                        assert query(B, H, W, C, stride, backward) == R.dw_tiling(B, H, W, C, stride, bool(backward)).rows, (B, H, W, C, stride, backward)
    for B, H, W, C, stride in R.DW_REFUSED:
        assert not R.dw_shape_ok(B, H, W, C, stride) and query(B, H, W, C, stride, 0) == -1 and query(B, H, W, C, stride, 1) == -1


def test_dw_tiling_is_the_query_of_the_library():
    lib = _cdll()
    if lib is None:
        pytest.skip("libttk_hip.so is not built here: tests/test_bc_rows_gpu.py holds the query")
    lib.ttk_bc_partial_rows_dw.argtypes, lib.ttk_bc_partial_rows_dw.restype = [ctypes.c_int] * 6, ctypes.c_int
    check_dw_query(lib.ttk_bc_partial_rows_dw)


def test_dw_forward_table_reaches_every_instantiation_and_seam():
    T = {case: R.dw_tiling(*case[:5], False) for case in R.DW_FWD_CASES}
    inst = {(case[4], case[5], t.SL, t.carry) for case, t in T.items()}
    assert inst == {(s, k, sl, cy) for s in (1, 2) for k in (False, True) for sl in (32, 64) for cy in (False, True)}     # all sixteen
    tl = lambda W, C, s, H=11, B=2: R.dw_tiling(B, H, W, C, s, False)
    assert tl(78, 64, 1).carry and not tl(79, 64, 1).carry and tl(79, 64, 1).NCT == 5 and tl(78, 64, 1).NCT == 1      # 78 | 79
    assert tl(158, 64, 2).carry and not tl(159, 64, 2).carry and tl(158, 32, 1).carry and not tl(159, 32, 1).carry   # 158 | 159
    assert T[(1, 5, 256, 64, 1, True)].NCT == 16
    assert {H % 5 for (B, H, W, C, s, k), t in T.items() if W == 78 and t.R == 5} >= {4, 0, 1}                      # H around a multiple of R, carried
    full = lambda W, C, s: R.dw_tiling(1, 300, W, C, s, False).R                                                        # the band height a tall image gets
    col = {c[1] - full(c[2], c[3], c[4]) for c, t in T.items() if t.NCT > 1 and c[2] == 79 and c[3] == 64}
    assert col >= {-1, 0, 1, 30} and any(t.NCT > 1 and t.nbands == 2 for t in T.values()) and any(t.NCT > 1 and t.nbands == 3 for t in T.values())   # column tiles AND bands: R - 1 | R | R + 1 | 2 R + 1
    plain = [(c, t) for c, t in T.items() if not t.carry and t.NCT == 1 and t.nbands > 1]
    assert {t.nbands for c, t in plain} >= {2, 3, 4} and any(t.nbands == 1 and c[2] == 159 and c[4] == 2 for c, t in T.items())                      # plain bands: Ho = R | R + 1 | 2 R + 1 ...
    assert all(t.R == 1 for C in (32, 64) for s in (1, 2) for W in range(1, 257) for t in [R.dw_tiling(1, 300, W, C, s, False)]
               if not t.carry and t.NCT == 1 and t.nbands > 1)                                                          # ... at R = 1: the forward has no taller plain band
    clamp = [t for (B, H, W, C, s, k), t in T.items() if s == 2 and C == 64 and W >= 185]
    assert {c[2] for c in T if c[4] == 2 and c[3] == 64 and c[2] >= 185} >= {185, 256} and len(clamp) >= 4
    assert all(t.R == 1 and t.stage_rows == 3 and t.over_budget and t.lds <= R.LDS_LIMIT for t in clamp)             # over the pixel budget, inside 160 KB
    assert all(R.dw_tiling(1, 3, W, 64, 2, False).lds <= R.LDS_LIMIT for W in range(185, 257))
    assert not any(t.over_budget for c, t in T.items() if not (c[4] == 2 and c[3] == 64 and c[2] >= 185))
    assert {(c[1] % 2, c[2] % 2) for c in T if c[4] == 2} == {(0, 0), (0, 1), (1, 0), (1, 1)}                        # the stride-2 parities of (H, W)
    assert any(t.nbands == 1 and t.NI > 1 and c[0] % t.NI for c, t in T.items())
    assert any(t.tiles > t.rows for t in T.values()) and any(t.nslabs == 16 and t.rows == 32 for t in T.values())   # a workgroup walks; 16 slabs
    assert {c[3] for c in T} >= {32, 64, 128, 1024} and (1, 1, 1, 32, 1, False) in T


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", R.DW_FWD_CASES, ids=R.dw_id)
def test_dw_forward_reference_and_emulation(case, family):
    c = R.dw_case(*case, family)
    a = _t(c.a.v.astype(np.float64)).permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(a, _t(c.w.astype(np.float64)).reshape(c.C, 1, 3, 3), stride=c.stride, padding=1, groups=c.C).permute(0, 2, 3, 1).numpy()
    assert np.abs(ref - c.p.ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)
    n_bad, share = R.dw_fwd_outside(c, R.rne_bf16(c.acc))
    print(f"CAPS dw_fwd {R.dw_id(case)} {family}: bit for bit {share:.4f}, undecided a_in {c.a.undecided.mean():.2e}, Y {c.p.Y:.2e}")
    assert n_bad == 0 and share > 0.99
    assert c.a.undecided.mean() <= R.UNDECIDED_CAP and (family == "full" or not c.a.undecided.any())
    rows_of, depth = R.dw_row_of_output(c.t, c.B)
    assert rows_of.max() == c.t.rows - 1 and len(np.unique(rows_of)) == c.t.rows


DW_MUTATIONS = [("halo_wraps", (2, 11, 79, 64, 1, False)), ("swap_hw", (1, 7, 159, 64, 2, False)), ("skip_before_rounding", (5, 17, 17, 128, 1, True)),
                ("trunc_operand", (1, 11, 158, 32, 1, True))]


# (skip_before_rounding with the short constants: fma(sc, y, sh) is exact in float32 at these magnitudes, one rounding or two give the same
# a_in - the planted error has nothing to show there and runs with the full constants only)
DW_MUTATION_RUNS = [(n, c, f) for n, c in DW_MUTATIONS for f in R.FAMILIES if not (n == "skip_before_rounding" and f == "short")]


@pytest.mark.parametrize("name,case,family", DW_MUTATION_RUNS, ids=[f"{n}-{R.dw_id(c)}-{f}" for n, c, f in DW_MUTATION_RUNS])
def test_dw_forward_planted_error_is_far_outside(name, case, family):
    assert case in R.DW_FWD_CASES
    c = R.dw_case(*case, family)
    if name == "skip_before_rounding":
        # one bf16 step of a_in is mostly swallowed by the output's own bf16 rounding: what catches it is a_out == a_in bit for bit,
        # at the pixels the case plants for it (bc_ref._dw_case) - any difference there is outside by definition
        a = R.dw_a_in(c.y, c.bn, c.sk, name).v
        differ = (a != c.a.v) & ~c.a.undecided
        print(f"MUTATION dw_fwd {name} {R.dw_id(case)} {family}: {int(differ.sum())} elements of a_out differ from the emulated a_in ({c.planted} planted)")
        assert c.planted > 0 and differ.reshape(-1, c.C)[:c.planted, 0].all() and c.want_a
        return
    elif name == "trunc_operand":
        lo, _, _ = R.fma32(c.y, c.bn[BN_SCALE], R.shift_of(c.bn))
        lo, _, _ = R.add32(lo, c.sk)
        taps = R.dw_taps(R.relu(R.trunc_bf16(lo)).astype(np.float64), c.stride)
    else:
        taps = R.dw_taps(c.a.v.astype(np.float64), c.stride, name)
    v = R.rne_bf16(R.dw_chain(taps, c.w)[0])
    n_bad, _ = R.dw_fwd_outside(c, v)
    x = R.excess(c.p, v)
    print(f"MUTATION dw_fwd {name} {R.dw_id(case)} {family}: {n_bad} of {v.size} elements differ, worst {x:.3g}x the allowed error")
    assert n_bad > 0 and x > 10


@pytest.mark.parametrize("family", R.FAMILIES)
def test_relu_before_the_rounding_is_the_same_operand(family):
    """the issue's planted error `relu before the rounding of a value that rounds to -0 or +0`: relu and round-to-nearest commute (rounding
    keeps sign and zero, relu_pk turns -0 into +0), so the operand VALUES are the same and only the sign bit of a zero could differ -
    which a_out's bit-for-bit check on the device holds (+0 everywhere relu closed).  Asserted here as a no-op on values, with -0 present."""
    c = R.dw_case(5, 17, 17, 128, 1, True, family)
    m = R.dw_a_in(c.y, c.bn, c.sk, "relu_before_rounding")
    assert np.array_equal(m.v, c.a.v)
    assert (c.a.v.view(np.uint32)[c.a.v == 0] == 0).all()         # the reference's zeros are +0
    p = R.pw_case("fwd", 257, 64, 128, family)                     # the pointwise `a` operand: the same
    lo, _, _ = R.fma32(p.ydw, p.bn_dw[BN_SCALE], R.shift_of(p.bn_dw))
    assert np.array_equal(R.rne_bf16(np.maximum(lo, 0)) + np.float32(0), R.act_operand(p.ydw, p.bn_dw).lo)
    tiny = R.rne_bf16(np.float32([-1e-45, -0.0, 1e-45]))
    assert (R.relu(tiny).view(np.uint32) == 0).all() and np.signbit(tiny[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# depthwise backward
# ---------------------------------------------------------------------------------------------------------------------------------
def test_dw_backward_table_reaches_every_instantiation_and_seam():
    T = {case: R.dw_tiling(*case[:5], True) for case in R.DW_BWD_CASES}
    assert {(c[4], t.SL, c[5] == "lean") for c, t in T.items()} == {(s, sl, ln) for s in (1, 2) for sl in (32, 64) for ln in (False, True)}   # all eight
    assert T[(2, 9, 47, 64, 1, "lean")].NCT == 1 and T[(2, 9, 48, 64, 1, "lean")].NCT == 3                                # 47 | 48
    t50, t52 = T[(1, 9, 50, 64, 1, "skip")], T[(1, 9, 52, 64, 1, "lean")]
    assert 50 % t50.TW and 50 - (t50.NCT - 1) * t50.TW < t50.TW and t52.NCT * t52.TW == 52                               # a narrower last tile | an even split
    assert {(c[1] % 2, c[2] % 2) for c in T if c[4] == 2 and c[3] == 64} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c[4] == 2 and t.R % 2 for c, t in T.items())                                                              # an odd clamped R
    assert any(R.fold_fast_ok(t.rows, 9 * c[3]) for c, t in T.items()) and any(1 < t.rows < 16 for t in T.values()) and any(t.rows == 1 for t in T.values())
    assert any(t.tiles > t.rows for t in T.values()) and any(t.NI > 1 and c[0] % t.NI for c, t in T.items()) and any(t.nbands > 1 for t in T.values())
    full = lambda W, C, s: R.dw_tiling(1, 600, W, C, s, True).R
    for W, s, cols in ((48, 1, True), (47, 1, False), (94, 2, False)):                                                  # H = R - 1 | R | R + 1 | 2 R + 1 in column-tile and plain form
        got = {c[1] - full(W, 64, s) for c, t in T.items() if c[2] == W and c[3] == 64 and c[4] == s and (t.NCT > 1) == cols}
        assert got >= {-1, 0, 1, full(W, 64, s) + 1}, (W, s, got)
        assert {t.nbands for c, t in T.items() if c[2] == W and c[4] == s and (t.NCT > 1) == cols} >= {1, 2, 3}
    assert any(c[5] == "skip_in" and c[4] == 2 for c in T) and any(c[0] > 1 for c in T)
    assert {c[3] for c in T} >= {32, 64, 128, 1024} and all(t.lds <= R.LDS_LIMIT for t in T.values())


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", R.DW_BWD_CASES, ids=R.dwb_id)
def test_dw_backward_reference_and_emulation(case, family):
    c = R.dw_bwd_case(*case, family)
    dy = _t(c.dy.v.astype(np.float64).reshape(c.B, c.Ho, c.Wo, c.C)).permute(0, 3, 1, 2)
    w = _t(c.w.astype(np.float64)).reshape(c.C, 1, 3, 3)
    G = torch.nn.functional.conv_transpose2d(dy, w, stride=c.stride, padding=1, groups=c.C, output_padding=((c.H - 1) % c.stride, (c.W - 1) % c.stride))
    G = G.permute(0, 2, 3, 1).numpy() + (0 if c.sg is None else c.sg.astype(np.float64))
    assert np.abs(G - c.p.ref).max() <= 1e-12 * max(np.abs(G).max(), 1.0)
    a = _t(c.a.v.astype(np.float64)).permute(0, 3, 1, 2).reshape(1, c.B * c.C, c.H, c.W)
    dw = torch.nn.functional.conv2d(a, dy.reshape(c.B * c.C, 1, c.Ho, c.Wo), padding=1, dilation=c.stride, groups=c.B * c.C)[:, :, :3, :3].reshape(c.B, c.C, 9).sum(0).numpy()
    assert np.abs(dw - c.q.ref).max() <= 1e-12 * max(np.abs(dw).max(), 1.0)
    v = np.where(c.open, R.rne_bf16(c.acc), np.float32(0))
    n_bad, share = R.dw_bwd_outside(c, v)
    und = float(c.dy.undecided.mean())
    print(f"CAPS dw_bwd {R.dwb_id(case)} {family}: bit for bit {share:.4f}, undecided dy {und:.2e}, widened {(c.p.widen > 0).mean():.2e}, dW widened {(c.q.widen > 0).mean():.2e}")
    assert n_bad == 0 and share > 0.99
    assert und <= R.UNDECIDED_CAP and (c.p.widen > 0).mean() <= R.WIDENED_CAP and (family == "full" or und == 0)
    assert c.a.undecided.mean() <= R.UNDECIDED_CAP and (c.q.widen > 0).mean() <= R.WG_WIDENED_CAP and (family == "full" or not c.a.undecided.any())
    if c.B > 1:
        assert np.array_equal(v[0], v[-1])                           # the copied image
    # the fused weight gradient: workgroup rows summed in float32 and folded as the launch folds them meet the criterion; one row left out does not
    r_ok = R.wg_ratio(c.q, R.dw_wgrad_model(c))[0]
    assert r_ok <= 1.0, r_ok
    if c.t.rows > 1:
        r_bad = R.wg_ratio(c.q, R.dw_wgrad_model(c, skip_row=c.t.rows - 1))[0]
        print(f"MUTATION dw_bwd skip_fold_row {R.dwb_id(case)} {family}: {r_bad:.3g}x the allowed error (the emulation: {r_ok:.3f})")
        assert r_bad > 10
    rows_of, depth = R.dw_bwd_rows(c.t, c.B, c.H, c.W, c.stride)
    assert len(np.unique(rows_of)) == c.t.rows


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", [(2, 7, 10, 64, 2, "lean"), (2, 9, 5, 64, 2, "skip_in")], ids=R.dwb_id)
def test_dw_backward_parity_class_exchanged_is_far_outside(case, family):
    assert case in R.DW_BWD_CASES
    c = R.dw_bwd_case(*case, family)
    taps = R.dw_taps_t(c.dy.v.astype(np.float64).reshape(c.B, c.Ho, c.Wo, c.C), c.H, c.W, c.stride, "parity")
    v = np.where(c.open, R.rne_bf16(R.dw_chain(taps, c.w)[0]), np.float32(0))
    n_bad, _ = R.dw_bwd_outside(c, v)
    x = R.excess(c.p, v, c.open)
    print(f"MUTATION dw_bwd parity {R.dwb_id(case)} {family}: {n_bad} of {v.size} elements outside, worst {x:.3g}x the allowed error")
    assert n_bad > 0 and x > 10


def test_fused_table_reaches_every_instantiation_and_seam():
    plans = {case: R.fused_plan(*case) for case in R.FUSED_CASES}
    assert {p.inst for p in plans.values()} == set(R.FUSED_INSTANCES.values()) and len(R.FUSED_INSTANCES) == 3
    for (cin, cout), (_, _, CP) in R.FUSED_INSTANCES.items():
        mine = {case[0]: p for case, p in plans.items() if case[1:] == (cin, cout)}
        assert set(mine) >= {1, CP - 1, CP, CP + 1, 2 * CP, 2 * CP + 1}
        assert mine[2 * CP].slices == 1 and mine[2 * CP + 1].slices == 2 and (2 * CP + 1) % mine[2 * CP + 1].rows == 1
        assert {15, 16, 256} <= {p.slices for p in mine.values()} and mine[30 * CP].fold == "plain" and mine[32 * CP].fold == "fast"
        assert all(p.lds <= R.LDS_LIMIT for p in mine.values())
    assert all(R.fused_plan(5, cin, cout) is None for cin, cout in ((128, 256), (64, 64), (32, 32), (256, 256)))


def check_fused_queries(rows, scratch_bytes):
    for cin in POW2[:4]:
        for cout in POW2[:4]:
            for M in (1, 31, 32, 33, 64, 65, 127, 128, 129, 256, 257, 960, 1024, 4096, 16321, 65281, 70000):
                plan = R.fused_plan(M, cin, cout)
                assert rows(M, cin, cout) == (0 if plan is None else plan.slices), (M, cin, cout)
                assert scratch_bytes(M, cin, cout) == (0 if plan is None else plan.scratch_bytes), (M, cin, cout)


def test_fused_plan_is_the_query_of_the_library():
    lib = _cdll()
    if lib is None:
        pytest.skip("libttk_hip.so is not built here: tests/test_bc_rows_gpu.py holds the query")
    for f, res in ((lib.ttk_bc_pw_bwd_fused_rows, ctypes.c_int), (lib.ttk_bc_pw_bwd_fused_scratch_bytes, ctypes.c_size_t)):
        f.argtypes, f.restype = [ctypes.c_int64, ctypes.c_int, ctypes.c_int], res
    check_fused_queries(lib.ttk_bc_pw_bwd_fused_rows, lib.ttk_bc_pw_bwd_fused_scratch_bytes)
