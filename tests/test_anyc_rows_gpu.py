"""The any-channel-count kernel family (ttk_anyc_*: csrc/anyc_pw.hip, csrc/anyc_pix.hip) through the C ABI, element by element against
float64, off the square path (tests/anyc_ref.py: the reference, the yardsticks, the criterion, the derived statistics bound, the restated
host logic and the tables of cases with the feature each is there for; tests/test_anyc_ref.py: all of that without a GPU, and the ten
mutations the criterion catches).  Every entry point runs on every case that applies to it:
  * every output starts as NaN, lies between two bands of a sentinel value (64 floats before, 4096 after: a store through a block width of
    32 in a narrow block lands there) and the bands must be untouched - the partial-sum rows and the weight-gradient scratch included;
  * every element is judged by |x - f64| <= (MARGIN Y + 2^-24) s with exact zeros where s == 0, masked gradients under the undecided rule;
  * the statistics against the tensor AS STORED by the bound derived in anyc_ref's docstring; TTK_AUX_GMAX exactly, the rest of the
    BatchNorm block bitwise intact;
  * every call repeats bit for bit;
  * the weight-gradient fold exactly: the slice tiles / workgroup rows read back from the scratch and folded in numpy float32 in the order
    launch_fold_partials uses give `dw` bit for bit, overwriting and accumulating onto a random dw0;
  * ttk_anyc_partial_rows and the three *_wgrad_scratch_bytes equal their restatements; the tenth slice of 641 x 520 x 680 is a zero tile;
  * with every image a copy of the first, every image's depthwise outputs are the same bits;
  * at three shapes both families accept, the tuned entry point and the ttk_anyc_* one are judged by the same criterion on the same case.
Each quantity prints `RATIO <entry> <quantity> <case> <value>`, value = worst |x - f64| / ((MARGIN Y + 2^-24) s) - the assertion is
value <= 1 - and `STAT <entry> <case> <sum> <second sum>`, the worst error over the derived bound (<= 1).  Figures of the MI355X:
profiles/anyc_float64.txt."""
import functools
import types

import numpy as np
import pytest
import torch

import anyc_ref as R
import dw_ref

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENTINEL, FRONT, BACK = -24680.0, 64, 4096
_ids = lambda v: "x".join(map(str, v))
AUX, GMAX = R.BN_AUX, R.AUX_GMAX


def _lib():
    import trackertraincode._hip as hip
    return hip, hip.lib(), hip.ptr


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


class Bands:
    """output buffers of a test, NaN-filled, each with FRONT sentinel floats before it and BACK after its end"""

    def __init__(self):
        self.items = []

    def new(self, *shape, like=None):
        n = int(np.prod(shape))
        full = torch.full((FRONT + n + BACK,), SENTINEL, dtype=torch.float32, device="cuda")
        body = full[FRONT:FRONT + n]
        body.fill_(NAN)
        if like is not None:
            body.copy_(like.reshape(-1))
        self.items.append((full, n))
        return body.view(*shape)

    def check(self, what):
        torch.cuda.synchronize()
        for full, n in self.items:
            assert bool((full[:FRONT] == SENTINEL).all()) and bool((full[FRONT + n:] == SENTINEL).all()), \
                f"{what}: written outside a buffer of {n} floats"


class Verdicts:
    """collects the findings of one test so that one run shows all of them"""

    def __init__(self, case):
        self.case, self.bad = case, []

    def judge(self, name, q, out, masked=False):
        out = np.asarray(out, np.float64)
        if not np.isfinite(out).all():
            self.bad.append((name, "NaN left or written"))
            return
        r = R.outside(q, out.reshape(q.ref.shape), masked)
        print("RATIO", name, _ids(self.case), f"{r:.3f}")
        if not r <= 1.0:
            self.bad.append((name, f"worst error {r:.3g} x the allowance (Y = {q.Y / R.U:.2f} U)"))

    def stats(self, name, part, v, d, square, length):
        ps = part.cpu().numpy().astype(np.float64)
        if not np.isfinite(ps).all():
            self.bad.append((name, "a row of part is not finite"))
            return
        r = R.stat_ratios(ps, v, d, square, length)
        print("STAT", name, _ids(self.case), f"{r[0]:.3f} {r[1]:.3f}")
        if not max(r) <= 1.0:
            self.bad.append((name, f"statistics {r[0]:.3g}, {r[1]:.3g} x the bound"))

    def same(self, name, a, b):
        if not torch.equal(_bits(a), _bits(b)):
            self.bad.append((name, "not bit for bit the same"))

    def gmax(self, name, bn, bn0, out):
        """TTK_AUX_GMAX raised from 0 to max |out| exactly, nothing else of the block touched"""
        got, want = _bits(bn).clone(), _bits(bn0).clone()
        if got[AUX, GMAX].item() != int(_bits(out.abs().max().reshape(1)).item()):
            self.bad.append((name, f"TTK_AUX_GMAX {bn[AUX, GMAX].item()!r}, max |out| {out.abs().max().item()!r}"))
        got[AUX, GMAX] = want[AUX, GMAX]
        if not torch.equal(got, want):
            self.bad.append((name, "a word of the BatchNorm block beside TTK_AUX_GMAX changed"))

    def fold(self, name, scratch, rows, dw, base=None):
        """dw == the rows of the scratch folded as launch_fold_partials does, bit for bit"""
        part = scratch.cpu().numpy().reshape(rows, -1)
        if not np.isfinite(part).all():
            self.bad.append((name, "a row of the scratch was not written"))
            return
        want = R.fold(part, None if base is None else base.cpu().numpy())
        if not np.array_equal(want.view(np.int32), dw.cpu().numpy().reshape(-1).view(np.int32)):
            self.bad.append((name, f"dw is not the {R.fold_form(*part.shape)} fold of its {rows} scratch rows"))

    def done(self):
        assert not self.bad, (self.case, self.bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# pointwise
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _pw_dev(case):
    hip, L, p = _lib()
    c = R.pw_case(case)
    blk = lambda a: hip.to_blocks_any(_t(a))
    d = types.SimpleNamespace(ydw=blk(c.ydw), g=blk(c.g), y=blk(c.y32), w=_t(c.w), wt=_t(c.w.T), piv=_t(c.piv), bn_dw=_t(c.bn_dw), bn_pw=_t(c.bn))
    d.bn_dw[AUX, GMAX + 1:] = torch.arange(1, c.Cin - GMAX, device="cuda") * 0.25  # the words beside the two the family knows: not zero
    d.dw0 = _t(np.random.default_rng(sum(case) + 1).normal(0, 1, (c.Cout, c.Cin)).astype(np.float32))
    return c, d


def _pw_bn_unchanged(c, d, what):
    torch.cuda.synchronize()
    bn = _t(c.bn_dw)
    bn[AUX, GMAX + 1:] = d.bn_dw[AUX, GMAX + 1:]
    assert torch.equal(_bits(d.bn_dw), _bits(bn)) and torch.equal(_bits(d.bn_pw), _bits(_t(c.bn))), (what, "a BatchNorm block was written")


def _pw_fwd(case, tuned=False):
    hip, L, p = _lib()
    c, d = _pw_dev(case)
    V, q = Verdicts(case), R.pw_forward(case)
    rows = R.gemm_rows(c.M)
    assert L.partial_rows_gemm(c.M) == rows
    B = Bands()
    runs = []
    for _ in range(2):
        y, part = B.new(c.M, c.Cout), B.new(rows, 2, c.Cout)
        if tuned:
            L.call("ttk_pwconv1x1_fwd", p(d.ydw), p(d.bn_dw), p(d.w), p(y), p(part), p(d.piv), c.M, c.Cin, c.Cout, None, 0)
        else:
            L.call("ttk_anyc_pw_fwd", p(d.ydw), p(d.bn_dw), p(d.w), p(y), p(part), p(d.piv), c.M, c.Cin, c.Cout)
        runs.append((y, part))
    B.check("pw_fwd")
    (y, part), (y2, part2) = runs
    V.same("y again", y, y2)
    V.same("part again", part, part2)
    name = "pwconv1x1_fwd" if tuned else "anyc_pw_fwd"
    out = hip.from_blocks_any(y).cpu().numpy()
    V.judge(name + " y", q, out)
    if not tuned:
        v = (out - c.piv).astype(np.float32).astype(np.float64)  # y - pivot rounded once, as the kernel forms it
        V.stats(name, part, v, v, True, R.GEMM_STAT_LENGTH)
        y3 = B.new(c.M, c.Cout)
        L.call("ttk_anyc_pw_fwd", p(d.ydw), p(d.bn_dw), p(d.w), p(y3), None, None, c.M, c.Cin, c.Cout)
        B.check("pw_fwd, part = NULL")
        V.same("y with part = NULL", y, y3)
    _pw_bn_unchanged(c, d, name)
    V.done()


def _pw_bwd_data(case, tuned=False):
    hip, L, p = _lib()
    c, d = _pw_dev(case)
    V, q = Verdicts(case), R.pw_dgrad(case)
    assert q.share <= R.UNDECIDED_CAP
    rows = R.gemm_rows(c.M)
    B = Bands()
    runs = []
    for _ in range(2):
        g_dw, part, bn = B.new(c.M, c.Cin), B.new(rows, 2, c.Cin), B.new(8, c.Cin, like=d.bn_dw)
        if tuned:
            L.call("ttk_pwconv1x1_bwd_data", p(d.g), p(d.y), p(d.bn_pw), p(d.wt), p(d.ydw), p(bn), p(g_dw), p(part), c.M, c.Cin, c.Cout, None, 0)
        else:
            L.call("ttk_anyc_pw_bwd_data", p(d.g), p(d.y), p(d.bn_pw), p(d.w), p(d.ydw), p(bn), p(g_dw), p(part), c.M, c.Cin, c.Cout)
        runs.append((g_dw, part, bn))
    B.check("pw_bwd_data")
    (g_dw, part, bn), (g2, part2, bn2) = runs
    V.same("g_dw again", g_dw, g2)
    V.same("part again", part, part2)
    V.same("bn_dw again", bn, bn2)
    name = "pwconv1x1_bwd_data" if tuned else "anyc_pw_bwd_data"
    out = hip.from_blocks_any(g_dw).cpu().numpy()
    V.judge(name + " g_dw", q, out, masked=True)
    if np.isfinite(out).all() and not (np.all(out[:, c.closed_channel] == 0) and np.all(out[:, c.zero_channels] == 0)):
        V.bad.append((name, "the column of an always-closed channel is not exactly zero"))
    if not tuned:
        yc = (c.ydw - c.bn_dw[R.BN_MEAN]).astype(np.float32).astype(np.float64)
        V.stats(name, part, out.astype(np.float64), yc, False, R.GEMM_STAT_LENGTH)
        V.gmax(name, bn, d.bn_dw, g_dw)
    _pw_bn_unchanged(c, d, name)
    V.done()


@pytest.mark.parametrize("case", R.pw_cases_of("f"), ids=_ids)
def test_anyc_pw_fwd_elements(case):
    _pw_fwd(case)


@pytest.mark.parametrize("case", R.pw_cases_of("d"), ids=_ids)
def test_anyc_pw_bwd_data_elements(case):
    _pw_bwd_data(case)


@pytest.mark.parametrize("case", R.pw_cases_of("w"), ids=_ids)
def test_anyc_pw_bwd_weight_elements_and_fold(case):
    hip, L, p = _lib()
    c, d = _pw_dev(case)
    V, q = Verdicts(case), R.pw_wgrad(case)
    slices, n = R.wgrad_slices(*case), c.Cin * c.Cout
    assert L.anyc_wgrad_scratch_bytes("pw", *case) == 4 * slices * n
    if case in R.PW_SLICE_PLANS:
        assert (slices, R.rows_per(*case)) == R.PW_SLICE_PLANS[case]
    B = Bands()

    def run(accumulate):
        scratch = B.new(slices, n)
        dw = B.new(c.Cout, c.Cin, like=d.dw0 if accumulate else None)
        L.call("ttk_anyc_pw_bwd_weight", p(d.g), p(d.y), p(d.bn_pw), p(d.ydw), p(d.bn_dw), p(dw), accumulate, p(scratch), c.M, c.Cin, c.Cout)
        return dw, scratch

    (dw, sc), (dw_b, sc_b) = run(0), run(0)
    (acc, sc_c), (acc_b, _) = run(1), run(1)
    B.check("pw_bwd_weight")
    V.same("dw again", dw, dw_b)
    V.same("scratch again", sc, sc_b)
    V.same("scratch of the accumulating call", sc, sc_c)
    V.same("accumulated dw again", acc, acc_b)
    V.judge("anyc_pw_bwd_weight dw", q, dw.cpu().numpy())
    V.judge("anyc_pw_bwd_weight dw0+dw", R.onto(q, d.dw0.cpu().numpy().astype(np.float64)), acc.cpu().numpy())
    if not bool((dw[:, c.zero_channels] == 0).all()):
        V.bad.append(("dw", "the column of a zero-operand channel is not exactly zero"))
    V.fold("dw", sc, slices, dw)
    V.fold("dw0+dw", sc_c, slices, acc, d.dw0)
    for s, (mb, me) in enumerate(R.slice_plan(*case)):
        if me <= mb and not bool((_bits(sc[s]) == 0).all()):
            V.bad.append(("scratch", f"slice {s} starts past M and is not a tile of zeros"))
    if case == R.EMPTY_SLICE_CASE:
        assert R.slice_plan(*case)[9] == (648, 641) and slices == 10
    _pw_bn_unchanged(c, d, "anyc_pw_bwd_weight")
    V.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# depthwise
# ---------------------------------------------------------------------------------------------------------------------------------
def _dw_inputs(hip, c, rep=False):
    one = (lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(a[:1], a.shape))) if rep else (lambda a: a)
    blk = lambda a: None if a is None else hip.to_blocks_any(_t(one(a)))
    d = types.SimpleNamespace(yprev=blk(c.yprev), x=blk(c.x), w=_t(c.w), bn_prev=_t(c.bn_prev), bn_dw=_t(c.bn_dw), piv=_t(c.piv), g=blk(c.g),
                              y=blk(c.y32), sg=blk(c.sg))
    d.bn_prev[AUX, GMAX + 1:] = torch.arange(1, c.C - GMAX, device="cuda") * 0.25
    d.dw0 = _t(np.random.default_rng(dw_ref.case_seed(c.case) + 1).normal(0, 1, (c.C, 9)).astype(np.float32))
    return d


@functools.lru_cache(maxsize=2)
def _dw_dev(case):
    hip, L, p = _lib()
    c = R.dw_case(case)
    return c, _dw_inputs(hip, c)


def _geo(c):
    return c.B, c.H, c.W, c.C, c.stride


def _dw_fwd(L, p, c, d, B, tuned=False, part=True, piv=True, want_a=None):
    want_a = c.want_a if want_a is None else want_a
    y = B.new(c.B, c.Ho, c.Wo, c.C)
    a = B.new(c.B, c.H, c.W, c.C) if want_a else None
    rows = L.partial_rows_dwconv(*_geo(c), False) if tuned else R.pix_rows(c.B * c.Ho * c.Wo)
    pt = B.new(rows, 2, c.C) if part else None
    args = (p(d.yprev), p(d.bn_prev), p(d.x), p(a), p(d.w), p(y), p(pt), p(d.piv) if piv else None, *_geo(c))
    if tuned:
        L.call("ttk_dwconv3x3_fwd", *args, 0)
    else:
        L.call("ttk_anyc_dw_fwd", *args)
    return y, a, pt


def _dw_bwd(L, p, c, d, B, tuned=False, a_in=None, wgrad=True, accumulate=0):
    """one backward launch on fresh banded buffers -> (g_prev, part, dw, scratch, bn_prev)"""
    pixels = c.B * c.H * c.W
    rows = L.partial_rows_dwconv(*_geo(c), True) if tuned else R.pix_rows(pixels)
    bn = B.new(8, c.C, like=d.bn_prev)
    gp, pt = B.new(c.B, c.H, c.W, c.C), B.new(rows, 2, c.C)
    dw = sc = None
    if wgrad:
        dw = B.new(c.C, 9, like=d.dw0 if accumulate else None)
        sc = None if tuned else B.new(rows, c.C * 9)
    args = (p(d.g), p(d.y), p(d.bn_dw), p(d.w), p(d.sg), p(d.yprev), p(bn), p(d.x) if a_in is None else None, p(a_in), p(gp), p(pt), p(dw),
            accumulate, p(sc), *_geo(c))
    if tuned:
        L.call("ttk_dwconv3x3_bwd_data", *args, 0)
    else:
        L.call("ttk_anyc_dw_bwd_data", *args)
    return gp, pt, dw, sc, bn


@pytest.mark.parametrize("case", R.DW_CASES, ids=_ids)
def test_anyc_dw_fwd_elements(case):
    hip, L, p = _lib()
    c, d = _dw_dev(case)
    V = Verdicts(case)
    qy, qa = R.dw_forward(case)
    pixels = c.B * c.Ho * c.Wo
    assert L.anyc_partial_rows(pixels) == R.pix_rows(pixels)
    B = Bands()
    y, a, pt = _dw_fwd(L, p, c, d, B)
    y2, a2, pt2 = _dw_fwd(L, p, c, d, B)
    y3, _, _ = _dw_fwd(L, p, c, d, B, part=False)
    y4, _, pt4 = _dw_fwd(L, p, c, d, B, piv=False)
    y5, _, pt5 = _dw_fwd(L, p, c, d, B, want_a=False)
    B.check("anyc_dw_fwd")
    np64 = lambda t: hip.from_blocks_any(t).cpu().numpy().astype(np.float64)
    y64 = np64(y)
    V.judge("anyc_dw_fwd y", qy, y64)
    if c.want_a:
        V.judge("anyc_dw_fwd a_out", qa, np64(a))
        V.same("a_out again", a, a2)
    length = R.pix_stat_length(pixels)
    v = (y64.astype(np.float32) - c.piv).astype(np.float64).reshape(-1, c.C)  # y - pivot rounded once (float32), as the kernel forms it
    V.stats("anyc_dw_fwd", pt, v, v, True, length)
    v0 = y64.reshape(-1, c.C)
    V.stats("anyc_dw_fwd_pivot_null", pt4, v0, v0, True, length)
    V.same("y again", y, y2)
    V.same("part again", pt, pt2)
    V.same("y with part = NULL", y, y3)
    V.same("y with pivot = NULL", y, y4)
    V.same("y without a_out", y, y5)
    V.same("part without a_out", pt, pt5)
    V.done()


@pytest.mark.parametrize("case", R.DW_CASES, ids=_ids)
def test_anyc_dw_bwd_elements_and_fold(case):
    hip, L, p = _lib()
    c, d = _dw_dev(case)
    V = Verdicts(case)
    qg, qw = R.dw_dgrad(case), R.dw_wgrad(case)
    assert qg.share <= R.UNDECIDED_CAP
    pixels = c.B * c.H * c.W
    rows = R.pix_rows(pixels)
    assert L.anyc_partial_rows(pixels) == rows and L.anyc_wgrad_scratch_bytes("dw", c.B, c.H, c.W, c.C) == 4 * rows * 9 * c.C
    B = Bands()
    gp, pt, dw, sc, bn = _dw_bwd(L, p, c, d, B)
    gp2, pt2, dw2, sc2, bn2 = _dw_bwd(L, p, c, d, B)
    gp3, pt3, acc, sc3, _ = _dw_bwd(L, p, c, d, B, accumulate=1)
    gp4, pt4, _, _, bn4 = _dw_bwd(L, p, c, d, B, wgrad=False)
    B.check("anyc_dw_bwd_data")
    g64 = hip.from_blocks_any(gp).cpu().numpy().astype(np.float64)
    V.judge("anyc_dw_bwd_data g_prev", qg, g64, masked=True)
    V.judge("anyc_dw_bwd_data dW", qw, dw.cpu().numpy())
    V.judge("anyc_dw_bwd_data dW0+dW", qw.onto(d.dw0.cpu().numpy().astype(np.float64)), acc.cpu().numpy())
    yc = (c.yprev - c.bn_prev[R.BN_MEAN]).astype(np.float32).astype(np.float64).reshape(-1, c.C)
    V.stats("anyc_dw_bwd_data", pt, g64.reshape(-1, c.C), yc, False, R.pix_stat_length(pixels))
    V.gmax("anyc_dw_bwd_data", bn, d.bn_prev, gp)
    for name, a, b in (("g_prev", gp, gp2), ("part", pt, pt2), ("dW", dw, dw2), ("scratch", sc, sc2), ("bn_prev", bn, bn2)):
        V.same(name + " again", a, b)
    V.same("g_prev of the accumulating call", gp, gp3)
    V.same("scratch of the accumulating call", sc, sc3)
    V.same("g_prev without the weight gradient", gp, gp4)
    V.same("part without the weight gradient", pt, pt4)
    V.same("bn_prev without the weight gradient", bn, bn4)
    V.fold("dW", sc, rows, dw)
    V.fold("dW0+dW", sc3, rows, acc, d.dw0)
    if c.want_a:  # the block input materialised by the forward kernel: the same arithmetic, the same bits
        _, a_out, _ = _dw_fwd(L, p, c, d, B)
        gp5, pt5, dw5, sc5, bn5 = _dw_bwd(L, p, c, d, B, a_in=a_out)
        B.check("anyc_dw_bwd_data with a_in")
        for name, a, b in (("g_prev", gp, gp5), ("part", pt, pt5), ("dW", dw, dw5), ("scratch", sc, sc5), ("bn_prev", bn, bn5)):
            V.same(name + " materialised == recomputed", a, b)
    V.done()


@pytest.mark.parametrize("case", R.DW_POSITION_CASES, ids=_ids)
def test_anyc_dw_outputs_do_not_depend_on_the_image_position(case):
    hip, L, p = _lib()
    c = R.dw_case(case)
    d = _dw_inputs(hip, c, rep=True)
    B = Bands()
    y, a, _ = _dw_fwd(L, p, c, d, B)
    gp = _dw_bwd(L, p, c, d, B, wgrad=False)[0]
    B.check("position")
    for name, t in (("y", y), ("a_out", a), ("g_prev", gp)):
        if t is None:
            continue
        assert bool(torch.isfinite(t).all()), name
        v = _bits(hip.from_blocks_any(t).contiguous())
        diff = (v != v[:1]).flatten(1).any(1)
        assert not bool(diff.any()), (name, "images that differ from the first:", diff.nonzero().flatten().tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# stem
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.STEM_CASES, ids=_ids)
def test_anyc_stem_elements_and_fold(case):
    hip, L, p = _lib()
    c = R.stem_case(case)
    V = Verdicts(case)
    rows = R.pix_rows(c.M)
    assert L.anyc_partial_rows(c.M) == rows and L.anyc_wgrad_scratch_bytes("stem", *case) == 4 * rows * 25 * c.C
    x, w, piv, bn = _t(c.x), _t(c.w), _t(c.piv), _t(c.bn)
    g, ygiven = hip.to_blocks_any(_t(c.g)), hip.to_blocks_any(_t(c.y32))
    dw0 = _t(np.random.default_rng(sum(case)).normal(0, 1, (c.C, 25)).astype(np.float32))
    B = Bands()
    fw = []
    for _ in range(2):
        y, part = B.new(c.M, c.C), B.new(rows, 2, c.C)
        L.call("ttk_anyc_stem_fwd", p(x), p(w), p(y), p(part), p(piv), c.B, c.H, c.W, c.C)
        fw.append((y, part))
    y3 = B.new(c.M, c.C)
    L.call("ttk_anyc_stem_fwd", p(x), p(w), p(y3), None, None, c.B, c.H, c.W, c.C)

    def wgrad(accumulate):
        sc, dw = B.new(rows, c.C * 25), B.new(c.C, 25, like=dw0 if accumulate else None)
        L.call("ttk_anyc_stem_bwd_weight", p(g), p(ygiven), p(bn), p(x), p(dw), accumulate, p(sc), c.B, c.H, c.W, c.C)
        return dw, sc

    (dw, sc), (dw2, sc2), (acc, sc3) = wgrad(0), wgrad(0), wgrad(1)
    B.check("anyc_stem")
    (y, part), (y2, part2) = fw
    out = hip.from_blocks_any(y).cpu().numpy()
    V.judge("anyc_stem_fwd y", c.fwd, out)
    v = (out - c.piv).astype(np.float32).astype(np.float64)
    V.stats("anyc_stem_fwd", part, v, v, True, R.pix_stat_length(c.M))
    V.same("y again", y, y2)
    V.same("part again", part, part2)
    V.same("y with part = NULL", y, y3)
    V.judge("anyc_stem_bwd_weight dW", c.wgrad, dw.cpu().numpy())
    V.judge("anyc_stem_bwd_weight dW0+dW", c.wgrad.onto(dw0.cpu().numpy().astype(np.float64)), acc.cpu().numpy())
    V.same("dW again", dw, dw2)
    V.same("scratch again", sc, sc2)
    V.same("scratch of the accumulating call", sc, sc3)
    V.fold("dW", sc, rows, dw)
    V.fold("dW0+dW", sc3, rows, acc, dw0)
    assert torch.equal(_bits(bn), _bits(_t(c.bn)))
    V.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# global average pool and bn_act
# ---------------------------------------------------------------------------------------------------------------------------------
def _pool(case, tuned=False):
    hip, L, p = _lib()
    c = R.pool_case(case)
    V = Verdicts(case)
    blk = lambda a: None if a is None else hip.to_blocks_any(_t(a))
    y, skip, bn0, gfeat = blk(c.y), blk(c.skip), _t(c.bn), _t(c.gfeat)
    bn0[AUX, GMAX + 1:] = torch.arange(1, c.C - GMAX, device="cuda") * 0.25
    tail = (0,) if tuned else ()
    pre = "ttk_" if tuned else "ttk_anyc_"
    tag = pre[4:]
    assert R.grid_1d(c.B * (c.C // 4)) == min(-(-c.B * (c.C // 4) // 256), 4096)
    B = Bands()
    fw = []
    for _ in range(2):
        feat, act = B.new(c.B, c.C), B.new(c.B, c.HW, c.C)
        L.call(pre + "avgpool_fwd", p(y), p(bn0), p(skip), p(feat), c.B, c.HW, c.C, *tail)
        L.call(pre + "bn_act", p(y), p(bn0), p(skip), p(act), c.M, c.C)
        fw.append((feat, act))
    B.check("avgpool_fwd, bn_act")
    V.judge(tag + "avgpool_fwd feat", c.feat, fw[0][0].cpu().numpy())
    V.judge(tag + "bn_act a", c.act, fw[0][1].cpu().numpy())  # plain channels-last rows
    V.same("feat again", fw[0][0], fw[1][0])
    V.same("act again", fw[0][1], fw[1][1])
    if case not in R.POOL_FWD_ONLY:
        rows = L.partial_rows_elementwise(c.M * (c.C // 4)) if tuned else R.pix_rows(c.M)
        if not tuned:
            assert L.anyc_partial_rows(c.M) == rows
        bw = []
        for _ in range(2):
            g, part, bn = B.new(c.B, c.HW, c.C), B.new(rows, 2, c.C), B.new(8, c.C, like=bn0)
            L.call(pre + "avgpool_bwd", p(gfeat), p(y), p(bn), p(skip), p(g), p(part), c.B, c.HW, c.C, *tail)
            bw.append((g, part, bn))
        B.check("avgpool_bwd")
        (g, part, bn), (g2, part2, bn2) = bw
        g64 = hip.from_blocks_any(g).cpu().numpy().astype(np.float64)
        V.judge(tag + "avgpool_bwd g", c.gin, g64, masked=True)
        V.gmax(tag + "avgpool_bwd", bn, bn0, g)
        if not tuned:
            yc = (c.y - c.bn[R.BN_MEAN]).astype(np.float32).astype(np.float64).reshape(-1, c.C)
            V.stats(tag + "avgpool_bwd", part, g64.reshape(-1, c.C), yc, False, R.pix_stat_length(c.M))
        for name, a, b in (("g", g, g2), ("part", part, part2), ("bn", bn, bn2)):
            V.same(name + " again", a, b)
    V.done()


@pytest.mark.parametrize("case", R.POOL_CASES, ids=_ids)
def test_anyc_pool_and_bn_act_elements(case):
    _pool(case)


# ---------------------------------------------------------------------------------------------------------------------------------
# the two families side by side: same contracts, same layout, neighbours in one chain (csrc/anyc_common.h)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuned", [False, True], ids=["anyc", "tuned"])
def test_both_families_meet_the_criterion_pointwise(tuned):
    hip, L, p = _lib()
    case = R.SIDE_PW
    _pw_fwd(case, tuned)
    _pw_bwd_data(case, tuned)
    c, d = _pw_dev(case)
    V, B = Verdicts(case), Bands()
    dw = B.new(c.Cout, c.Cin)
    if tuned:  # wsplit does not exist for the weight gradient: the atomic form onto a zeroed dw
        dw.zero_()
        L.call("ttk_pwconv1x1_bwd_weight", p(d.g), p(d.y), p(d.bn_pw), p(d.ydw), p(d.bn_dw), p(dw), None, c.M, c.Cin, c.Cout, 0)
    else:
        sc = B.new(R.wgrad_slices(*case), c.Cin * c.Cout)
        L.call("ttk_anyc_pw_bwd_weight", p(d.g), p(d.y), p(d.bn_pw), p(d.ydw), p(d.bn_dw), p(dw), 0, p(sc), c.M, c.Cin, c.Cout)
    B.check("pw_bwd_weight")
    V.judge(("pwconv1x1" if tuned else "anyc_pw") + "_bwd_weight dw", R.pw_wgrad(case), dw.cpu().numpy())
    V.done()


@pytest.mark.parametrize("tuned", [False, True], ids=["anyc", "tuned"])
def test_both_families_meet_the_criterion_depthwise(tuned):
    hip, L, p = _lib()
    case = R.SIDE_DW
    c, d = _dw_dev(case)
    V, B = Verdicts(case), Bands()
    y, _, _ = _dw_fwd(L, p, c, d, B, tuned)
    gp, _, dw, _, _ = _dw_bwd(L, p, c, d, B, tuned)
    B.check("depthwise")
    name = "dwconv3x3" if tuned else "anyc_dw"
    np64 = lambda t: hip.from_blocks_any(t).cpu().numpy().astype(np.float64)
    V.judge(name + "_fwd y", R.dw_forward(case)[0], np64(y))
    V.judge(name + "_bwd_data g_prev", R.dw_dgrad(case), np64(gp), masked=True)
    V.judge(name + "_bwd_data dW", R.dw_wgrad(case), dw.cpu().numpy())
    V.done()


@pytest.mark.parametrize("tuned", [False, True], ids=["anyc", "tuned"])
def test_both_families_meet_the_criterion_pool(tuned):
    _pool(R.SIDE_POOL, tuned)
