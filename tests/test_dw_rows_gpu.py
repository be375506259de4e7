"""The fp32 depthwise 3x3 pair (csrc/dwconv_tiled.hip) through the C ABI, element by element against float64, at every tile form
(tests/dw_ref.py: the reference, the yardstick, the criterion and its derivation, the table of cases with the path each is there for;
tests/test_dw_ref.py: all of that without a GPU, and the mutations the criterion catches):
  * ttk_dwconv3x3_fwd / _fwd_rawskip: y, a_out, the statistics; part = NULL and pivot = NULL; raw residual == stored residual bit for bit;
  * ttk_dwconv3x3_bwd_data / _bwd_data_rawskip: g_prev, the statistics, TTK_AUX_GMAX from three starting values with the rest of bn_prev
    bitwise intact, the block input recomputed == materialised bit for bit, and the fused weight gradient in all its modes: atomics
    overwriting (mode 0 onto NaN) and accumulating (mode 1 onto a non-zero tensor), scratch rows folded in either mode, rows left unfolded
    (mode 2, dw untouched), dw = NULL (dw_partial untouched);
  * position independence: with every image a copy of the first, every image's y, a_out and g_prev are the same bits - each output
    element is one fixed 9-tap chain, so a band, image or column seam that leaks shows at the bit level;
  * refusals, nothing written: stride 3, C = 48 | 2048, W = 257, a_out or skip_grad at stride 2, the stride-2 forward wider than 163.
Every output - y, a_out, g_prev, part, dw, dw_partial, and the bn_prev block the backward writes one word of - lies between two NaN guard
bands, starts as NaN (an accumulated dw: its base) and the bands must be untouched; every row of `part` must be finite and the row
count is `expected_path(...).rows`; every call repeats bit for bit (the atomic weight gradient need not).

Each quantity prints `RATIO <quantity> <case> <value>`, value = worst |x - f64| / ((MARGIN Y + 2^-24) s) over its elements - the assertion
is value <= 1 - and the statistics `STAT <entry> <case> <sum> <second sum>`, the worst error over the derived bound (<= 1).  Worst per
quantity and tile form on the MI355X: profiles/dw_float64.txt."""
import functools
import types

import numpy as np
import pytest
import torch

import dw_ref as R
from test_conv_rows_gpu import Guard, _t, _bits

pytestmark = pytest.mark.gpu
_ids = lambda v: "x".join(map(str, v))
BOTH = [c for c in R.CASES if c not in R.FORWARD_ONLY]
AUX, GMAX = R.BN_AUX, R.AUX_GMAX


def _lib():
    import trackertraincode._hip as hip
    return hip, hip.lib(), hip.ptr


def _inputs(hip, L, p, c, rep=False):
    """the case's inputs on the device, activations as channel blocks; rep: every image a copy of the first"""
    one = (lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(a[:1], a.shape))) if rep else (lambda a: a)
    blk = lambda a: None if a is None else hip.to_blocks(_t(one(a)))
    d = types.SimpleNamespace(yprev=blk(c.yprev), x=blk(c.x), raw=blk(c.raw), w=_t(c.w.reshape(c.C, 1, 3, 3)), bn_prev=_t(c.bn_prev),
                              bn_skip=_t(c.bn_skip), bn_dw=_t(c.bn_dw), piv=_t(c.piv), g=blk(c.g), y=blk(c.y32), sg=blk(c.sg))
    d.bn_prev[AUX] = torch.arange(1, c.C + 1, device="cuda") * 0.25  # the words beside TTK_AUX_GMAX: anything but zero
    d.dw0 = _t(np.random.default_rng(R.case_seed(c.case) + 1).normal(0, 1, (c.C, 9)).astype(np.float32))
    if c.form == "raw":  # x = relu(bn_skip(raw)) as ttk_bn_act stores it: the operand of the stored form the raw form must equal
        x = torch.full(tuple(d.raw.shape), float("nan"), device="cuda")
        L.call("ttk_bn_act", p(d.raw), p(d.bn_skip), None, p(x), c.B * c.H * c.W, c.C)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(x).all())
        d.x = hip.to_blocks(x)
    return d


@functools.lru_cache(maxsize=2)
def _device(case):
    hip, L, p = _lib()
    c = R.make_case(case)
    return c, _inputs(hip, L, p, c)


def _geo(c):
    return c.B, c.H, c.W, c.C, c.stride


def _fwd(L, p, c, d, G, form=None, part=True, piv=True):
    form = form or c.form
    y = G.new(c.B, c.Ho, c.Wo, c.C)
    a = G.new(c.B, c.H, c.W, c.C) if c.want_a else None
    pt = G.new(L.partial_rows_dwconv(*_geo(c), False), 2, c.C) if part else None
    pv = p(d.piv) if piv else None
    if form == "raw":
        L.call("ttk_dwconv3x3_fwd_rawskip", p(d.yprev), p(d.bn_prev), p(d.raw), p(d.bn_skip), p(a), p(d.w), p(y), p(pt), pv, *_geo(c))
    else:
        L.call("ttk_dwconv3x3_fwd", p(d.yprev), p(d.bn_prev), p(d.x) if form == "stored" else None, p(a), p(d.w), p(y), p(pt), pv, *_geo(c), 0)
    G.check("dwconv3x3_fwd " + form)
    return y, a, pt


def _bwd(L, p, c, d, G, form=None, a_in=None, gmax0=0.0, part=True, dw="nan", mode=0, scratch=False):
    """one backward launch on fresh guarded buffers -> (g_prev, part, dw, dw_partial, bn_prev)"""
    form = form or c.form
    rows = L.partial_rows_dwconv(*_geo(c), True)
    bn = G.new(8, c.C)
    bn.copy_(d.bn_prev)
    bn[AUX, GMAX] = gmax0
    gp = G.new(c.B, c.H, c.W, c.C)
    pt = G.new(rows, 2, c.C) if part else None
    dwt = None
    if dw is not None:
        dwt = G.new(c.C, 9)
        if dw == "dw0":
            dwt.copy_(d.dw0)
    sc = G.new(rows, c.C, 9) if scratch else None
    head = (p(d.g), p(d.y), p(d.bn_dw), p(d.w), p(d.sg), p(d.yprev), p(bn))
    tail = (p(gp), p(pt), p(dwt), mode, p(sc), *_geo(c))
    if a_in is not None:
        L.call("ttk_dwconv3x3_bwd_data", *head, None, p(a_in), *tail, 0)
    elif form == "raw":
        L.call("ttk_dwconv3x3_bwd_data_rawskip", *head, p(d.raw), p(d.bn_skip), *tail)
    else:
        L.call("ttk_dwconv3x3_bwd_data", *head, p(d.x) if form == "stored" else None, None, *tail, 0)
    G.check("dwconv3x3_bwd_data " + form)
    return gp, pt, dwt, sc, bn


def _np(hip, t):
    """a channel-block tensor of the device as channels-last float64"""
    return hip.from_blocks(t).cpu().numpy().astype(np.float64)


class Verdicts:
    """collects the findings of one test so that one run shows all of them"""

    def __init__(self, case):
        self.case, self.bad = case, []

    def judge(self, name, q, out, masked=False):
        out = np.asarray(out, np.float64)
        if not np.isfinite(out).all():
            self.bad.append((name, "NaN left or written"))
            return
        r = R.masked_outside(q, out) if masked else q.outside(out)
        print("RATIO", name, _ids(self.case), f"{r:.3f}")
        if not r <= 1.0:
            self.bad.append((name, f"worst error {r:.3g} x the allowance (Y = {q.Y / R.U:.2f} U)"))

    def stats(self, name, part, v, d, square):
        ps = part.cpu().numpy().astype(np.float64)
        if not np.isfinite(ps).all():
            self.bad.append((name, "a row of part is not finite"))
            return
        r = R.stat_ratios(ps, v, d, square)
        print("STAT", name, _ids(self.case), f"{r[0]:.3f} {r[1]:.3f}")
        if not max(r) <= 1.0:
            self.bad.append((name, f"statistics {r[0]:.3g}, {r[1]:.3g} x the bound"))

    def same(self, name, a, b):
        if not torch.equal(_bits(a), _bits(b)):
            self.bad.append((name, "not bit for bit the same"))

    def done(self):
        assert not self.bad, (self.case, self.bad)


@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_dw_fwd_elements(case):
    hip, L, p = _lib()
    c, d = _device(case)
    V = Verdicts(case)
    qy, qa = R.forward(case)
    P = R.expected_path(*case[:5], False)
    assert L.partial_rows_dwconv(*_geo(c), False) == P.rows
    G = Guard()
    y, a, pt = _fwd(L, p, c, d, G)
    y64 = _np(hip, y)
    V.judge("y", qy, y64)
    if c.want_a:
        V.judge("a_out", qa, _np(hip, a))
    v = (y64 - c.piv.astype(np.float64)).reshape(-1, c.C)
    V.stats("fwd", pt, v, v, True)
    y2, a2, pt2 = _fwd(L, p, c, d, G)
    V.same("y again", y, y2)
    V.same("part again", pt, pt2)
    if c.want_a:
        V.same("a_out again", a, a2)
    y3, _, _ = _fwd(L, p, c, d, G, part=False)
    V.same("y with part = NULL", y, y3)
    y4, _, pt4 = _fwd(L, p, c, d, G, piv=False)
    V.same("y with pivot = NULL", y, y4)
    v0 = y64.reshape(-1, c.C)
    V.stats("fwd_pivot_null", pt4, v0, v0, True)
    if c.form == "raw":  # the stored form given the materialised x: the same bits
        ys, as_, pts = _fwd(L, p, c, d, G, form="stored")
        V.same("y raw == stored", y, ys)
        V.same("part raw == stored", pt, pts)
        if c.want_a:
            V.same("a_out raw == stored", a, as_)
    V.done()


@pytest.mark.parametrize("case", BOTH, ids=_ids)
def test_dw_bwd_elements(case):
    hip, L, p = _lib()
    c, d = _device(case)
    V = Verdicts(case)
    qg, qw = R.dgrad(case), R.wgrad(case)
    assert qg.share <= R.UNDECIDED_CAP
    P = R.expected_path(*case[:5], True)
    assert L.partial_rows_dwconv(*_geo(c), True) == P.rows
    G = Guard()
    bn0 = _bits(d.bn_prev).clone()

    def gmax_ok(name, bn, start, gp):
        want = max(np.float32(start), np.float32(gp.abs().max().item()))
        got = _bits(bn).clone()
        if got[AUX, GMAX].item() != int(np.float32(want).view(np.int32)):
            V.bad.append((name, f"TTK_AUX_GMAX {bn[AUX, GMAX].item()!r} from {start!r}, max |g_prev| {gp.abs().max().item()!r}"))
        got[AUX, GMAX] = bn0[AUX, GMAX]
        if not torch.equal(got, bn0):
            V.bad.append((name, "a word of bn_prev beside TTK_AUX_GMAX changed"))

    # 1. block input recomputed; atomics overwrite a NaN-filled dw; the slot starts at 0
    gp, pt, dw, _, bn = _bwd(L, p, c, d, G, dw="nan", mode=0)
    g64 = _np(hip, gp)
    V.judge("g_prev", qg, g64, masked=True)
    V.judge("dW_atomic_overwrite", qw, dw.cpu().numpy())
    v = g64.reshape(-1, c.C)
    V.stats("bwd", pt, v, (c.yprev.astype(np.float64) - c.bn_prev[R.BN_MEAN]).reshape(-1, c.C), False)
    top = float(gp.abs().max())
    gmax_ok("slot from 0", bn, 0.0, gp)
    # 2. atomics accumulate onto a non-zero dw
    gp2, pt2, dw2, _, _ = _bwd(L, p, c, d, G, dw="dw0", mode=1)
    V.same("g_prev again", gp, gp2)
    V.same("part again", pt, pt2)
    q_onto = qw.onto(d.dw0.cpu().numpy().astype(np.float64))
    V.judge("dW_atomic_accumulate", q_onto, dw2.cpu().numpy())
    # 3. / 4. scratch rows folded, overwriting and accumulating; each twice, bit for bit
    for name, base, mode, q in (("dW_scratch_overwrite", "nan", 0, qw), ("dW_scratch_accumulate", "dw0", 1, q_onto)):
        runs = [_bwd(L, p, c, d, G, dw=base, mode=mode, scratch=True) for _ in range(2)]
        V.same(name + " twice", runs[0][2], runs[1][2])
        V.same(name + " rows twice", runs[0][3], runs[1][3])
        V.same(name + " g_prev", gp, runs[0][0])
        V.judge(name, q, runs[0][2].cpu().numpy())
        if not bool(torch.isfinite(runs[0][3]).all()):
            V.bad.append((name, "a scratch row was not written"))
    # 5. rows left unfolded: dw stays as it was, the sum of the rows is the gradient; the slot starts at half the maximum
    gp5, _, dw5, rows5, bn5 = _bwd(L, p, c, d, G, dw="dw0", mode=2, scratch=True, gmax0=0.5 * top)
    V.same("mode 2 leaves dw", dw5, d.dw0)
    V.same("mode 2 g_prev", gp, gp5)
    V.judge("dW_rows_unfolded", qw, rows5.cpu().numpy().astype(np.float64).sum(0))
    gmax_ok("slot from half", bn5, 0.5 * top, gp5)
    # 6. dw = NULL: dw_partial untouched; part = NULL; the slot starts at twice the maximum and stays
    gp6, _, _, rows6, bn6 = _bwd(L, p, c, d, G, dw=None, mode=0, scratch=True, part=False, gmax0=2.0 * top)
    V.same("g_prev with dw = NULL, part = NULL", gp, gp6)
    if not bool(rows6.isnan().all()):
        V.bad.append(("dw = NULL", "dw_partial was written"))
    gmax_ok("slot from twice", bn6, 2.0 * top, gp6)
    # 7. the block input materialised by the forward kernel: the same arithmetic, the same bits (g_prev, statistics, weight-gradient rows)
    if c.want_a:
        _, a_out, _ = _fwd(L, p, c, d, G)
        gp7, pt7, _, rows7, _ = _bwd(L, p, c, d, G, a_in=a_out, dw="dw0", mode=2, scratch=True)
        V.same("g_prev materialised == recomputed", gp, gp7)
        V.same("part materialised == recomputed", pt, pt7)
        V.same("weight-gradient rows materialised == recomputed", rows5, rows7)
    # 8. the raw residual operand against the stored one
    if c.form == "raw":
        gp8, pt8, _, rows8, bn8 = _bwd(L, p, c, d, G, form="stored", dw="dw0", mode=2, scratch=True, gmax0=0.5 * top)
        V.same("g_prev raw == stored", gp, gp8)
        V.same("part raw == stored", pt, pt8)
        V.same("weight-gradient rows raw == stored", rows5, rows8)
        V.same("bn_prev raw == stored", bn5, bn8)
    V.done()


@pytest.mark.parametrize("case", R.POSITION_CASES, ids=_ids)
def test_dw_outputs_do_not_depend_on_the_image_position(case):
    hip, L, p = _lib()
    c = R.make_case(case)
    d = _inputs(hip, L, p, c, rep=True)
    assert R.expected_path(*case[:5], False).tiles > 1 and R.expected_path(*case[:5], True).tiles > 1
    G = Guard()
    y, a, _ = _fwd(L, p, c, d, G)
    gp = _bwd(L, p, c, d, G, dw=None)[0]
    for name, t in (("y", y), ("a_out", a), ("g_prev", gp)):
        if t is None:
            continue
        v = _bits(hip.from_blocks(t).contiguous())
        assert bool(torch.isfinite(t).all()), name
        diff = (v != v[:1]).flatten(1).any(1)
        assert not bool(diff.any()), (name, "images that differ from the first:", diff.nonzero().flatten().tolist())


def test_dw_refusals_write_nothing():
    """shapes and arguments outside the contract of include/ttk.h return -1 from the argument checks, before anything is launched"""
    hip, L, p = _lib()
    G = Guard()

    def bufs(B, H, W, C, s):
        Ho, Wo = R.out_hw(H, W, s)
        z = lambda *sh: torch.zeros(*sh, device="cuda")
        ins = types.SimpleNamespace(act=z(B, H, W, C), out=z(B, Ho, Wo, C), w=z(C, 9), bn=z(8, C))
        outs = types.SimpleNamespace(y=G.new(B, Ho, Wo, C), a=G.new(B, H, W, C), gp=G.new(B, H, W, C), part=G.new(8, 2, C), dw=G.new(C, 9))
        return ins, outs

    def fwd(i, o, geo, a_out=False):
        L.call("ttk_dwconv3x3_fwd", p(i.act), p(i.bn), None, p(o.a) if a_out else None, p(i.w), p(o.y), p(o.part), None, *geo, 0)

    def bwd(i, o, geo, sg=False):
        L.call("ttk_dwconv3x3_bwd_data", p(i.out), p(i.out), p(i.bn), p(i.w), p(i.act) if sg else None, p(i.act), p(i.bn), None, None, p(o.gp),
               p(o.part), p(o.dw), 0, None, *geo, 0)

    every = []
    # (shape the buffers are sized for, geometry passed): the buffers hold the larger of the two, were a refusal ever missing
    for size, geo in (((1, 4, 4, 32, 1), (1, 4, 4, 32, 3)), ((1, 4, 4, 64, 1), (1, 4, 4, 48, 1)), ((1, 2, 2, 2048, 1), (1, 2, 2, 2048, 1)),
                      ((1, 1, 257, 32, 1), (1, 1, 257, 32, 1))):
        assert L.partial_rows_dwconv(*geo, False) == -1 and L.partial_rows_dwconv(*geo, True) == -1
        i, o = bufs(*size)
        every.append(o)
        with pytest.raises(RuntimeError, match="dwconv3x3_fwd: unsupported shape"):
            fwd(i, o, geo)
        with pytest.raises(RuntimeError, match="dwconv3x3_bwd_data: unsupported shape"):
            bwd(i, o, geo)
    i, o = bufs(2, 6, 6, 32, 2)
    every.append(o)
    with pytest.raises(RuntimeError, match="a_out requires stride 1"):
        fwd(i, o, (2, 6, 6, 32, 2), a_out=True)
    with pytest.raises(RuntimeError, match="residual gradient requires stride 1"):
        bwd(i, o, (2, 6, 6, 32, 2), sg=True)
    # the stride-2 forward wider than 163: three staged rows exceed the 64 KiB of LDS of a workgroup.  The row query is asked FIRST - a
    # host function - so that a library without the refusal fails here and never launches the shape.
    assert L.partial_rows_dwconv(1, 3, 163, 32, 2, False) == 2
    for shape in R.OVERWIDE_FWD:
        assert not R.fwd_admitted(*shape)
        assert L.partial_rows_dwconv(*shape, False) == -1
        assert L.partial_rows_dwconv(*shape, True) == R.expected_path(*shape, True).rows  # the data gradient takes them
        i, o = bufs(*shape)
        every.append(o)
        with pytest.raises(RuntimeError, match="dwconv3x3_fwd: unsupported shape"):
            fwd(i, o, shape)
    G.check("refused depthwise calls")
    for o in every:
        assert all(bool(t.isnan().all()) for t in vars(o).values())
