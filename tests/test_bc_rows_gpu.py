"""The kernels of the bf16-COMPUTE path (csrc/bc_gemm.hip, bc_wgrad.hip, bc_fused.hip, bc_dw.hip) through the C ABI against tests/bc_ref.py, element by element: every
stored bf16 value inside the bracket rne(f64 -+ allowed) of the float64 contraction of the kernel's own bf16 operands (allowed = (4 Y +
2^-24) s + the widening of undecided operands; the data gradient under its mask with the undecided band), every row of `part` against the
sums of the values as stored within the bound counted from the summation, at every instantiation of bc_gemm_e_k / bc_gemm_l_k and every
seam of e_grid / l_plan (bc_ref.CASES; tests/test_bc_ref.py asserts what the table reaches), for both constant families.

Every call: outputs start as NaN between two bands of TAIL sentinel elements that must stay as they were; a second call repeats the
bits; the last pixel is a copy of the first and its output row repeats the bits; refusals leave every output untouched.  No element is
left out of a comparison.
Weight gradient (test_pointwise_weight_gradient): every element of dW within (4 Y + 2^-24) (s + |dw0|) + widening of the float64 contraction,
into zeros, onto a random dw0 and with dw = NULL + ttk_bc_bn_bwd_finalize_fold, the scratch NaN-filled beforehand - and the slice tiles of
the scratch, folded in numpy in the plan's order (bc_ref.fold), give dW bit for bit.
Fused backward: the data gradient bitwise ttk_bc_pw_bwd_data's and inside the criterion, `part` per slice, dW as above.  Depthwise: the
forward's stored values and a_out bit for bit against the nine-fma emulation wherever it is exact (the bracket elsewhere), the data
gradient likewise under its mask, dW in every mode (rows folded, rows left for ttk_bc_bn_bwd_finalize_fold, atomics) - the atomic
modes to the criterion only.  Inputs: the first of up to 32 seeded draws per case whose operands meet the caps (bc_ref.SALTS), printed
as `draw N`.  Each test prints its worst ratio (`BC` lines of a run with -s; on the MI355X: profiles/bc_float64.txt)."""
import numpy as np
import pytest
import torch

import bc_ref as R
from test_bc_ref import check_query, check_wgrad_queries

pytestmark = pytest.mark.gpu

SENT_BF16 = 0x4B1D     # a finite bf16 pattern no kernel writes by accident
SENT_F32 = 12345.0
NAN_BF16 = 0x7FC0


def _hip():
    import trackertraincode._hip as hip
    return hip, hip.lib(), hip.ptr


class Guarded:
    """an output of n elements, NaN, between two bands of TAIL sentinels"""

    def __init__(self, n, bf16):
        self.n, self.bf16 = n, bf16
        if bf16:
            self.buf = torch.full((n + 2 * R.TAIL,), SENT_BF16, dtype=torch.int16, device="cuda")
            self.buf[R.TAIL:R.TAIL + n] = NAN_BF16
        else:
            self.buf = torch.full((n + 2 * R.TAIL,), SENT_F32, dtype=torch.float32, device="cuda")
            self.buf[R.TAIL:R.TAIL + n] = float("nan")
        self.body = self.buf[R.TAIL:R.TAIL + n]
        self.before = self.buf.clone()

    def bands_intact(self):
        a, b = self.buf.view(torch.int16 if self.bf16 else torch.int32), self.before.view(torch.int16 if self.bf16 else torch.int32)
        return bool(torch.equal(a[:R.TAIL], b[:R.TAIL]) and torch.equal(a[R.TAIL + self.n:], b[R.TAIL + self.n:]))

    def untouched(self):
        return bool(torch.equal(self.buf.view(torch.int16 if self.bf16 else torch.int32), self.before.view(torch.int16 if self.bf16 else torch.int32)))

    def bits(self):
        return self.body.cpu().numpy().view(np.uint16 if self.bf16 else np.uint32).copy()


def _bf16_dev(x):
    """x[M][C] (bf16 values as float32) -> the device tensor in storage order"""
    return torch.from_numpy(R.bf16_bits(R.to_blocks(x)).view(np.int16)).cuda()


def _f32_dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def _prepare(L, p, w):
    cout, cin = w.shape
    prep = torch.zeros(L.cdll.ttk_bc_prepared_bytes(cin, cout), dtype=torch.uint8, device="cuda")
    L.bc_prepare_weights([_f32_dev(w).view(cout, cin, 1, 1)], [prep])
    return prep


def _launch(L, p, c, d, out, part):
    if c.mode == "fwd":
        L.call("ttk_bc_pw_fwd", p(d["ydw"]), p(d["bn_dw"]), p(d["prep"]), p(out), p(part), p(d["piv"]), c.M, c.cin, c.cout)
    else:
        L.call("ttk_bc_pw_bwd_data", p(d["g"]), p(d["y"]), p(d["bn_pw"]), p(d["prep"]), p(d["ydw"]), p(d["bn_dw"]), p(out), p(part), c.M, c.cin, c.cout)


def _inputs(L, p, c):
    d = dict(ydw=_bf16_dev(c.ydw), bn_dw=_f32_dev(c.bn_dw), bn_pw=_f32_dev(c.bn_pw), piv=_f32_dev(c.piv), prep=_prepare(L, p, c.w))
    if c.mode == "dgrad":
        d.update(g=_bf16_dev(c.g), y=_bf16_dev(c.y))
    return d


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_pointwise_rows(case, family):
    hip, L, p = _hip()
    c = R.pw_case(*case, family)
    rows = L.cdll.ttk_bc_partial_rows_pw(c.M, c.K, c.N)
    assert rows == c.path.rows and c.path.lds <= R.LDS_LIMIT
    d = _inputs(L, p, c)
    runs = []
    for _ in range(2):
        out, part = Guarded(c.M * c.N, True), Guarded(rows * 2 * c.N, False)
        _launch(L, p, c, d, out.body, part.body)
        torch.cuda.synchronize()
        assert out.bands_intact() and part.bands_intact(), "a store outside the output"
        runs.append((out.bits(), part.bits()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "a second call does not repeat the bits"
    bits = R.from_blocks(runs[0][0], c.M, c.N)
    v = R.bf16_widen(bits)
    assert np.isfinite(v).all()
    n_out = R.outside(c.p, v, c.open, c.mask_undecided)
    ratio = R.ratio(c.p, v, c.open)
    part = runs[0][1].view(np.float32).reshape(rows, 2, c.N).astype(np.float64)
    dd, q = R.stat_terms(c, v.astype(np.float64))
    sums = R.stats_outside(part, c.rows_of, dd, q, c.L)
    mask_u = 0 if c.open is None else int(c.mask_undecided.sum())
    print(f"BC {R.case_id(case)} {family} (draw {c.salt}) {c.path.kernel}{c.path.inst}: outside {n_out} of {v.size}, ratio {ratio:.3f}, Y {c.p.Y:.2e}, sums {sums:.3f} (L {c.L}), "
          f"undecided {c.op.undecided.mean():.1e}, widened {c.p.widened_share:.1e}, undecided mask {mask_u}")
    assert n_out == 0, f"{n_out} elements outside the bracket, worst {R.excess(c.p, v, c.open):.3g}x the allowed error"
    assert sums <= 1.0
    if family == "short":
        assert mask_u == 0 and not c.op.undecided.any()
    if c.M >= 2:
        assert np.array_equal(bits[0], bits[-1]), "the copy of a pixel row comes out as other bits"


def test_query_agrees_with_the_launch_over_the_power_of_two_grid():
    """ttk_bc_partial_rows_pw answers -1 exactly where the entry points refuse, and bc_ref.expected_path's rows elsewhere"""
    hip, L, p = _hip()
    check_query(L.cdll.ttk_bc_partial_rows_pw)
    M = 5
    for cin in (32, 64, 128, 256, 512, 1024):
        for cout in (32, 64, 128, 256, 512, 1024):
            w = np.zeros((cout, cin), np.float32)
            prep = _prepare(L, p, w)
            x, bn_i, bn_o = _bf16_dev(np.zeros((M, cin), np.float32)), _f32_dev(np.ones((8, cin))), _f32_dev(np.ones((8, cout)))
            gy = _bf16_dev(np.zeros((M, cout), np.float32))
            for mode, K, N in (("fwd", cin, cout), ("dgrad", cout, cin)):
                rows = L.cdll.ttk_bc_partial_rows_pw(M, K, N)
                out, part = Guarded(M * N, True), Guarded(max(rows, 1) * 2 * N, False)
                try:
                    if mode == "fwd":
                        L.call("ttk_bc_pw_fwd", p(x), p(bn_i), p(prep), p(out.body), p(part.body), None, M, cin, cout)
                    else:
                        L.call("ttk_bc_pw_bwd_data", p(gy), p(gy), p(bn_o), p(prep), p(x), p(bn_i), p(out.body), p(part.body), M, cin, cout)
                    launched = True
                except RuntimeError:
                    launched = False
                torch.cuda.synchronize()
                assert launched == (rows > 0) == (R.expected_path(mode, M, cin, cout) is not None), (mode, cin, cout)
                assert out.bands_intact() and part.bands_intact()
                if launched:
                    assert (out.bits() == 0).all(), (mode, cin, cout)     # zero operands: every output +0
                else:
                    assert out.untouched() and part.untouched(), f"refused {mode} {cin} -> {cout} wrote an output"
    for cin, cout in R.REFUSED_FWD:
        assert L.cdll.ttk_bc_partial_rows_pw(M, cin, cout) == -1
    for cin, cout in R.REFUSED_DGRAD:
        assert L.cdll.ttk_bc_partial_rows_pw(M, cout, cin) == -1


PREP_LAYERS = [(32, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (512, 1024), (1024, 1024), (64, 32), (256, 128),
               (32, 1024), (1024, 32), (32, 32), (128, 64), (32, 64)]


def test_prepare_weights_sixteen_layers_and_refusals():
    hip, L, p = _hip()
    rng = np.random.default_rng(16)
    assert len(PREP_LAYERS) == 16
    ws = [_f32_dev(rng.normal(0, 1, (co, ci)) / np.sqrt(ci)).view(co, ci, 1, 1) for ci, co in PREP_LAYERS]
    size = lambda ci, co: L.cdll.ttk_bc_prepared_bytes(ci, co)
    fresh = lambda: [torch.full((size(ci, co) + 64,), 0xA5, dtype=torch.uint8, device="cuda") for ci, co in PREP_LAYERS]
    together = fresh()
    L.bc_prepare_weights(ws, together)
    single = fresh()
    for w, q in zip(ws, single):
        L.bc_prepare_weights([w], [q])
    torch.cuda.synchronize()
    for i, ((ci, co), a, b) in enumerate(zip(PREP_LAYERS, together, single)):
        assert size(ci, co) == 4 * ci * co
        assert torch.equal(a, b), f"{ci} -> {co}: the image of the sixteen-layer call differs from the single-layer call's"
        assert (a[size(ci, co):] == 0xA5).all(), "a store past the image"
        # the image holds the weights rounded to nearest even, each exactly once per half (forward | data gradient)
        w16 = np.sort(R.bf16_bits(ws[i].cpu().numpy().reshape(-1)))
        img = a[:size(ci, co)].cpu().numpy().view(np.uint16).reshape(2, ci * co)
        assert np.array_equal(np.sort(img[0]), w16) and np.array_equal(np.sort(img[1]), w16)
    # through the forward and the data gradient: the images of the sixteen-layer call give the bits of test_pointwise_rows' single-layer images
    for case in (("fwd", 33, 32, 64), ("dgrad", 257, 256, 256)):
        c = R.pw_case(*case, "full")
        i = PREP_LAYERS.index((c.cin, c.cout))
        ws2 = list(ws)
        ws2[i] = _f32_dev(c.w).view(c.cout, c.cin, 1, 1)
        images = fresh()
        L.bc_prepare_weights(ws2, images)
        d = _inputs(L, p, c)
        outs = []
        for prep in (d["prep"], images[i][:size(c.cin, c.cout)]):
            d["prep"] = prep
            out, part = Guarded(c.M * c.N, True), Guarded(c.path.rows * 2 * c.N, False)
            _launch(L, p, c, d, out.body, part.body)
            torch.cuda.synchronize()
            outs.append((out.bits(), part.bits()))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    # refusals: no layer, seventeen layers, a bad shape in the middle - every image stays as it was
    for bad_ws in ([], ws + ws[:1], ws[:3] + [torch.zeros(48, 32, 1, 1, device="cuda")] + ws[4:]):
        images = fresh() + fresh()[:1]
        before = [q.clone() for q in images]
        with pytest.raises(RuntimeError):
            L.bc_prepare_weights(bad_ws, images[:len(bad_ws)])
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(images, before))


# ---------------------------------------------------------------------------------------------------------------------------------
# pointwise weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", R.WG_CASES, ids=R.wg_id)
def test_pointwise_weight_gradient(case, family):
    hip, L, p = _hip()
    c = R.wg_case(*case, family)
    plan, n = c.plan, c.cin * c.cout
    assert L.cdll.ttk_bc_pw_wgrad_slices(c.M, c.cin, c.cout) == plan.slices
    assert L.cdll.ttk_bc_pw_wgrad_scratch_bytes(c.M, c.cin, c.cout) == plan.scratch_bytes and plan.lds <= R.LDS_LIMIT
    g, y, ydw, bn_pw, bn_dw = _bf16_dev(c.g), _bf16_dev(c.y), _bf16_dev(c.ydw), _f32_dev(c.bn_pw), _f32_dev(c.bn_dw)

    def run(dw0, defer=False):
        dw, scr = Guarded(n, False), Guarded(plan.slices * n, False)       # (the scratch starts as NaN)
        dw.body.copy_(torch.zeros(n, device="cuda") if dw0 is None else _f32_dev(dw0).reshape(-1))
        L.call("ttk_bc_pw_bwd_weight", p(g), p(y), p(bn_pw), p(ydw), p(bn_dw), None if defer else p(dw.body), p(scr.body), c.M, c.cin, c.cout)
        if defer:
            part, bnx = torch.zeros(1, 2, c.cin, device="cuda"), bn_dw.clone()
            gamma, dgm, dbt = torch.ones(c.cin, device="cuda"), torch.zeros(c.cin, device="cuda"), torch.zeros(c.cin, device="cuda")
            L.call("ttk_bc_bn_bwd_finalize_fold", p(part), 1, c.cin, c.M, p(gamma), p(bnx), p(dgm), p(dbt), 0, p(scr.body), plan.slices, n, p(dw.body), 1)
        torch.cuda.synchronize()
        assert dw.bands_intact() and scr.bands_intact(), "a store outside the output"
        return dw.bits().view(np.float32), scr.bits().view(np.float32).reshape(plan.slices, n)

    zeros, tiles = run(None)
    again, tiles2 = run(None)
    assert np.array_equal(zeros.view(np.uint32), again.view(np.uint32)) and np.array_equal(tiles.view(np.uint32), tiles2.view(np.uint32)), "a second call does not repeat the bits"
    assert np.isfinite(tiles).all(), "a slice tile keeps a NaN of the scratch"
    onto, _ = run(c.dw0)
    deferred, _ = run(c.dw0, defer=True)
    fast = plan.fold == "fast"
    assert np.array_equal(R.fold(tiles, np.zeros(n, np.float32), fast).view(np.uint32), zeros.view(np.uint32)), "dW is not the fold of the scratch tiles"
    assert np.array_equal(R.fold(tiles, c.dw0.reshape(-1), fast).view(np.uint32), onto.view(np.uint32)), "dw0 + dW is not the fold of the scratch tiles"
    assert np.array_equal(deferred.view(np.uint32), onto.view(np.uint32)), "the deferred fold differs from the launch's own"
    r0, plain0 = R.wg_ratio(c.p, zeros.reshape(c.cout, c.cin))
    r1, plain1 = R.wg_ratio(R.wg_onto(c.p, c.dw0), onto.reshape(c.cout, c.cin))
    print(f"BC wgrad {R.wg_id(case)} {family} (draw {c.salt}) {plan.inst} {plan.slices} slices, fold {plan.fold}: error / allowed {r0:.3f} (onto dw0 {r1:.3f}), ratio {plain0:.3f} ({plain1:.3f}), "
          f"Y chain {c.p.Y_chain:.2e} own {c.p.Y_own:.2e}, widened {c.p.widened_share:.1e}")
    assert r0 <= 1.0 and r1 <= 1.0


def test_weight_gradient_queries_and_refusals():
    hip, L, p = _hip()
    check_wgrad_queries(L.cdll.ttk_bc_pw_wgrad_slices, L.cdll.ttk_bc_pw_wgrad_scratch_bytes)
    M = 5
    for cin, cout in R.WG_REFUSED:
        assert L.cdll.ttk_bc_pw_wgrad_slices(M, cin, cout) == 0 and L.cdll.ttk_bc_pw_wgrad_scratch_bytes(M, cin, cout) == 0
        x, gy = _bf16_dev(np.zeros((M, cin), np.float32)), _bf16_dev(np.zeros((M, cout), np.float32))
        dw, scr = Guarded(cin * cout, False), Guarded(cin * cout, False)
        with pytest.raises(RuntimeError):
            L.call("ttk_bc_pw_bwd_weight", p(gy), p(gy), p(_f32_dev(np.ones((8, cout)))), p(x), p(_f32_dev(np.ones((8, cin)))), p(dw.body), p(scr.body), M, cin, cout)
        torch.cuda.synchronize()
        assert dw.untouched() and scr.untouched(), f"refused {cin} -> {cout} wrote an output"


# ---------------------------------------------------------------------------------------------------------------------------------
# depthwise forward
# ---------------------------------------------------------------------------------------------------------------------------------
def _nhwc_dev(x):
    return _bf16_dev(x.reshape(-1, x.shape[-1]))


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", R.DW_FWD_CASES, ids=R.dw_id)
def test_depthwise_forward(case, family):
    hip, L, p = _hip()
    c = R.dw_case(*case, family)
    t = c.t
    assert t.lds <= R.LDS_LIMIT, "the launch would ask for more LDS than a workgroup can have"
    assert L.cdll.ttk_bc_partial_rows_dw(c.B, c.H, c.W, c.C, c.stride, 0) == t.rows
    y, sk, bn, w, piv = _nhwc_dev(c.y), (_nhwc_dev(c.sk) if c.skip else None), _f32_dev(c.bn), _f32_dev(c.w), _f32_dev(c.piv)
    n_in, n_out = c.B * c.H * c.W * c.C, c.B * c.Ho * c.Wo * c.C
    runs = []
    for _ in range(2):
        out, part, a_out = Guarded(n_out, True), Guarded(t.rows * 2 * c.C, False), (Guarded(n_in, True) if c.want_a else None)
        L.call("ttk_bc_dw_fwd", p(y), p(bn), p(sk), p(a_out.body) if c.want_a else None, p(w), p(out.body), p(part.body), p(piv), c.B, c.H, c.W, c.C, c.stride)
        torch.cuda.synchronize()
        assert out.bands_intact() and part.bands_intact() and (a_out is None or a_out.bands_intact()), "a store outside the output"
        runs.append((out.bits(), part.bits(), a_out.bits() if c.want_a else None))
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]) if a is not None), "a second call does not repeat the bits"
    bits = R.from_blocks(runs[0][0], c.B * c.Ho * c.Wo, c.C).reshape(c.B, c.Ho, c.Wo, c.C)
    v = R.bf16_widen(bits)
    n_bad, share = R.dw_fwd_outside(c, v)
    rows_of, depth = R.dw_row_of_output(t, c.B)
    part = runs[0][1].view(np.float32).reshape(t.rows, 2, c.C).astype(np.float64)
    d = (v.astype(np.float64) - c.piv.astype(np.float64)).reshape(-1, c.C)
    sums = R.stats_outside(part, rows_of.reshape(-1), d, d * d, depth)
    print(f"BC dw_fwd {R.dw_id(case)} {family} (draw {c.salt}) S{c.stride} SKIP{int(c.skip)} SL{t.SL} CARRY{int(t.carry)} R{t.R} NI{t.NI} NCT{t.NCT} lds {t.lds}: outside {n_bad} of {v.size}, "
          f"bit for bit {share:.4f}, Y {c.p.Y:.2e}, sums {sums:.3f} (L {depth}), undecided a_in {c.a.undecided.mean():.1e}")
    assert n_bad == 0 and share > 0.99 and sums <= 1.0
    if c.want_a:
        a = R.bf16_widen(R.from_blocks(runs[0][2], c.B * c.H * c.W, c.C)).reshape(c.B, c.H, c.W, c.C)
        ok = np.where(c.a.undecided, (a >= c.a.lo) & (a <= c.a.hi), a.view(np.uint32) == (c.a.v + np.float32(0)).view(np.uint32))
        assert ok.all(), "a_out is not the emulated block input bit for bit"
    if c.B > 1:
        assert np.array_equal(bits[0], bits[-1]), "the copy of an image comes out as other bits"


def test_depthwise_queries_and_refusals():
    hip, L, p = _hip()
    from test_bc_ref import check_dw_query
    check_dw_query(L.cdll.ttk_bc_partial_rows_dw)
    x = _bf16_dev(np.zeros((5 * 257, 64), np.float32))
    bn, w = _f32_dev(np.ones((8, 2048))), _f32_dev(np.zeros((2048, 9)))

    def refused(name, *args):
        out, part, a_out = Guarded(5 * 257 * 64, True), Guarded(4096, False), Guarded(5 * 257 * 64, True)
        with pytest.raises(RuntimeError):
            if name == "fwd":
                B, H, W, C, s, want_a = args
                L.call("ttk_bc_dw_fwd", p(x), p(bn), None, p(a_out.body) if want_a else None, p(w), p(out.body), p(part.body), None, B, H, W, C, s)
            else:
                B, H, W, C, s, sg, acc, partial = args
                L.call("ttk_bc_dw_bwd_data", p(x), p(x), p(bn), p(w), p(x) if sg else None, p(x), p(bn), None, None, p(out.body), p(part.body), p(a_out.body.view(torch.float32)),
                       acc, p(x.view(torch.float32)) if partial else None, B, H, W, C, s)
        torch.cuda.synchronize()
        assert out.untouched() and part.untouched() and a_out.untouched(), f"refused {name}{args} wrote an output"

    for B, H, W, C, s in R.DW_REFUSED:
        refused("fwd", B, H, W, C, s, False)
        refused("bwd", B, H, W, C, s, False, 1, False)
    refused("fwd", 1, 5, 5, 64, 2, True)                 # a_out with stride 2
    refused("bwd", 1, 5, 5, 64, 2, True, 1, False)       # skip_grad with stride 2
    refused("bwd", 1, 5, 5, 64, 1, False, 2, False)      # dw_accumulate = 2 without dw_partial


# ---------------------------------------------------------------------------------------------------------------------------------
# fused pointwise backward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", R.FUSED_CASES, ids=R.wg_id)
def test_pointwise_backward_fused(case, family):
    hip, L, p = _hip()
    f = R.fused_case(*case, family)
    c, plan, n = f.c, f.plan, f.c.cin * f.c.cout
    assert L.cdll.ttk_bc_pw_bwd_fused_rows(c.M, c.cin, c.cout) == plan.slices and plan.lds <= R.LDS_LIMIT
    assert L.cdll.ttk_bc_pw_bwd_fused_scratch_bytes(c.M, c.cin, c.cout) == plan.scratch_bytes
    g, y, ydw, bn_pw, bn_dw, prep = _bf16_dev(c.g), _bf16_dev(c.y), _bf16_dev(c.ydw), _f32_dev(c.bn_pw), _f32_dev(c.bn_dw), _prepare(L, p, f.w)

    def run(dw0, defer=False):
        gd, part, dw, scr = Guarded(c.M * c.cin, True), Guarded(plan.slices * 2 * c.cin, False), Guarded(n, False), Guarded(plan.slices * n, False)
        dw.body.copy_(torch.zeros(n, device="cuda") if dw0 is None else _f32_dev(dw0).reshape(-1))
        L.call("ttk_bc_pw_bwd_fused", p(g), p(y), p(bn_pw), p(prep), p(ydw), p(bn_dw), p(gd.body), None if defer else p(dw.body), p(scr.body), p(part.body), c.M, c.cin, c.cout)
        if defer:
            bnx, z = bn_dw.clone(), [torch.zeros(c.cin, device="cuda") for _ in range(2)]
            L.call("ttk_bc_bn_bwd_finalize_fold", p(torch.zeros(1, 2, c.cin, device="cuda")), 1, c.cin, c.M, p(torch.ones(c.cin, device="cuda")), p(bnx), p(z[0]), p(z[1]), 0,
                   p(scr.body), plan.slices, n, p(dw.body), 1)
        torch.cuda.synchronize()
        assert gd.bands_intact() and part.bands_intact() and dw.bands_intact() and scr.bands_intact(), "a store outside the output"
        return gd.bits(), part.bits(), dw.bits(), scr.bits().view(np.float32).reshape(plan.slices, n)

    first, again = run(None), run(None)
    assert all(np.array_equal(a, b) for a, b in zip(first, again)), "a second call does not repeat the bits"
    onto, deferred = run(c.dw0), run(c.dw0, defer=True)
    assert np.array_equal(onto[2], deferred[2]), "the deferred fold differs from the launch's own"
    # the data gradient: ttk_bc_pw_bwd_data's bits, and inside the criterion itself
    rows_pw = L.cdll.ttk_bc_partial_rows_pw(c.M, c.cout, c.cin)
    sep, sep_part = Guarded(c.M * c.cin, True), Guarded(rows_pw * 2 * c.cin, False)
    L.call("ttk_bc_pw_bwd_data", p(g), p(y), p(bn_pw), p(prep), p(ydw), p(bn_dw), p(sep.body), p(sep_part.body), c.M, c.cin, c.cout)
    torch.cuda.synchronize()
    assert np.array_equal(first[0], sep.bits()), "the fused data gradient differs from ttk_bc_pw_bwd_data's"
    v = R.bf16_widen(R.from_blocks(first[0], c.M, c.cin))
    n_out = R.outside(f.dg, v, f.open, f.mask_undecided)
    part = first[1].view(np.float32).reshape(plan.slices, 2, c.cin).astype(np.float64)
    v64 = v.astype(np.float64)
    sums = R.stats_outside(part, np.arange(c.M) // plan.rows, v64, v64 * (c.ydw.astype(np.float64) - c.bn_dw[R.BN_MEAN].astype(np.float64)), plan.depth)
    # the weight gradient
    tiles = first[3]
    assert np.isfinite(tiles).all()
    # (fold_rows_fast_body's tree from 16 slices on, fold_partials_k's serial order below: both restated by bc_ref.fold)
    assert np.array_equal(R.fold(tiles, np.zeros(n, np.float32), plan.fold == "fast").view(np.uint32), first[2]), "dW is not the fold of the scratch tiles"
    assert np.array_equal(R.fold(tiles, c.dw0.reshape(-1), plan.fold == "fast").view(np.uint32), onto[2]), "dw0 + dW is not the fold of the scratch tiles"
    r0, plain0 = R.wg_ratio(c.p, first[2].view(np.float32).reshape(c.cout, c.cin))
    r1, plain1 = R.wg_ratio(R.wg_onto(c.p, c.dw0), onto[2].view(np.float32).reshape(c.cout, c.cin))
    print(f"BC fused {R.wg_id(case)} {family} (draw {c.salt}) {plan.inst} {plan.slices} slices, fold {plan.fold}: data gradient outside {n_out} of {v.size}, sums {sums:.3f} (L {plan.depth}); "
          f"dW error / allowed {r0:.3f} (onto dw0 {r1:.3f}), ratio {plain0:.3f} ({plain1:.3f})")
    assert n_out == 0 and sums <= 1.0 and r0 <= 1.0 and r1 <= 1.0


def test_fused_queries():
    hip, L, p = _hip()
    from test_bc_ref import check_fused_queries
    check_fused_queries(L.cdll.ttk_bc_pw_bwd_fused_rows, L.cdll.ttk_bc_pw_bwd_fused_scratch_bytes)



# ---------------------------------------------------------------------------------------------------------------------------------
# depthwise data gradient + fused weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", R.DW_BWD_CASES, ids=R.dwb_id)
def test_depthwise_backward(case, family):
    hip, L, p = _hip()
    c = R.dw_bwd_case(*case, family)
    t, C = c.t, c.C
    assert t.lds <= R.LDS_LIMIT and L.cdll.ttk_bc_partial_rows_dw(c.B, c.H, c.W, C, c.stride, 1) == t.rows
    g, ydw, yprev = _nhwc_dev(c.g), _nhwc_dev(c.ydw), _nhwc_dev(c.yprev)
    sk, sg = (None if c.sk is None else _nhwc_dev(c.sk)), (None if c.sg is None else _nhwc_dev(c.sg))
    a_given = _nhwc_dev(c.a.v) if c.form != "lean" and not c.a.undecided.any() else None   # (the materialised block input, both strides)
    bn_dw, bn_prev, w = _f32_dev(c.bn_dw), _f32_dev(c.bn_prev), _f32_dev(c.w)
    n_in = c.B * c.H * c.W * C

    def run(accumulate, partial, a_in=None, dw0=None, fold_after=False):
        gp, part, dw, rows = Guarded(n_in, True), Guarded(t.rows * 2 * C, False), Guarded(9 * C, False), Guarded(t.rows * 9 * C, False)
        if dw0 is not None:
            dw.body.copy_(_f32_dev(dw0).reshape(-1))
        L.call("ttk_bc_dw_bwd_data", p(g), p(ydw), p(bn_dw), p(w), p(sg), p(yprev), p(bn_prev), p(sk), p(a_in), p(gp.body), p(part.body), p(dw.body), accumulate,
               p(rows.body) if partial else None, c.B, c.H, c.W, C, c.stride)
        if fold_after:
            bnx, z = bn_prev.clone(), [torch.zeros(C, device="cuda") for _ in range(2)]
            L.call("ttk_bc_bn_bwd_finalize_fold", p(torch.zeros(1, 2, C, device="cuda")), 1, C, c.B * c.H * c.W, p(torch.ones(C, device="cuda")), p(bnx), p(z[0]), p(z[1]), 0,
                   p(rows.body), t.rows, 9 * C, p(dw.body), 1)
        torch.cuda.synchronize()
        assert gp.bands_intact() and part.bands_intact() and dw.bands_intact() and rows.bands_intact(), "a store outside the output"
        assert partial or rows.untouched()
        return gp.bits(), part.bits(), dw.bits().view(np.float32).reshape(C, 9), rows.bits().view(np.float32).reshape(t.rows, 9 * C)

    folded, again = run(0, True), run(0, True)                      # rows folded onto NaN (overwriting)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(folded, again)), "a second call does not repeat the bits"
    onto = run(1, True, dw0=c.dw0)                                  # rows folded onto dw0
    deferred = run(2, True, dw0=c.dw0, fold_after=True)             # rows left for ttk_bc_bn_bwd_finalize_fold
    atom0, atom1 = run(0, False), run(1, False, dw0=c.dw0)          # memset + atomics | accumulating atomics: held to the criterion only
    assert np.array_equal(onto[2].view(np.uint32), deferred[2].view(np.uint32)), "the deferred fold differs from the launch's own"
    others = [onto, deferred, atom0, atom1] + ([run(0, True, a_in=a_given)] if a_given is not None else [])
    assert all(np.array_equal(o[0], folded[0]) and np.array_equal(o[1], folded[1]) for o in others), "g_prev / part differ between the weight-gradient modes or with a_in given"
    if a_given is not None:
        assert np.array_equal(others[-1][2].view(np.uint32), folded[2].view(np.uint32))
    # ---- data gradient and its sums
    v = R.bf16_widen(R.from_blocks(folded[0], c.B * c.H * c.W, C)).reshape(c.B, c.H, c.W, C)
    n_bad, share = R.dw_bwd_outside(c, v)
    rows_of, depth = R.dw_bwd_rows(t, c.B, c.H, c.W, c.stride)
    part = folded[1].view(np.float32).reshape(t.rows, 2, C).astype(np.float64)
    v64 = v.astype(np.float64).reshape(-1, C)
    sums = R.stats_outside(part, rows_of.reshape(-1), v64, v64 * (c.yprev.astype(np.float64).reshape(-1, C) - c.bn_prev[R.BN_MEAN].astype(np.float64)), depth)
    # ---- weight gradient
    tiles = folded[3]
    fast = R.fold_fast_ok(t.rows, 9 * C)
    # (fold_rows_fast_body's tree from 16 rows on, fold_partials_k's serial order below: both restated by bc_ref.fold)
    assert np.array_equal(R.fold(tiles, None, fast, False).view(np.uint32), folded[2].reshape(-1).view(np.uint32)), "dW is not the fold of the workgroup rows"
    assert np.array_equal(R.fold(tiles, c.dw0.reshape(-1), fast).view(np.uint32), onto[2].reshape(-1).view(np.uint32)), "dw0 + dW is not the fold of the workgroup rows"
    q0, q1 = c.q, R.wg_onto(c.q, c.dw0)
    r = [R.wg_ratio(q0, folded[2])[0], R.wg_ratio(q1, onto[2])[0], R.wg_ratio(q0, atom0[2])[0], R.wg_ratio(q1, atom1[2])[0]]
    print(f"BC dw_bwd {R.dwb_id(case)} {family} (draw {c.salt}) S{c.stride} SL{t.SL} R{t.R} NI{t.NI} NCT{t.NCT} rows {t.rows}{' fast fold' if fast else ''}: g_prev outside {n_bad} of {v.size}, bit for bit {share:.4f}, "
          f"Y {c.p.Y:.2e}, sums {sums:.3f} (L {depth}); dW error / allowed rows {r[0]:.3f}, rows onto dw0 {r[1]:.3f}, atomics {r[2]:.3f}, atomics onto dw0 {r[3]:.3f} (Y {c.q.Y:.2e}), "
          f"undecided dy {c.dy.undecided.mean():.1e}, undecided mask {int(c.mask_undecided.sum())}")
    assert n_bad == 0 and sums <= 1.0 and max(r) <= 1.0
    if c.B > 1:
        gb = R.from_blocks(folded[0], c.B * c.H * c.W, C).reshape(c.B, -1)
        assert np.array_equal(gb[0], gb[-1]), "the copy of an image comes out as other bits"
