"""The MobileNet pointwise (1x1) GEMMs through the C ABI, row by row against float64, at every kernel form (tests/pw_ref.py: the
reference, the yardstick, the criterion's two pointwise differences, the table of cases with the kernel instantiation each is there for;
tests/test_pw_ref.py: all of that on its own, and the mutations the criterion catches):
  * ttk_pwconv1x1_fwd and ttk_pwconv1x1_bwd_data with the per-call split, with the block of ttk_pwconv_prepare_weights and - where the
    table says so - with wsplit = NULL; activations through to_blocks / from_blocks; the partial sums, exactly the reported row count;
  * ttk_pwconv1x1_bwd_weight with atomics and, where ttk_pwconv_wgrad_partial_bytes reports a size, with scratch (bitwise repeatable);
    accumulation onto a non-zero dw once per kernel form;
  * ttk_pwconv1x1_bwd_fused: both outputs by the same criterion, with and without scratch;
  * the 192- and 256-row tiles of the row-block kernels at the smallest M the cost model gives them on this device (searched).
Every output starts as NaN (a weight gradient: zeros; scratch: NaN) between two NaN guard bands, must be finite afterwards and the bands
untouched; every call runs twice on fresh buffers and repeats bit for bit (the atomic weight gradients need not); bn_dw and bn_pw are
bitwise unchanged after every call.  The zero-operand input channels give exactly-zero weight-gradient columns, the always-closed
channel an exactly-zero data-gradient column.

Each output prints `RATIO <entry> <form> <case> <value>`, value = worst (|x - f64| - floor - 2^-24 s) / (s Y) over its elements
(conv_ref.Product.ratio); the assertion is value <= MARGIN = 4.  Worst per entry point on the MI355X (profiles/pw_float64.txt has the
forms and cases):
    ttk_pwconv1x1_fwd 1.07 (pw16r_k<6,FWD>, 8193x128x1024)   ttk_pwconv1x1_bwd_data 0.84 (pw_gemm_k<128,2,2,DGRAD,2> without wsplit, 129x256x128)
    ttk_pwconv1x1_bwd_weight 1.09 (pw_wgrad_k<128,32>, both forms, 256x32x128)
    ttk_pwconv1x1_bwd_fused: data gradient 1.08, weight gradient 2.84 with atomics and 0.82 with scratch (pw_bwd_fused_k<32,64> at
    32801x32x64, where Y is the blocked chain's 6.4e-8; pw_bwd_fused16_k<128,128> at 33x128x128)
Refused, outputs still NaN: Cin = 48, Cin = 2048, M = 0; ttk_pwconv1x1_bwd_fused at 64 -> 64 and, for the fp16 forms, without wsplit."""
import functools

import numpy as np
import pytest
import torch

import pw_ref as R
from test_conv_rows_gpu import Guard, _bits, _check_forward_sums, _t

pytestmark = pytest.mark.gpu
NAN = float("nan")
_ids = lambda v: "x".join(map(str, v))


def _lib():
    import trackertraincode._hip as hip
    return hip.lib(), hip.ptr, hip


@functools.lru_cache(maxsize=None)
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=2)
def _dev(case):
    """the case's inputs on the device (activations in channel blocks), the transposed weights and the prepared weight block"""
    L, p, H = _lib()
    c = R.make_case(case)
    d = dict(ydw=H.to_blocks(_t(c.ydw)), g=H.to_blocks(_t(c.g)), y=H.to_blocks(_t(c.y32)), w=_t(c.w), wt=_t(c.w.T), piv=_t(c.piv),
             bn_dw=_t(c.bn_dw), bn_pw=_t(c.bn))
    G = Guard()
    d["prep"] = G.new(L.pwconv_prepared_bytes(c.Cin, c.Cout), dtype=torch.uint8, fill=0xff)
    L.pwconv_prepare_weights([d["w"].view(c.Cout, c.Cin, 1, 1)], [d["prep"]])
    G.check("pwconv_prepare_weights")
    return c, d


def _bn_unchanged(c, d, what):
    torch.cuda.synchronize()
    assert torch.equal(_bits(d["bn_dw"]), _bits(_t(c.bn_dw))) and torch.equal(_bits(d["bn_pw"]), _bits(_t(c.bn))), (what, "a BatchNorm block was written")


def _judge(entry, form, case, p, out, masked=False):
    out = np.asarray(out, np.float64)
    assert np.isfinite(out).all(), (entry, form, case, "NaN left or written")
    ratio, zeros_ok = R.masked_ratio(p, out) if masked else p.ratio(out)
    print("RATIO", entry, form, _ids(case), f"{ratio:.3f}")
    assert zeros_ok, (entry, form, case, "an element whose every product is zero (or whose mask is closed) is not exactly zero")
    if not ratio <= R.MARGIN:
        e = (np.abs(out - p.ref) - p.floor - R.U * p.s) / np.where(p.s > 0, p.s * p.Y, np.inf)
        row = int(e.max(1).argmax())
        raise AssertionError((entry, form, case, f"ratio {ratio:.2f} > {R.MARGIN} in row {row} of {out.shape[0]}", f"Y {p.Y:.2e}"))
    return ratio


def _check_dgrad_sums(part, out, c, tol):
    """part[rows][2][Cin]: (sum g_dw, sum g_dw * (ydw - mean)) per channel against the gradient the kernel stored, at the tolerance of
    tests/test_pwconv_gpu.py (2e-5) / of its fused test (3e-5); no NaN left in any row"""
    ps = part.cpu().numpy().astype(np.float64)
    assert np.isfinite(ps).all()
    o64 = out.astype(np.float64)
    yc = c.ydw.astype(np.float64) - c.bn_dw[R.BN_MEAN]
    np.testing.assert_allclose(ps[:, 0].sum(0), o64.sum(0), rtol=0, atol=tol * np.abs(o64).sum(0).max())
    np.testing.assert_allclose(ps[:, 1].sum(0), (o64 * yc).sum(0), rtol=0, atol=tol * np.abs(o64 * yc).sum(0).max())


def _weights(d, form, G, L, c, transposed):
    """(w argument, wsplit argument) of one form: per-call split into fresh scratch | the prepared block | raw weights alone"""
    w = d["wt"] if transposed else d["w"]
    if form == "percall":
        return w, G.new(L.pwconv_prepared_bytes(c.Cin, c.Cout), dtype=torch.uint8, fill=0xff)
    return (None, d["prep"]) if form == "prepared" else (w, None)


def _part_rows(L, M, K, Nout, dgrad, form):
    """rows of `part` the call writes: ttk_partial_rows_pwconv for the kernel that runs the shape when it is given wsplit; with
    wsplit = NULL the fp32 kernels run whatever the shape, and they write one row per 128 rows of M, ttk_partial_rows_gemm(M)
    (include/ttk.h) - at the row-block shapes that is NOT what ttk_partial_rows_pwconv reports"""
    rows = L.partial_rows_gemm(M, K, Nout, dgrad)
    assert rows == R.partial_rows(M, K, Nout, dgrad, _cus())
    return rows if form != "nosplit" else L.partial_rows_gemm(M)


def _forward(case, forms):
    L, p, H = _lib()
    c, d = _dev(case)
    for form in forms:
        rows = _part_rows(L, c.M, c.Cin, c.Cout, False, form)
        name = R.gemm_path(c.M, c.Cin, c.Cout, False, form != "nosplit", _cus())
        ref = R.forward(case, not R.is_fp32_form(name))
        runs = []
        for _ in range(2):
            G = Guard()
            y, part = G.new(c.M, c.Cout), G.new(rows, 2, c.Cout)
            w, ws = _weights(d, form, G, L, c, False)
            L.call("ttk_pwconv1x1_fwd", p(d["ydw"]), p(d["bn_dw"]), p(w), p(y), p(part), p(d["piv"]), c.M, c.Cin, c.Cout, p(ws), 0)
            G.check("pwconv1x1_fwd " + form)
            runs.append((y, part))
        (y, part), (y2, part2) = runs
        assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(part), _bits(part2)), form
        out = H.from_blocks(y).cpu().numpy()
        _judge("fwd", f"{form}:{name}", case, ref, out)
        _check_forward_sums(part, out, ref, c.piv)
    _bn_unchanged(c, d, "pwconv1x1_fwd")


def _dgrad(case, forms):
    L, p, H = _lib()
    c, d = _dev(case)
    for form in forms:
        rows = _part_rows(L, c.M, c.Cout, c.Cin, True, form)
        name = R.gemm_path(c.M, c.Cout, c.Cin, True, form != "nosplit", _cus())
        ref = R.dgrad(case, not R.is_fp32_form(name))
        assert ref.share <= R.UNDECIDED_CAP
        runs = []
        for _ in range(2):
            G = Guard()
            g_dw, part = G.new(c.M, c.Cin), G.new(rows, 2, c.Cin)
            wt, ws = _weights(d, form, G, L, c, True)
            L.call("ttk_pwconv1x1_bwd_data", p(d["g"]), p(d["y"]), p(d["bn_pw"]), p(wt), p(d["ydw"]), p(d["bn_dw"]), p(g_dw), p(part), c.M, c.Cin,
                   c.Cout, p(ws), 0)
            G.check("pwconv1x1_bwd_data " + form)
            runs.append((g_dw, part))
        (g_dw, part), (g2, part2) = runs
        assert torch.equal(_bits(g_dw), _bits(g2)) and torch.equal(_bits(part), _bits(part2)), form
        out = H.from_blocks(g_dw).cpu().numpy()
        _judge("bwd_data", f"{form}:{name}", case, ref, out, masked=True)
        assert np.all(out[:, c.closed_channel] == 0) and np.all(out[:, c.zero_channels] == 0)
        _check_dgrad_sums(part, out, c, 2e-5)
    _bn_unchanged(c, d, "pwconv1x1_bwd_data")


@pytest.mark.parametrize("case", R.cases_of("f"), ids=_ids)
def test_pw_fwd_rows(case):
    _forward(case, ("percall", "prepared"))


@pytest.mark.parametrize("case", R.cases_of("d"), ids=_ids)
def test_pw_bwd_data_rows(case):
    _dgrad(case, ("percall", "prepared"))


@pytest.mark.parametrize("case", R.cases_of("n"), ids=_ids)
def test_pw_fwd_and_bwd_data_without_wsplit(case):
    """wsplit = NULL selects the fp32 MFMA kernels at shapes that otherwise run split (include/ttk.h): pw_gemm_k<128,...> with K >= 64"""
    e = R.expected_path(*case, _cus())
    assert R.is_fp32_form(e["fwd_nosplit"]) and R.is_fp32_form(e["dgrad_nosplit"]) and not R.is_fp32_form(e["fwd"]) and not R.is_fp32_form(e["dgrad"])
    _forward(case, ("nosplit",))
    _dgrad(case, ("nosplit",))


@pytest.mark.parametrize("Cin,Cout,dgrad,want", R.TALL, ids=lambda v: str(int(v)))
def test_row_block_kernels_at_192_and_256_row_tiles(Cin, Cout, dgrad, want):
    """pw16r_k<6|8,FWD>, pw16m_k<6,DGRAD>, pw16r_k<8,DGRAD>: the smallest M at which ttk_pwconv_tile_rows reports the height (four column
    tiles: the row count is lowest), found as test_pwconv_gpu.py::test_row_block_gemm_every_tile_height searches - and the restated cost
    model agrees with the library on it and on the way there."""
    L, p, H = _lib()
    M = R.find_tall_M(L.cdll.ttk_pwconv_tile_rows, Cin, Cout, dgrad, want)
    assert M is not None, f"no M below {R.TALL_LIMIT} runs {want}-row tiles for {Cin}->{Cout}"
    K, Nout = (Cout, Cin) if dgrad else (Cin, Cout)
    rblk, rt, blocks = R.r_plan(M, K, Nout, _cus())
    print(f"TALL {Cin}->{Cout} {'dgrad' if dgrad else 'fwd'}: {want}-row tiles first at M = {M} (rt {rt}, {blocks} row blocks, {_cus()} CUs)")
    assert 32 * rblk == want and R.find_tall_M(lambda *a: R.tile_rows(*a, cus=_cus()), Cin, Cout, dgrad, want) == M
    name = R.gemm_path(M, K, Nout, dgrad, True, _cus())
    assert name == {(False, 192): "pw16r_k<6,FWD>", (False, 256): "pw16r_k<8,FWD>", (True, 192): "pw16m_k<6,DGRAD>", (True, 256): "pw16r_k<8,DGRAD>"}[(dgrad, want)]
    (_dgrad if dgrad else _forward)((M, Cin, Cout), ("prepared",))


def _wgrad_forms(L, c):
    nb = L.pwconv_wgrad_partial_bytes(c.M, c.Cin, c.Cout)
    assert nb == R.wgrad_partial_bytes(c.M, c.Cin, c.Cout)  # 4 * Cin * Cout * slices of the restated plan, 0 where no reproducible form
    return nb, [("atomic", False)] + ([("scratch", True)] if nb else [])


@pytest.mark.parametrize("case", R.cases_of("w"), ids=_ids)
def test_pw_bwd_weight_rows(case):
    L, p, H = _lib()
    c, d = _dev(case)
    nb, forms = _wgrad_forms(L, c)
    for form, use_scratch in forms:
        name, slices, rows, _ = R.wgrad_plan(c.M, c.Cin, c.Cout, use_scratch)
        ref = R.wgrad(case, not R.is_fp32_form(name))
        runs = []
        for _ in range(2):
            G = Guard()
            dw = G.zeros(c.Cout, c.Cin)
            scratch = G.new(nb // 4) if use_scratch else None
            L.call("ttk_pwconv1x1_bwd_weight", p(d["g"]), p(d["y"]), p(d["bn_pw"]), p(d["ydw"]), p(d["bn_dw"]), p(dw), p(scratch), c.M, c.Cin, c.Cout, 0)
            G.check("pwconv1x1_bwd_weight " + form)
            if use_scratch:
                assert bool(torch.isfinite(scratch).all()), "a slice tile of the scratch was not written"
            runs.append(dw)
        if use_scratch:
            assert torch.equal(_bits(runs[0]), _bits(runs[1])), form  # the slice-wise form is bitwise reproducible
        for dw in runs:
            out = dw.cpu().numpy()
            _judge("bwd_weight", f"{form}:{name}", case, ref, out)
            assert np.all(out[:, c.zero_channels] == 0)
    _bn_unchanged(c, d, "pwconv1x1_bwd_weight")


def _accumulate_cases():
    """one case per weight-gradient kernel form and scratch use: the first M of the table with two slices"""
    seen, out = set(), []
    for case in R.cases_of("w"):
        for use_scratch in (False, True):
            if use_scratch and not R.wgrad_partial_bytes(*case):
                continue
            name, slices, _, _ = R.wgrad_plan(*case, use_scratch)
            if slices == 2 and (name, use_scratch) not in seen:
                seen.add((name, use_scratch))
                out.append((case, use_scratch))
    return out


@pytest.mark.parametrize("case,use_scratch", _accumulate_cases(), ids=lambda v: _ids(v) if isinstance(v, tuple) else ("scratch" if v else "atomic"))
def test_pw_bwd_weight_accumulates_onto_dw(case, use_scratch):
    """dw holds a running gradient dw0 = +-s / 2 (s: the element's float64 scale): the result is dw0 + the product.  On top of what the
    criterion allows the product itself, every float32 addition onto dw rounds at most 2^-24 (|dw0| + s); an element receives at most
    four additions per slice (the waves that share a tile through atomics), so n = 4 * slices of them.  A zero-operand column receives
    +0 only: dw0 comes back bit for bit."""
    L, p, H = _lib()
    c, d = _dev(case)
    name, slices, _, _ = R.wgrad_plan(*case, use_scratch)
    ref = R.wgrad(case, not R.is_fp32_form(name))
    rng = np.random.default_rng(7)
    dw0 = (0.5 * ref.s * rng.choice([-1.0, 1.0], ref.s.shape)).astype(np.float32)
    dw0[:, c.zero_channels] = rng.normal(0, 1, (c.Cout, 2)).astype(np.float32)
    G = Guard()
    dw = G.new(c.Cout, c.Cin)
    dw.copy_(_t(dw0))
    scratch = G.new(L.pwconv_wgrad_partial_bytes(*case) // 4) if use_scratch else None
    L.call("ttk_pwconv1x1_bwd_weight", p(d["g"]), p(d["y"]), p(d["bn_pw"]), p(d["ydw"]), p(d["bn_dw"]), p(dw), p(scratch), c.M, c.Cin, c.Cout, 0)
    G.check("pwconv1x1_bwd_weight onto dw")
    out = dw.cpu().numpy()
    assert np.isfinite(out).all()
    assert np.array_equal(out[:, c.zero_channels], dw0[:, c.zero_channels])
    err = np.abs(out.astype(np.float64) - dw0 - ref.ref)
    allowed = ref.allowed() + 4 * slices * R.U * (np.abs(dw0) + ref.s)
    print("ACCUMULATE", name, "scratch" if use_scratch else "atomic", _ids(case), f"worst err / allowed {float((err[ref.s > 0] / allowed[ref.s > 0]).max()):.3f}")
    assert np.all(err <= allowed), name


@pytest.mark.parametrize("case", R.cases_of("u"), ids=_ids)
def test_pw_bwd_fused_rows(case):
    L, p, H = _lib()
    c, d = _dev(case)
    name = R.FUSED[(c.Cin, c.Cout)][0]
    split = not R.is_fp32_form(name)
    rd, rw = R.dgrad(case, split), R.wgrad(case, split)
    assert rd.share <= R.UNDECIDED_CAP
    rows = L.cdll.ttk_pwconv1x1_bwd_fused_rows(c.M, c.Cin, c.Cout)
    nb = L.cdll.ttk_pwconv1x1_bwd_fused_partial_bytes(c.M, c.Cin, c.Cout)
    assert rows == R.fused_rows(c.M, c.Cin, c.Cout) and nb == 4 * rows * c.Cin * c.Cout
    for form in ("atomic", "scratch"):
        runs = []
        for _ in range(2):
            G = Guard()
            g_dw, part, dw = G.new(c.M, c.Cin), G.new(rows, 2, c.Cin), G.zeros(c.Cout, c.Cin)
            scratch = G.new(nb // 4) if form == "scratch" else None
            L.call("ttk_pwconv1x1_bwd_fused", p(d["g"]), p(d["y"]), p(d["bn_pw"]), p(d["w"]), p(d["prep"]), p(d["ydw"]), p(d["bn_dw"]), p(g_dw), p(dw),
                   p(scratch), p(part), c.M, c.Cin, c.Cout)
            G.check("pwconv1x1_bwd_fused " + form)
            if scratch is not None:
                assert bool(torch.isfinite(scratch).all()), "a walker's tile of the scratch was not written"
            runs.append((g_dw, part, dw))
        for i, (x, x2) in enumerate(zip(*runs)):
            if i < 2 or form == "scratch":  # the atomic weight gradient need not repeat
                assert torch.equal(_bits(x), _bits(x2)), (form, i)
        g_dw, part, _ = runs[0]
        out = H.from_blocks(g_dw).cpu().numpy()
        _judge("bwd_fused_data", f"{form}:{name}", case, rd, out, masked=True)
        assert np.all(out[:, c.closed_channel] == 0) and np.all(out[:, c.zero_channels] == 0)
        _check_dgrad_sums(part, out, c, 3e-5)
        for _, _, dw in runs:
            o = dw.cpu().numpy()
            _judge("bwd_fused_weight", f"{form}:{name}", case, rw, o)
            assert np.all(o[:, c.zero_channels] == 0)
    _bn_unchanged(c, d, "pwconv1x1_bwd_fused")


def test_wgrad_partial_bytes_is_zero_exactly_where_the_scratch_form_is_not_reproducible():
    """Host only: for every (Cin, Cout) the reported scratch size is that of the restated slice plan, and 0 for 32 -> 32 alone, whose one
    32 x 32 tile is shared by four waves through atomics (ttk_pwconv1x1_bwd_weight drops the scratch there; include/ttk.h: 0 = no such
    form).  The launches that show the reproducibility are the table's own cases (test_pw_bwd_weight_rows)."""
    L, p, H = _lib()
    chans = [32 << i for i in range(6)]
    for M in (1, 64, 65, 129, 257, 300, 5000, 140001):
        for ci in chans:
            for co in chans:
                nb = L.pwconv_wgrad_partial_bytes(M, ci, co)
                assert nb == R.wgrad_partial_bytes(M, ci, co), (M, ci, co)
                assert (nb == 0) == (ci == 32 and co == 32)
    assert L.pwconv_wgrad_partial_bytes(300, 48, 64) == 0 and L.pwconv_wgrad_partial_bytes(0, 64, 64) == 0


def test_refusals_leave_the_outputs_untouched():
    L, p, H = _lib()
    rng = np.random.default_rng(3)
    M, C = 4, 2048
    x = _t(rng.normal(0, 1, (M, C)).astype(np.float32))
    bn = _t(R.bn_block(C, rng))
    w = _t(rng.normal(0, 1, (C, C)).astype(np.float32))
    G = Guard()
    out, part, dw = G.new(M, C), G.new(4, 2, C), G.new(C, C)
    ws = G.new(L.pwconv_prepared_bytes(1024, 1024), dtype=torch.uint8, fill=0xff)
    for m, cin, cout in ((4, 48, 64), (4, 2048, 64), (4, 64, 2048), (0, 64, 64)):
        with pytest.raises(RuntimeError, match="pwconv1x1_fwd: unsupported shape"):
            L.call("ttk_pwconv1x1_fwd", p(x), p(bn), p(w), p(out), p(part), None, m, cin, cout, p(ws), 0)
        with pytest.raises(RuntimeError, match="pwconv1x1_bwd_data: unsupported shape"):
            L.call("ttk_pwconv1x1_bwd_data", p(x), p(x), p(bn), p(w), p(x), p(bn), p(out), p(part), m, cin, cout, p(ws), 0)
        with pytest.raises(RuntimeError, match="pwconv1x1_bwd_weight: unsupported shape"):
            L.call("ttk_pwconv1x1_bwd_weight", p(x), p(x), p(bn), p(x), p(bn), p(dw), None, m, cin, cout, 0)
        with pytest.raises(RuntimeError, match="pwconv1x1_bwd_fused: only the"):
            L.call("ttk_pwconv1x1_bwd_fused", p(x), p(x), p(bn), p(w), p(ws), p(x), p(bn), p(out), p(dw), None, p(part), m, cin, cout)
    with pytest.raises(RuntimeError, match="pwconv1x1_bwd_fused: only the"):
        L.call("ttk_pwconv1x1_bwd_fused", p(x), p(x), p(bn), p(w), p(ws), p(x), p(bn), p(out), p(dw), None, p(part), 4, 64, 64)
    assert L.cdll.ttk_pwconv1x1_bwd_fused_rows(4, 64, 64) == 0 and L.cdll.ttk_pwconv1x1_bwd_fused_partial_bytes(4, 64, 64) == 0
    for cin, cout in ((64, 128), (128, 128), (128, 256), (256, 256)):  # the fp16 forms need the prepared block
        with pytest.raises(RuntimeError, match="pwconv1x1_bwd_fused: the fp16 forms"):
            L.call("ttk_pwconv1x1_bwd_fused", p(x), p(x), p(bn), p(w), None, p(x), p(bn), p(out), p(dw), None, p(part), 4, cin, cout)
    G.check("refused pointwise calls")
    assert bool(out.isnan().all()) and bool(part.isnan().all()) and bool(dw.isnan().all()) and bool((ws == 0xff).all())
