"""The 5x5 stem through the C ABI, element by element against float64, at every kernel form (tests/stem_ref.py: the reference, the
yardstick, the criterion, the bf16 bracket, the table of cases with the launch path each is there for; tests/test_stem_ref.py: all of that
on its own, and the mutations the criterion catches):
  * ttk_stem_fwd: the band kernel (one band, several, a short band behind a full one, a second band per workgroup, static + dynamic LDS
    above 64 KB) and the gather kernel (one tile per wave, and a second through the prefetch), fp32 and bf16 storage; with and without
    `part`, with and without `pivot`;
  * ttk_stem_bwd_weight, GIVEN y as the float64 forward rounded once (bf16 storage: y and g rounded to bf16), at band heights 3, 4, 5, 6,
    7, 11 and 13, with a second tile per workgroup at height 7: accumulate = 1 into zeros, accumulate = 0 into NaN, accumulate = 1 onto a
    random dw0, and the scratch form with accumulate 0 and 1;
  * the refusals: a gradient of W >= 314, act_bf16 of 1 or 2, H or W of 4 - the message matches and every output is still NaN.
Every output starts as NaN (dw: NaN, zeros or dw0 as the form says) between two NaN guard bands of 64 elements, must be finite afterwards
and the bands untouched; every call runs twice on fresh buffers and repeats bit for bit (the atomic weight gradient need not).  Where the
float64 scale of an element is zero - the outputs of the all-zero image - the device value must be exactly +0.

Each output prints `RATIO <entry> <BxHxW> <form> <value>`, value = worst (|x - f64| - 2^-24 s) / (s Y) over its elements (conv_ref.py; a
bf16 forward output: stem_ref.bracket_ratio, and the assertion is the bracket); the assertion is value <= MARGIN = 4.

W = 394..402 forward (the band kernel's dynamic LDS is within the host's 64 KB, its 1 KB of static `red` lifts the sum to 65 632 - 66 560
bytes): the MI355X ACCEPTED the launch at W = 394, 398 and 402 (a gfx950 workgroup may hold up to the CU's 160 KB) and every element met
the criterion, ratios as at the narrower widths.  The host's size test is left as it is; stem_ref.fwd_form restates it.
Worst per entry point and form on the MI355X (profiles/stem_float64.txt has the cases):
    ttk_stem_fwd 0.79 (217x5x403: gather kernel, second tile), band kernel 0.77 (769x25x5); bf16 -0.04 (every stored value is the rounding of
    an accumulator inside the output's own float32 rounding of float64)
    ttk_stem_bwd_weight 0.45 in the forms onto zeros / NaN, atomic and scratch alike, 0.37 onto dw0 (2x5x6, band height 3); at the band
    heights 7 (second tile), 11 and 13 below 0.25; bf16 0.20 (769x25x5 atomic onto dw0), its scratch forms 0.03
The sequential chain over all pixels is the pessimistic order for the gradient, as expected: no gradient ratio reaches 1.  The sums are
within 0.03 of their tolerance everywhere.
"""
import functools
import types

import numpy as np
import pytest
import torch

import stem_ref as S

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 64
_ids = lambda v: "x".join(map(str, v))
BF16_FLAG = 3  # TTK_STORE_ACT_BF16 | TTK_STORE_GRAD_BF16
_STORAGE = [(s, False) for s in S.SHAPES] + [(s, True) for s in S.BF16_SHAPES]
_STORAGE_IDS = [_ids(s) + ("-bf16" if b else "-fp32") for s, b in _STORAGE]


class Guard:
    """Output buffers of one launch, each between two guard bands of GUARD NaNs (tests/test_conv_rows_gpu.py)"""

    def __init__(self):
        self.items = []

    def new(self, *shape, dtype=torch.float32):
        n = int(np.prod(shape))
        full = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device="cuda")
        self.items.append((full, n))
        return full[GUARD:GUARD + n].view(*shape)

    def like(self, init):
        """a guarded buffer that starts as `init` (None: NaN) - dw, which the entry point may accumulate onto"""
        v = self.new(S.C, S.TAPS)
        if init is not None:
            v.copy_(init)
        return v

    def check(self, what):
        torch.cuda.synchronize()
        for full, n in self.items:
            assert bool(torch.cat([full[:GUARD], full[GUARD + n:]]).isnan().all()), f"{what}: written outside a buffer of {n} elements"


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _lib():
    import trackertraincode._hip as hip
    return hip.lib(), hip.ptr


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _host(t):
    """float32 numpy of a device tensor; bf16 widened exactly"""
    if t.dtype == torch.bfloat16:
        return S.bf16_widen(t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16))
    return t.cpu().numpy()


def _form(shape, entry):
    f = S.facts(*shape)
    if entry == "fwd":
        if f["fwd_form"] == "gather":
            return "gather" + ("+2nd" if f["fwd_second_tile"] else "")
        return "band" + "/".join(map(str, sorted(set(f["fwd_band_heights"]), reverse=True))) + ("+2nd" if f["fwd_second_band"] else "")
    return f"rows{f['wgrad_rows']}" + ("+2nd" if f["wgrad_second_tile"] else "")


def _judge(entry, shape, form, p, out):
    out = np.asarray(out, np.float64)
    assert np.isfinite(out).all(), (entry, shape, "NaN left or written")
    ratio, zeros_ok = p.ratio(out)
    print("RATIO", entry, _ids(shape), form, f"{ratio:.3f}")
    assert zeros_ok, (entry, shape, "an element whose every product is zero is not exactly zero")
    if not ratio <= S.MARGIN:
        e = (np.abs(out - p.ref) - S.U * p.s) / np.where(p.s > 0, p.s * p.Y, np.inf)
        at = np.unravel_index(int(e.argmax()), e.shape)
        raise AssertionError((entry, shape, form, f"ratio {ratio:.2f} > {S.MARGIN} at element {at} of {out.shape}", f"Y {p.Y:.2e}"))
    return ratio


def _judge_bf16(entry, shape, form, p, stored):
    assert np.isfinite(stored).all(), (entry, shape, "NaN left or written")
    print("RATIO", entry, _ids(shape), form, f"{S.bracket_ratio(p, stored):.3f}")
    n = S.bracket_outside(p, stored)
    if n:
        lo, hi = S.bracket(p)
        at = np.argwhere((stored < lo) | (stored > hi) | ((p.s == 0) & (stored.view(np.uint32) != 0)))[0]
        raise AssertionError((entry, shape, form, f"{n} elements outside the bf16 bracket, first at {tuple(at)}",
                              float(lo[tuple(at)]), float(stored[tuple(at)]), float(hi[tuple(at)])))


@functools.lru_cache(maxsize=2)
def _device(shape, bf16):
    c = S.stem5_case(*shape, bf16=bf16)
    act = (lambda v: _t(v).to(torch.bfloat16)) if bf16 else _t  # exact: the case's g and y32 are bf16 values already
    return c, types.SimpleNamespace(x=_t(c.x), w=_t(c.w), piv=_t(c.piv), bn=_t(c.bn), g=act(c.g), y=act(c.y32), dw0=_t(c.dw0),
                                    act=torch.bfloat16 if bf16 else torch.float32, flag=BF16_FLAG if bf16 else 0)


def _check_sums(what, part, p, stored, piv, bf16):
    """stem_ref.sums_outside: against float64 of y - pivot (bf16 storage: of the stored value) and the squares of the stored values"""
    ps = part.cpu().numpy().astype(np.float64)
    assert np.isfinite(ps).all()  # every row below partial_rows_elementwise is written: idle workgroups write zeros
    own = stored.astype(np.float64) - piv.astype(np.float64)
    flat = own if bf16 else p.ref - piv.astype(np.float64)
    out = S.sums_outside(ps[:, 0].sum(0), ps[:, 1].sum(0), flat, own)
    print("SUMS", what, f"{out:.3f}")  # worst error / tolerance
    assert out <= 1.0, (what, out)


def _run_fwd(shape, bf16):
    L, p = _lib()
    c, d = _device(shape, bf16)
    form = _form(shape, "fwd")
    rows = L.partial_rows_elementwise(c.M * (S.C // 4))
    assert rows == S.facts(*shape)["fwd_grid"]

    def call(part=True, pivot=True):
        G = Guard()
        y, pt = G.new(c.M, S.C, dtype=d.act), (G.new(rows, 2, S.C) if part else None)
        L.call("ttk_stem_fwd", p(d.x), p(d.w), p(y), p(pt), p(d.piv) if pivot else None, c.B, c.H, c.W, d.flag)
        G.check("stem_fwd")
        return y, pt

    (y, part), (y2, part2) = call(), call()
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(part), _bits(part2))
    stored = _host(y)
    entry = "stem_fwd_bf16" if bf16 else "stem_fwd"
    if bf16:
        _judge_bf16(entry, shape, form, c.fwd, stored)
    else:
        _judge(entry, shape, form, c.fwd, stored)
    _check_sums(f"{entry} {_ids(shape)} pivot", part, c.fwd, stored, c.piv, bf16)
    y3, part3 = call(pivot=False)  # the sums are those of y
    assert torch.equal(_bits(y), _bits(y3))
    _check_sums(f"{entry} {_ids(shape)} no pivot", part3, c.fwd, stored, np.zeros(S.C, np.float32), bf16)
    y4, _ = call(part=False)  # eval: no sums
    assert torch.equal(_bits(y), _bits(y4))


@pytest.mark.parametrize("shape,bf16", _STORAGE, ids=_STORAGE_IDS)
def test_stem_fwd_rows(shape, bf16):
    _run_fwd(shape, bf16)


@pytest.mark.parametrize("W", [394, 398])
def test_stem_fwd_band_with_static_and_dynamic_lds_above_64k(W):
    """beside (1, 5, 402) of the table: the first width whose 1 KB of static LDS lifts the band kernel past 64 KB, and one in between"""
    f = S.facts(1, 5, W)
    assert f["fwd_form"] == "band" and f["fwd_lds"] > S.LDS_LIMIT
    _run_fwd((1, 5, W), False)


WGRAD_FORMS = [  # (name, accumulate, dw starts as, scratch)
    ("atomic_zeros", 1, "zeros", False),
    ("atomic_overwrite", 0, None, False),
    ("atomic_onto", 1, "dw0", False),
    ("scratch_overwrite", 0, None, True),
    ("scratch_onto", 1, "dw0", True),
]


@pytest.mark.parametrize("shape,bf16", [sb for sb in _STORAGE if S.wgrad_fits(sb[0][2])],
                         ids=[i for i, sb in zip(_STORAGE_IDS, _STORAGE) if S.wgrad_fits(sb[0][2])])
def test_stem_bwd_weight_rows(shape, bf16):
    L, p = _lib()
    c, d = _device(shape, bf16)
    form = _form(shape, "wgrad")
    nb = L.cdll.ttk_stem_wgrad_partial_bytes()
    grid = S.facts(*shape)["wgrad_grid"]
    assert nb >= 4 * S.C * S.TAPS * grid
    refs = {"zeros": c.wgrad, None: c.wgrad, "dw0": S.onto(c.wgrad, c.dw0)}
    for name, accumulate, start, use_scratch in WGRAD_FORMS:
        init = {"zeros": torch.zeros_like(d.dw0), None: None, "dw0": d.dw0}[start]
        runs = []
        for _ in range(2):
            G = Guard()
            dw = G.like(init)
            scratch = G.new(nb // 4) if use_scratch else None
            L.call("ttk_stem_bwd_weight", p(d.g), p(d.y), p(d.bn), p(d.x), p(dw), accumulate, p(scratch), c.B, c.H, c.W, d.flag)
            G.check("stem_bwd_weight " + name)
            if use_scratch:
                assert bool(torch.isfinite(scratch[:grid * S.C * S.TAPS]).all()), "a workgroup's row of the scratch was not written"
                assert bool(scratch[grid * S.C * S.TAPS:].isnan().all()), "scratch written past the grid's rows"
            runs.append(dw)
            _judge("stem_bwd_weight" + ("_bf16" if bf16 else ""), shape, form + ":" + name, refs[start], dw.cpu().numpy())
        if use_scratch:
            assert torch.equal(_bits(runs[0]), _bits(runs[1])), name  # folded in a fixed order


# ---- refusals: the message matches and every output is still NaN -------------------------------------------------------------------
def _refused_bwd(shape, flag, accumulate, use_scratch, match):
    L, p = _lib()
    B, H, W = shape
    Ho, Wo = S.out_hw(H, W)
    x, bn = torch.ones(B, H, W, device="cuda"), _t(S.bn_block(S.C, np.random.default_rng(1)))
    g, y = torch.ones(B * Ho * Wo, S.C, device="cuda"), torch.ones(B * Ho * Wo, S.C, device="cuda")  # large enough for either storage
    G = Guard()
    dw = G.like(None)
    scratch = G.new(L.cdll.ttk_stem_wgrad_partial_bytes() // 4) if use_scratch else None
    with pytest.raises(RuntimeError, match=match):
        L.call("ttk_stem_bwd_weight", p(g), p(y), p(bn), p(x), p(dw), accumulate, p(scratch), B, H, W, flag)
    G.check("refused stem_bwd_weight")
    assert bool(dw.isnan().all()) and (scratch is None or bool(scratch.isnan().all())), (shape, flag, accumulate, use_scratch)


def _refused_fwd(shape, flag, match):
    L, p = _lib()
    B, H, W = shape
    Ho, Wo = S.out_hw(H, W)
    x, w, piv = torch.ones(B, H, W, device="cuda"), torch.ones(S.C, S.TAPS, device="cuda"), torch.zeros(S.C, device="cuda")
    G = Guard()
    y, part = G.new(B * Ho * Wo, S.C), G.new(L.partial_rows_elementwise(B * Ho * Wo * (S.C // 4)), 2, S.C)
    with pytest.raises(RuntimeError, match=match):
        L.call("ttk_stem_fwd", p(x), p(w), p(y), p(part), p(piv), B, H, W, flag)
    G.check("refused stem_fwd")
    assert bool(y.isnan().all()) and bool(part.isnan().all()), (shape, flag)


@pytest.mark.parametrize("shape", [S.REFUSED_WIDTH, (1, 5, 393), (1, 5, 402), (1, 5, 403), (2, 9, 640)], ids=_ids)
def test_stem_bwd_weight_refuses_a_width_past_the_lds_band(shape):
    """... before anything is launched: accumulate = 0 without scratch zeroed dw first, until the checks moved above that launch"""
    assert not S.wgrad_fits(shape[2])
    for flag in (0, BF16_FLAG):
        for accumulate in (0, 1):
            for use_scratch in (False, True):
                _refused_bwd(shape, flag, accumulate, use_scratch, rf"stem_bwd_weight: image too wide for the LDS band \(W={shape[2]}\)")


@pytest.mark.parametrize("flag", [1, 2])
def test_stem_refuses_one_storage_bit_alone(flag):
    match = "the stem takes fp32 tensors or activations AND gradients bfloat16"
    _refused_fwd((2, 7, 9), flag, match)
    for accumulate in (0, 1):
        for use_scratch in (False, True):
            _refused_bwd((2, 7, 9), flag, accumulate, use_scratch, match)


@pytest.mark.parametrize("shape", [(1, 4, 5), (1, 5, 4), (2, 4, 4)], ids=_ids)
def test_stem_refuses_a_side_of_four(shape):
    for flag in (0, BF16_FLAG):
        _refused_fwd(shape, flag, "stem_fwd: bad shape")
        for accumulate in (0, 1):
            _refused_bwd(shape, flag, accumulate, False, "stem_bwd_weight: bad shape")
