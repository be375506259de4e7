"""The fused intensity augmentation (ttk_intensity_augment, csrc/intensity.hip) through the C ABI, pixel by pixel against float64
(tests/intensity_ref.py: the reference, the bound carried beside it, the criterion, the bitwise rules and the tables of cases;
tests/test_intensity_ref.py: all of that without a GPU, and the sixteen planted errors the criterion catches).
  * every case of the table at out_shift 0 and -0.5: |x - f64| <= 4 e + 2^-24 |f64| on EVERY pixel, no pixel left out; exact levels and
    untouched images bit for bit;
  * every output starts as NaN between two bands of a sentinel value, and the bands must be untouched;
  * NaN in parameter slot 7 and a NaN-filled noise tensor under std == 0 change no bit; noise == NULL under std > 0 gives the bits of
    std == 0 and meets the criterion of the chain without noise;
  * in place == out of place, a second call and an image at positions 0, B/2 and B - 1 among different neighbours: the same bits;
  * refusals (143 x 142, H = 2, W = 2, B = 0, null x / y / params) raise and leave the output untouched;
  * KorniaImageDistortions.apply on [B, 1, H, W] and on a non-contiguous view: the bits of the direct call.
Each case prints `RATIO <case> <shift> <row> <kernel> <oracle>`: the worst |x - f64| / (4 e + 2^-24 |f64|) of the kernel (asserted <= 1) and
of the float32 oracle on the same image, and the gamma-only rows `POWF <case> <row> <worst |x - f64| / (u v^g)>` (the bound takes 16).
Figures of the MI355X: profiles/intensity_float64.txt."""
import numpy as np
import pytest
import torch

import intensity_ref as R
from oracle import intensity as O

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENTINEL, FRONT, BACK = -24680.0, 64, 4096


def _lib():
    import trackertraincode._hip as hip
    return hip.lib(), hip.ptr


def _t(x):
    return torch.from_numpy(np.array(x)).cuda()


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


def _call(x, y, prm, noise, shift):
    L, p = _lib()
    B, H, W = x.shape
    L.call("ttk_intensity_augment", p(x), p(y), p(prm), p(noise), B, H, W, shift)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_intensity_pixels(name):
    x, prm, noise = R.inputs(name)
    dx, dn = _t(x), _t(noise)
    prm7 = prm.copy()
    prm7[:, R.SLOT7] = NAN  # the unused slot: read by nobody
    dp, dp7 = _t(prm), _t(prm7)
    quiet = _t(np.where((prm[:, R.NOISE] > 0)[:, None, None], noise, np.float32(NAN)).astype(np.float32))  # NaN where std == 0
    rows = R.CASES[name].rows
    bad = []
    for shift in R.SHIFTS:
        B = Bands()
        y, y2, y7, yq, yin = B.new(*x.shape), B.new(*x.shape), B.new(*x.shape), B.new(*x.shape), B.new(*x.shape, like=dx)
        _call(dx, y, dp, dn, shift)
        _call(dx, y2, dp, dn, shift)
        _call(dx, y7, dp7, dn, shift)
        _call(dx, yq, dp, quiet, shift)
        _call(yin, yin, dp, dn, shift)
        B.check(name)
        got = y.cpu().numpy()
        if not np.isfinite(got).all():
            bad.append((shift, "NaN left or written"))
            continue
        for what, other in (("a second call", y2), ("NaN in slot 7", y7), ("NaN noise under std == 0", yq), ("in place", yin)):
            if not torch.equal(_bits(y), _bits(other)):
                bad.append((shift, what, "not bit for bit the same"))
        worst, broken = R.judge(name, got, shift)
        oracle, _ = R.judge(name, O.augment(x, prm, noise, shift), shift)
        seen = set()
        for i in np.argsort(-worst):  # the worst image of every row name first
            label = f"{rows[i].name}/{rows[i].kind}".replace(" ", "_")
            if label not in seen:
                seen.add(label)
                print("RATIO", name, shift, label, f"{worst[i]:.3f} {oracle[i]:.3f}")
        if not worst.max() <= 1.0:
            i = int(worst.argmax())
            bad.append((shift, rows[i], f"image {i}: worst error {worst[i]:.3g} x the allowance"))
        if broken:
            bad.append((shift, "bitwise rule broken by images", broken[:8], [rows[i] for i in broken[:3]]))
        if shift == 0.0:
            for i, ref in enumerate(R.reference(name)):
                if R.active_ops(prm[i]) == ("gamma",):
                    w = ref.v.numpy()  # v^g, clamped: the clamp does not bind on [0, 1]
                    with np.errstate(divide="ignore", invalid="ignore"):
                        r = np.where(w > 0, np.abs(got[i] - w) / (R.U * w), np.where(got[i] == 0, 0.0, np.inf))
                    print("POWF", name, f"{rows[i].name}/{rows[i].kind}", f"{r.max():.3f}")
    # noise == NULL with std > 0: the result without noise
    shift = R.SHIFTS[1]
    B = Bands()
    y0, y0b = B.new(*x.shape), B.new(*x.shape)
    prm0 = prm.copy()
    prm0[:, R.NOISE] = 0
    _call(dx, y0, dp, None, shift)
    _call(dx, y0b, _t(prm0), dn, shift)
    B.check(name + ", noise = NULL")
    if not torch.equal(_bits(y0), _bits(y0b)):
        bad.append(("noise = NULL", "not the bits of std == 0"))
    ref0 = [R.finish(R.reference_image(x[i], prm0[i], None), shift) if prm[i, R.NOISE] > 0 else R.finish(r, shift)
            for i, r in enumerate(R.reference(name))]
    got0 = y0.cpu().numpy()
    w0 = np.array([R.ratios(got0[i], f64, e).max() for i, (f64, e, _) in enumerate(ref0)])
    print("RATIO", name, shift, "noise=NULL", f"{w0.max():.3f} -")
    if not w0.max() <= 1.0:
        bad.append(("noise = NULL", rows[int(w0.argmax())], f"{w0.max():.3g} x the allowance"))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", ["47x31", "b300", "141x143"])
def test_intensity_output_does_not_depend_on_the_image_position(name):
    """one image and its parameters at positions 0, B / 2 and B - 1 of a batch of otherwise different images and parameters"""
    x, prm, noise = (a.copy() for a in R.inputs(name))
    n = x.shape[0]
    src, spots = 1, (0, n // 2, n - 1)
    prm[src] = R.FULL2
    for s in spots:
        x[s], prm[s], noise[s] = x[src], prm[src], noise[src]
    B = Bands()
    y = B.new(*x.shape)
    _call(_t(x), y, _t(prm), _t(noise), -0.5)
    B.check(name)
    assert bool(torch.isfinite(y).all())
    for s in spots[1:]:
        assert torch.equal(_bits(y[s]), _bits(y[spots[0]])), (name, s)
    f64, e, _ = R.finish(R.reference_image(x[src], prm[src], noise[src]), -0.5)
    assert R.ratios(y[0].cpu().numpy(), f64, e).max() <= 1.0


def test_intensity_refusals_raise_and_leave_the_output_untouched():
    L, p = _lib()
    x, prm, noise = R.inputs("47x31")
    dx, dp = _t(x), _t(prm)
    B = Bands()
    y = B.new(2, 143 * 142)
    before = _bits(y).clone()
    for what, args in (("143x142", (p(dx), p(y), p(dp), None, 1, 143, 142, 0.0)), ("H = 2", (p(dx), p(y), p(dp), None, 2, 2, 5, 0.0)),
                       ("W = 2", (p(dx), p(y), p(dp), None, 2, 5, 2, 0.0)), ("B = 0", (p(dx), p(y), p(dp), None, 0, 47, 31, 0.0)),
                       ("x = NULL", (None, p(y), p(dp), None, 2, 47, 31, 0.0)), ("y = NULL", (p(dx), None, p(dp), None, 2, 47, 31, 0.0)),
                       ("params = NULL", (p(dx), p(y), None, None, 2, 47, 31, 0.0))):
        with pytest.raises(RuntimeError, match="LDS" if what == "143x142" else "bad arguments"):
            L.call("ttk_intensity_augment", *args)
        B.check(what)
        assert torch.equal(_bits(y), before), what
    assert (143, 142) in R.REFUSED and 143 * 142 > R.max_pixels()
    _call(dx[:2], y[:, :47 * 31].contiguous().view(2, 47, 31), dp, None, 0.0)  # and the entry point still works afterwards
    torch.cuda.synchronize()


def test_host_wrapper_gives_the_bits_of_the_direct_call():
    import trackertraincode.datatransformation as dtr

    name = "47x31"
    x, prm, noise = R.inputs(name)
    dx, dp, dn = _t(x), _t(prm), _t(noise)
    B = Bands()
    y = B.new(*x.shape)
    _call(dx, y, dp, dn, -0.5)
    B.check(name)
    chain = dtr.batch.KorniaImageDistortions(dtr.batch.RandomEqualize(p=1.0), dtr.batch.OnlyClip(p=1.0), out_shift=-0.5)
    out = chain.apply(dx[:, None], torch.from_numpy(prm.copy()), dn)
    assert out.shape == (x.shape[0], 1, 47, 31) and torch.equal(_bits(out[:, 0]), _bits(y))
    wide = torch.full((x.shape[0], 1, 47, 40), NAN, device="cuda")
    wide[..., 3:34] = dx[:, None]
    view = wide[..., 3:34]
    assert not view.is_contiguous()
    out2 = chain.apply(view, dp, dn)
    assert torch.equal(_bits(out2[:, 0]), _bits(y))
    assert torch.equal(_bits(view[:, 0]), _bits(dx)) and bool(torch.isnan(wide[..., :3]).all()) and bool(torch.isnan(wide[..., 34:]).all())
    out3 = chain.apply(dx, dp, dn)  # [B, H, W]
    assert torch.equal(_bits(out3), _bits(y))
