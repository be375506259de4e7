"""tests/intensity_ref.py on its own, without a GPU:
  * the two facts that make the lattices decided (all 256 values of k/256 fall in the same bin under torch.histc, under the kernel's
    q fl32(256/255) and under the reference; trunc(fl32(fl32(L/255) 255)) == L for every level);
  * the integer path of equalize against a literal torch restatement of kornia's `_scale_channel` (torch.histc, cumsum, //, cat, clamp,
    gather on im.long(), / 255) in float32 and in float64, on every equalize image of every case;
  * the blur against conv2d in float64 of the F.pad(mode="reflect")-padded image with the outer product of the normalised weights, the
    elementwise steps and the whole chain against their torch float64 one-liners;
  * oracle.intensity.augment and the float32 emulation of intensity_ref inside the criterion on every case and both shifts, bitwise rules
    included (the `ORACLE` lines of a run with -s have the worst ratio per case: how tight the bound is);
  * zero undecided pixels in every case, and the arbitrary-float family clear at 8 ulp too;
  * coverage: every operation alone and every adjacent pair at every shape, the full chain, both `step` branches at their 254 | 255
    boundary, a clamped LUT, the pixel counts around the block size, the largest admitted images, the parameter edges;
  * sixteen planted errors in the float32 emulation, each more than 10x outside the criterion in a named case (`MUTATION` lines), and
    the corner error among them shown to pass the trimmed criterion of tests/test_intensity_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import intensity_ref as R
from oracle import intensity as O

F32 = np.float32
FAR = 10.0
LATTICE255 = ("u255", "ramp", "saturate")  # images on k/255: the float64 restatement takes them from the float64 lattice


def _t(a):
    return torch.from_numpy(np.array(a))


# ---------------------------------------------------------------------------------------------------------------------------------
# the lattices are decided
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_lattice_value_is_decided_the_same_way_by_histc_the_kernel_form_and_the_reference():
    k = np.arange(256)
    for denom in (256.0, 255.0):
        x = (k.astype(F32) / F32(denom)).astype(F32)
        s = x * F32(255.0)
        kernel_bin = np.minimum((s * F32(F32(256.0) / F32(255.0))).astype(np.int64), 255)
        ref_bin, inside, und = R.decide_bin(R.product255(_t(x)))
        assert bool(inside.all()) and not bool(und.any())
        assert np.array_equal(ref_bin.numpy(), kernel_bin)
        for i in k:  # one value at a time: torch.histc says where it went
            h = torch.histc(_t(s[i:i + 1]), bins=256, min=0, max=255)
            assert int(h.argmax()) == kernel_bin[i] and float(h.sum()) == 1.0
        idx, und = R.decide_index(R.product255(_t(x)))
        assert not bool(und.any()) and np.array_equal(idx.numpy(), s.astype(np.int64))
    level = (k.astype(F32) / F32(255.0)).astype(F32)
    assert np.array_equal((level * F32(255.0)).astype(np.int64), k)  # trunc(fl(fl(L / 255) 255)) == L
    assert np.array_equal(np.trunc((k / 255.0) * 255.0).astype(np.int64), k)  # and in float64


# ---------------------------------------------------------------------------------------------------------------------------------
# anchors
# ---------------------------------------------------------------------------------------------------------------------------------
def _scale_channel(im01):
    """kornia.enhance.equalize -> _scale_channel, literally, in the dtype of its argument"""
    im = im01 * 255
    histo = torch.histc(im, bins=256, min=0, max=255)
    nonzero_histo = histo[histo != 0]
    step = (nonzero_histo.sum() - nonzero_histo[-1]) // 255
    if step == 0:
        result = im
    else:
        lut = (torch.cumsum(histo, 0) + (step // 2)) // step
        lut = torch.cat([torch.zeros(1, dtype=lut.dtype), lut[:-1]])
        lut = torch.clamp(lut, 0, 255)
        result = torch.gather(lut, 0, im.flatten().long()).reshape_as(im)
    return result / 255


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_equalize_integer_path_equals_the_literal_scale_channel(name):
    x, p, _ = R.inputs(name)
    seen = 0
    for i, row in enumerate(R.CASES[name].rows):
        if not p[i, R.EQ] > 0 or (name == "b300" and i >= 43):
            continue
        seen += 1
        x32 = _t(x[i])
        level, und, info = R.equalize_levels(x32)
        lit32 = _scale_channel(x32)
        k = torch.round(x32.double() * 255.0)
        x64 = k / 255.0 if row.kind in LATTICE255 else x32.double()
        if row.kind in LATTICE255:
            assert torch.equal(x64.float(), x32)
        lit64 = _scale_channel(x64)
        if level is None:
            assert info["step"] == 0
            assert torch.equal(lit32, (x32 * 255.0) / 255.0)
            assert float((lit64 - x64).abs().max()) <= 2.0 ** -52
            if row.kind != "arb":
                assert torch.equal(lit32, x32), "on the lattices kornia's round trip is the identity"
        else:
            assert info["step"] > 0
            assert torch.equal(lit32, level.float() / torch.tensor(255.0))
            assert torch.equal(lit64, level.double() / 255.0)
    assert seen or not (p[:, R.EQ] > 0).any()


def _blur_conv2d(v):
    g = R.weights64()
    pad = F.pad(v[None, None], (2, 2, 2, 2), mode="reflect")
    return F.conv2d(pad, torch.outer(g, g)[None, None])[0, 0]


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_blur_equals_conv2d_of_the_reflect_padded_image(shape):
    for kind in ("arb", "smooth"):
        v = _t(R.image(kind, *shape, 5)).double()
        got, e = R.blur_stage(v, torch.zeros_like(v))
        assert float((got - _blur_conv2d(v)).abs().max()) <= 25 * 2.0 ** -53  # two orders of summing 25 products of size <= 1
        assert float(e.min()) > 0 and float(e.max()) <= 2 * (R.K_W + 5.0) * R.U * 1.0001
    g = R.weights64()
    assert abs(float(g.sum()) - 1.0) <= 1e-15 and torch.equal(g, g.flip(0))
    assert abs(float(g[1] / g[2]) - np.exp(-1 / 4.5)) <= 1e-15 and abs(float(g[0] / g[2]) - np.exp(-4 / 4.5)) <= 1e-15


def test_elementwise_stages_equal_their_torch_one_liners():
    g = torch.Generator().manual_seed(3)
    v = torch.rand(37, 41, generator=g, dtype=torch.float64)
    z = torch.zeros_like(v)
    n = torch.randn(37, 41, generator=g, dtype=torch.float64)
    for gamma in (0.5, 1.0, 2.0):
        assert torch.equal(R.gamma_stage(v, z, gamma)[0], torch.clamp(torch.pow(v, gamma), 0, 1))
        assert torch.equal(R.gamma_stage(v, z, gamma)[1], R.P_POWF * R.U * torch.pow(v, gamma))
    e = torch.full_like(v, 1e-6)
    spread = R.gamma_stage(v, e, 0.5)[1] - R.P_POWF * R.U * v.sqrt()
    assert bool((spread >= (v.sqrt() - (v - e).clamp(min=0).sqrt()).abs() - 1e-18).all())
    for f in (0.7, 1.5):
        assert torch.equal(R.contrast_stage(v, z, f)[0], torch.clamp(v * f, 0, 1))
        assert torch.equal(R.brightness_stage(v, z, f)[0], torch.clamp(v + (f - 1.0), 0, 1))
    assert torch.equal(R.noise_stage(v, z, 0.25, n)[0], v + 0.25 * n)
    assert torch.equal(R.shift_stage(v + n, z, -0.5)[0], torch.clamp(v + n, 0, 1) - 0.5)
    assert torch.equal(R.level_stage(torch.arange(256))[0], torch.arange(256).double() / 255.0)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_chain_equals_the_torch_float64_chain(name):
    """the whole chain restated in torch float64 one-liners, the quantising steps through the literal float32 kornia forms"""
    x, p, noise = R.inputs(name)
    for i, ref in enumerate(R.reference(name)):
        if name == "b300" and i >= 43:
            break
        q = [float(a) for a in p[i]]
        x32 = _t(x[i])
        v32 = _scale_channel(x32) if q[R.EQ] > 0 else x32
        bits = int(q[R.BITS])
        if 0 < bits < 8:  # kornia.enhance.posterize: uint8(im 255) shifted right and left again
            v32 = (((v32 * 255).to(torch.uint8) >> (8 - bits)) << (8 - bits)).float() / 255
        if ref.info["step"] == 0 and not 0 < bits < 8:
            v = x32.double()  # the kernel leaves the image alone; kornia's round trip is the identity on the lattices (asserted above)
        elif q[R.EQ] > 0 or 0 < bits < 8:
            v = torch.round(v32.double() * 255.0) / 255.0  # the level, as a float64 quotient
            assert torch.equal(v.float(), v32)
        else:
            v = v32.double()
        if q[R.GAMMA] > 0:
            v = torch.clamp(torch.pow(v, q[R.GAMMA]), 0, 1)
        if q[R.CONTRAST] > 0:
            v = torch.clamp(v * q[R.CONTRAST], 0, 1)
        if q[R.BRIGHT] > 0:
            v = torch.clamp(v + (q[R.BRIGHT] - 1.0), 0, 1)
        if q[R.BLUR] > 0:
            v = _blur_conv2d(v)
        if q[R.NOISE] > 0:
            v = v + q[R.NOISE] * _t(noise[i]).double()
        for shift in R.SHIFTS:
            f64, e, _ = R.finish(ref, shift)
            assert np.abs(f64 - (torch.clamp(v, 0, 1) + shift).numpy()).max() <= 25 * 2.0 ** -53, (name, i)
            assert np.isfinite(e).all() and e.min() >= 0 and e.max() < 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# the inputs leave nothing undecided; the float32 restatements are inside the criterion
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_no_pixel_of_any_case_is_undecided(name):
    x, p, noise = R.inputs(name)
    assert x.min() >= 0.0 and np.isfinite(x).all()
    for i, ref in enumerate(R.reference(name)):
        assert int(ref.undecided.sum()) == 0, (name, i)
        if R.CASES[name].rows[i].kind == "arb" and (name != "b300" or i < 43):  # by construction clear at 8 ulp as well
            assert int(R.reference_image(x[i], p[i], noise[i], ulps=8.0).undecided.sum()) == 0
            q = R.product255(_t(x[i]))
            assert not bool(R.near(q, 8.0).any()) and not bool(R.decide_bin(q, 8.0)[2].any())
            assert not bool((q == torch.round(q)).any()), "the arbitrary family is off the lattices"


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_float32_restatements_meet_the_criterion(name):
    x, p, noise = R.inputs(name)
    for shift in R.SHIFTS:
        for what, fn in (("oracle", O.augment), ("emulation", R.emulate)):
            worst, broken = R.judge(name, fn(x, p, noise, shift), shift)
            print("ORACLE", what, name, shift, f"{worst.max():.3f}", R.CASES[name].rows[int(worst.argmax())].name)
            assert worst.max() <= 1.0, (what, name, shift, R.CASES[name].rows[int(worst.argmax())])
            assert not broken, (what, name, shift, "bitwise rule", broken[:8])
    # the rules apply where they should
    for ref, row, q in zip(R.reference(name), R.CASES[name].rows, p):
        ops = R.active_ops(q)
        off_lattice_identity = row.kind == "arb" and ops == ("eq",) and ref.info["step"] == 0  # kornia's round trip moves it by <= 1 ulp
        assert (ref.exact is not None) == (set(ops) <= {"eq", "post"} and not off_lattice_identity), (name, row)


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------------------
def test_tables_cover_what_they_claim():
    pixels = {h * w for h, w in R.SHAPES}
    assert {9, 255, 256, 258, 129 * 129} <= pixels and min(min(s) for s in R.SHAPES) == 3
    assert R.max_pixels() == 20216 and 142 * 142 <= 20216 and 141 * 143 <= 20216 < 143 * 142
    assert (142, 142) in R.SHAPES and (141, 143) in R.SHAPES and (143, 142) in R.REFUSED
    assert all((w, h) in R.SHAPES for h, w in R.SHAPES if h != w and h * w not in (255, 258, 141 * 143))
    pairs = {(a, b) for a, b in zip(R.CHAIN, R.CHAIN[1:])}
    for h, w in R.SHAPES:
        x, p, _ = R.inputs(f"{h}x{w}")
        ops = [R.active_ops(q) for q in p]
        assert {(o,) for o in R.CHAIN} <= set(ops) and pairs <= set(ops) and R.CHAIN in ops and () in ops
        if h != w:  # content that differs along rows and along columns: an H / W exchange shows
            for im, row in zip(x, R.CASES[f"{h}x{w}"].rows):
                assert im.std(axis=0).max() > 0 and im.std(axis=1).max() > 0, row
    assert {len(R.CASES[n].rows) for n in ("b1", "b2", "b300")} == {1, 2, 300}
    every = np.concatenate([R.inputs(n)[1] for n in R.CASE_NAMES])
    assert set(every[:, R.BITS].astype(int)) == {0, 1, 4, 7, 8, 9}
    assert {0.5, 1.0, 2.0} <= set(every[:, R.GAMMA].tolist())
    for slot in (R.CONTRAST, R.BRIGHT):
        assert {float(F32(0.7)), 1.5} <= set(every[:, slot].tolist())
    assert {float(F32(4 / 255)), float(F32(64 / 255))} <= set(every[:, R.NOISE].tolist())
    # both branches of `step`, at the boundary, on the planted images; a LUT that passes 255 and is clamped
    for name, hw in (("special16x16", 256), ("special31x47", 31 * 47)):
        info = {row.kind: ref.info for row, ref in zip(R.CASES[name].rows, R.reference(name)) if row.name == "eq"}
        assert (info["step0"]["rest"], info["step0"]["step"]) == (254, 0) and (info["step1"]["rest"], info["step1"]["step"]) == (255, 1)
        assert info["flat"]["step"] == 0 and info["zero"]["step"] == 0 and info["one"]["step"] == 0
        x = R.inputs(name)[0]
        kinds = [r.kind for r in R.CASES[name].rows]
        assert (x[kinds.index("block1")][:4, :4] == 1.0).all() and len(np.unique(x[kinds.index("two")])) == 2
        assert len(np.unique(x[kinds.index("ramp")])) == 256
    assert info["saturate"]["lut_max"] > 255 and info["saturate"]["step"] > 1 and info["ramp"]["step"] >= 1
    steps = {ref.info["step"] for n in R.CASE_NAMES for ref in R.reference(n)}
    assert {0, 1} <= steps and max(s for s in steps if s is not None) > 64
    small = [ref.info["step"] for n in ("3x3", "3x64", "64x3", "5x51") for ref in R.reference(n) if ref.info["step"] is not None]
    assert small and set(small) == {0}  # fewer than 256 pixels: always the step == 0 branch


# ---------------------------------------------------------------------------------------------------------------------------------
# planted errors
# ---------------------------------------------------------------------------------------------------------------------------------
PLANTED = [  # (number in the list of the module docstring's last item, mutation, case, shift, a case where it is truly a no-op or None)
    (1, "edge_repeat", "3x3", 0.0, None),
    (2, "symmetric", "64x3", 0.0, None),
    (3, "corners", "142x142", -0.5, None),
    (4, "swap_hw", "31x47", 0.0, "16x16"),
    (5, "bin_floor", "129x129", 0.0, "5x51"),
    (6, "lut_unshifted", "31x47", -0.5, "5x51"),
    (7, "step_total", "special31x47", 0.0, None),
    (8, "post_round", "edges31x47", 0.0, None),
    (9, "post_low", "3x64", -0.5, None),
    (10, "bright_mul", "3x86", 0.0, None),
    (11, "contrast_mean", "5x51", 0.0, None),
    (12, "no_clamp", "edges47x31", 0.0, "47x31"),
    (13, "noise_first", "47x31", -0.5, None),
    (14, "shift_first", "3x3", -0.5, None),
    (15, "sigma1", "141x143", 0.0, None),
    (15, "unnormalised", "64x3", 0.0, None),
    (16, "neighbour", "b2", 0.0, "b1"),
]


@pytest.mark.parametrize("number,mut,name,shift,noop", PLANTED, ids=[m[1] for m in PLANTED])
def test_planted_error_lands_far_outside_the_criterion(number, mut, name, shift, noop):
    x, p, noise = R.inputs(name)
    worst, _ = R.judge(name, R.emulate(x, p, noise, shift, mut), shift)
    clean, _ = R.judge(name, R.emulate(x, p, noise, shift), shift)
    print("MUTATION", number, mut, name, shift, f"{worst.max():.3g}", R.CASES[name].rows[int(worst.argmax())].name, f"(clean {clean.max():.3f})")
    assert clean.max() <= 1.0 and worst.max() > FAR
    if noop is not None:  # where the planted error changes nothing the emulation repeats its bits
        x, p, noise = R.inputs(noop)
        assert np.array_equal(R.emulate(x, p, noise, shift, mut), R.emulate(x, p, noise, shift))


def test_corner_error_passes_the_trimmed_criterion_and_fails_the_new_one():
    """The four corners of every blurred image judged under the trim alone, set to what an edge-repeating border gives: the criterion of
    test_kernel_matches_oracle_on_explicit_parameters (fewer than 1e-4 of the pixels beyond 2e-6) accepts it at its own inputs."""
    import test_intensity_gpu as T

    B, H, W = 48, 129, 129
    x, prm = T._images(B, H, W, 3), T._params(B, 4)
    noise = np.random.default_rng(5).standard_normal((B, H, W)).astype(F32)
    prm[:8] = 0
    ref = O.augment(x, prm, noise, out_shift=-0.5)
    got = R.emulate(x, prm, noise, -0.5, "corners")
    blurred = int((prm[:, O.BLUR] > 0).sum())
    bad = np.abs(got - ref) > 2e-6
    assert blurred >= 8 and bad.sum() >= 2 * blurred and bad.mean() < 1e-4  # accepted
    x, p, noise = R.inputs("142x142")
    worst, _ = R.judge("142x142", R.emulate(x, p, noise, -0.5, "corners"), -0.5)
    rows = [r.name for r, w in zip(R.CASES["142x142"].rows, worst) if w > FAR]
    assert rows == [r.name for r in R.CASES["142x142"].rows if "blur" in r.name or r.name.startswith("full")]
