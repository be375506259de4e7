"""The localizer's kernels one by one against tests/localizer_ref.py (float64): ttk_localizer_block at every (k, stride, residual)
combination and channel triple of the network on sizes that are odd and no multiple of any tile, and ttk_localizer_input."""
import numpy as np
import pytest
import torch

import localizer_ref as R
import trackertraincode._hip as H

pytestmark = pytest.mark.gpu

TRIPLES = [(8, 16, 12), (12, 48, 20), (20, 80, 20), (20, 40, 32), (56, 112, 56)]
KS = [(3, 1), (3, 2), (5, 2), (5, 1)]
SIZES = [(5, 7), (8, 8), (14, 18), (17, 19)]


def _block_params(rng, cin, cmid, cout, k):
    bn = lambda c: (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c), rng.normal(0, 0.3, c), rng.normal(0, 0.3, c), rng.uniform(0.5, 1.5, c))
    p = {"w1": rng.normal(0, cin ** -0.5, (cmid, cin, 1, 1)), "w2": rng.normal(0, 1.0 / k, (cmid, 1, k, k)),
         "w3": rng.normal(0, cmid ** -0.5, (cout, cmid, 1, 1)), "bn1": bn(cmid), "bn2": bn(cmid), "bn3": bn(cout)}
    # the parameters ARE float32 values, as a checkpoint's: the float64 yardstick and the kernel start from the same numbers
    return {n: (v.astype(np.float32) if isinstance(v, np.ndarray) else tuple(a.astype(np.float32) for a in v)) for n, v in p.items()}


def _run_block(x, packed, cin, cmid, cout, k, stride, residual):
    B, _, Hh, Ww = x.shape
    y = torch.full((B, cout, (Hh - 1) // stride + 1, (Ww - 1) // stride + 1), float("nan"), device="cuda")
    H.lib().call("ttk_localizer_block", H.ptr(x), H.ptr(packed), B, Hh, Ww, cin, cmid, cout, k, stride, int(residual), H.ptr(y))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("k,stride", KS)
@pytest.mark.parametrize("cin,cmid,cout", TRIPLES)
def test_block_against_float64(cin, cmid, cout, k, stride):
    """Criterion: the same unfused block (convolution, then BatchNorm) evaluated by torch on the CPU in float32 has an error e against
    float64; the kernel's may be 4 e (the folded BatchNorm and the different summation order, about one more rounding chain each), with
    a floor of 1e-6 max |value|.  The residual is added wherever the shapes allow it (Cin == Cout, stride 1)."""
    rng = np.random.default_rng(1000 * cin + 10 * k + stride)
    residual = cin == cout and stride == 1
    p = _block_params(rng, cin, cmid, cout, k)
    folded = R.fold_block(p)
    packed = R.pack(folded).cuda()
    worst = 0.0
    for Hh, Ww in SIZES:
        for B in (1, 3):
            x = rng.normal(0, 1, (B, cin, Hh, Ww)).astype(np.float32)
            y64 = R.block_forward(torch.from_numpy(x).double(), *folded, stride=stride, residual=residual)
            assert np.abs((R.block_unfused(torch.from_numpy(x).double(), p, stride, residual) - y64).numpy()).max() < 1e-12  # the fold itself
            e_cpu = float((R.block_unfused(torch.from_numpy(x), p, stride, residual).double() - y64).abs().max())
            y = _run_block(torch.from_numpy(x).cuda(), packed, cin, cmid, cout, k, stride, residual)
            assert y.shape == y64.shape and bool(torch.isfinite(y).all())
            e_gpu = float((y.cpu().double() - y64).abs().max())
            bound = max(4 * e_cpu, 1e-6 * float(y64.abs().max()))
            worst = max(worst, e_gpu / max(e_cpu, 1e-30))
            print(f"block {cin}->{cmid}->{cout} k{k} s{stride} {Hh}x{Ww} B{B}: kernel {e_gpu:.3e} cpu32 {e_cpu:.3e} ratio {e_gpu / max(e_cpu, 1e-30):.2f}")
            assert e_gpu <= bound, (Hh, Ww, B, e_gpu, e_cpu)
    print(f"block {cin}->{cmid}->{cout} k{k} s{stride}: worst ratio {worst:.2f}")


def test_block_two_runs_are_bitwise_equal():
    rng = np.random.default_rng(5)
    p = _block_params(rng, 20, 80, 20, 3)
    packed = R.pack(R.fold_block(p)).cuda()
    x = torch.from_numpy(rng.normal(0, 1, (3, 20, 28, 36)).astype(np.float32)).cuda()
    assert torch.equal(_run_block(x, packed, 20, 80, 20, 3, 1, True), _run_block(x, packed, 20, 80, 20, 3, 1, True))


@pytest.mark.parametrize("bad", ["k7", "stride3", "null", "channels", "residual"])
def test_block_refusals_write_nothing(bad):
    x = torch.zeros((1, 8, 6, 6), device="cuda")
    packed = torch.zeros(100000, device="cuda")
    y = torch.full((1, 12, 6, 6), 7.0, device="cuda")
    args = dict(x=H.ptr(x), p=H.ptr(packed), cin=8, cmid=16, cout=12, k=3, stride=1, res=0)
    args.update({"k7": dict(k=7), "stride3": dict(stride=3), "null": dict(p=None), "channels": dict(cmid=113),
                 "residual": dict(res=1)}[bad])  # (a residual with Cin != Cout)
    with pytest.raises(RuntimeError, match="localizer_block"):
        H.lib().call("ttk_localizer_block", args["x"], args["p"], 1, 6, 6, args["cin"], args["cmid"], args["cout"], args["k"], args["stride"],
                     args["res"], H.ptr(y))
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


def _input(frames, t_dev=None):
    S, T = frames.shape[:2]
    x = torch.full((S, 1, R.IN_H, R.IN_W), float("nan"), device="cuda")
    lb = torch.full((S, 3), float("nan"), device="cuda")
    H.lib().call("ttk_localizer_input", H.ptr(frames), int(frames.dtype == torch.uint8), S, T, frames.shape[2], frames.shape[3],
                 None if t_dev is None else H.ptr(t_dev), R.MUL, R.ADD, H.ptr(x), H.ptr(lb))
    torch.cuda.synchronize()
    return x, lb


@pytest.mark.parametrize("Hs,Ws", [(37, 41), (480, 640), (100, 300)])
def test_input_against_float64(Hs, Ws):
    """The area crop's own criterion: 5e-2 grey levels."""
    rng = np.random.default_rng(Hs)
    f = rng.integers(0, 256, (2, 1, Hs, Ws), dtype=np.uint8)
    x8, lb8 = _input(torch.from_numpy(f).cuda())
    x32, lb32 = _input(torch.from_numpy(f.astype(np.float32)).cuda())
    assert torch.equal(x8, x32) and torch.equal(lb8, lb32)
    worst = 0.0
    for q in range(2):
        ref, geo = R.letterbox(f[q, 0], R.MUL, R.ADD)
        worst = max(worst, float(np.abs(x8[q, 0].cpu().double().numpy() - ref).max()) / R.MUL)
        np.testing.assert_array_equal(lb8[q].cpu().numpy(), np.asarray(geo, dtype=np.float32))
    print(f"letterbox {Hs}x{Ws}: max error {worst:.3e} grey levels")
    assert worst <= 5e-2


def test_input_picks_the_frame_of_the_counter():
    rng = np.random.default_rng(9)
    f = torch.from_numpy(rng.integers(0, 256, (2, 3, 60, 80), dtype=np.uint8)).cuda()
    t = torch.tensor(1, dtype=torch.int32, device="cuda")
    x, lb = _input(f, t)
    want, _ = _input(f[:, 1:2].contiguous())
    assert torch.equal(x, want)
    assert torch.equal(_input(f)[0], _input(f[:, 0:1].contiguous())[0])  # no counter: frame 0
    for bad in (-1, 3):
        x, lb = _input(f, torch.tensor(bad, dtype=torch.int32, device="cuda"))
        assert bool(torch.isnan(x).all()) and bool(torch.isnan(lb).all())  # nothing is written
