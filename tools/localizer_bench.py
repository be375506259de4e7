#!/usr/bin/env python3
"""Measurements of the face localizer's inference path (csrc/localizer.hip) on the MI355X; the output is kept in profiles/localizer.txt.

    python tools/localizer_bench.py [--batches 1 16 256] [--passes 3] [--skip-closed-loop] [--frames 1000] [--out profiles/localizer.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/localizer_bench.py --target     (the per-kernel table, a run of its own)

Sections (host clock around work that ends in a synchronise, every leg warmed up):
  localize     `eval.Localizer.localize` on 480 x 640 uint8 frames resident in HBM at every batch size: frames per second, `passes` passes
  torch        the same module's forward through torch's own device convolutions (the module's plain-torch ops applied to device
               tensors) on the same weights and batch sizes - an outside yardstick; reported as unavailable if they do not run
  blocks       every inverted-residual block alone (ttk_localizer_block, device events, at the largest batch size) next to its algorithmic
               bytes: input + output + parameters
  closed loop  the 1000-frame set-up of tools/closed_loop_bench.py: ms per frame eager and graphed, without and with the localizer
--target runs 20 forwards at the largest batch size and nothing else (what the profiler traces)."""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "neuralnet-tracker-traincode_amd"))
import trackertraincode._hip as H  # noqa: E402
from trackertraincode import eval as E  # noqa: E402
from trackertraincode.neuralnets.models import LocalizerNet, NetworkWithPointHead  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def torch_forward(net, x):
    """LocalizerNet.forward's plain-torch branch on device tensors (torch's own convolutions)."""
    z = net.convnet(x)
    m = torch.softmax(z[:, 1].reshape(z.shape[0], -1), dim=1).view(-1, 7, 9)
    mean, std = net.boxstddev(m)
    return torch.cat([z[:, 0].mean(dim=[1, 2])[:, None], mean - std, mean + std], dim=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--skip-closed-loop", action="store_true", default=False)
    ap.add_argument("--target", action="store_true", default=False)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the MI355X")
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    torch.manual_seed(0)
    net = LocalizerNet().cuda().eval()  # (the time does not depend on the weights)
    loc = E.Localizer(net)
    g = torch.Generator().manual_seed(0)
    Bmax = max(args.batches)
    frames = torch.randint(0, 256, (Bmax, 480, 640), dtype=torch.uint8, generator=g).cuda()
    if args.target:
        x = torch.randn(Bmax, 1, 224, 288, device="cuda")
        with torch.no_grad():
            for _ in range(20):
                net(x)
        torch.cuda.synchronize()
        return
    say(f"# tools/localizer_bench.py on {torch.cuda.get_device_name(0)}; {H.lib().cdll.ttk_localizer_launches()} launches per forward")
    say("## Localizer.localize, 480 x 640 uint8 frames resident in HBM")
    for B in args.batches:
        reps = max(3, min(200, 2000 // B))
        loc.localize(frames[:B])
        fps = []
        for _ in range(args.passes):
            dt, _ = timed(lambda: [loc.localize(frames[:B]) for _ in range(reps)])
            fps.append(B * reps / dt)
        say(f"B = {B:4d}: " + ", ".join(f"{v:10.0f}" for v in fps) + f" frames/s ({1e3 * B / max(fps):.3f} ms per batch at best)")
    say("## the module's forward alone: HIP path against torch's own device convolutions, ms per batch")
    for B in args.batches:
        x = torch.randn(B, 1, 224, 288, device="cuda")
        reps = max(3, min(200, 2000 // B))
        with torch.no_grad():
            net(x)
            ours = min(timed(lambda: [net(x) for _ in range(reps)])[0] for _ in range(args.passes)) / reps
            try:
                ref = torch_forward(net, x)
                theirs = min(timed(lambda: [torch_forward(net, x) for _ in range(reps)])[0] for _ in range(args.passes)) / reps
                dev = float((ref - net(x)).abs().max())
                say(f"B = {B:4d}: HIP {1e3 * ours:8.3f}   torch {1e3 * theirs:8.3f}   (max |difference of the outputs| {dev:.2e})")
            except Exception as e:  # noqa: BLE001
                say(f"B = {B:4d}: HIP {1e3 * ours:8.3f}   torch: unavailable on this box ({type(e).__name__}: {str(e)[:120]})")
    say(f"## every block alone at B = {Bmax}: microseconds, algorithmic bytes (input + output + parameters), GB/s")
    Hh, Ww = 112, 144
    for i, (cin, cout, k, s, e) in enumerate(LocalizerNet.BLOCKS):
        cmid, Ho, Wo = cin * e, (Hh - 1) // s + 1, (Ww - 1) // s + 1
        nparam = cmid * cin + 2 * cmid + cmid * k * k + cout * cmid + cout
        x, p = torch.randn(Bmax, cin, Hh, Ww, device="cuda"), torch.randn(nparam, device="cuda")
        y = torch.empty(Bmax, cout, Ho, Wo, device="cuda")
        run = lambda: H.lib().call("ttk_localizer_block", H.ptr(x), H.ptr(p), Bmax, Hh, Ww, cin, cmid, cout, k, s, int(cin == cout and s == 1), H.ptr(y))
        run()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = 1e9
        for _ in range(args.passes):
            a.record()
            for _ in range(5):
                run()
            b.record()
            torch.cuda.synchronize()
            best = min(best, a.elapsed_time(b) / 5)
        nbytes = 4 * (x.numel() + y.numel() + nparam)
        say(f"block {i:2d} {cin:3d}->{cmid:3d}->{cout:3d} k{k} s{s} {Hh:3d}x{Ww:3d}: {1e3 * best:9.1f} us {nbytes / 1e6:9.2f} MB {nbytes / best / 1e6:8.1f} GB/s")
        Hh, Ww = Ho, Wo
    if not args.skip_closed_loop:
        say(f"## closed loop, {args.frames} frames of 480 x 640, factors (1.0, 1.2), full-size pose network: ms per frame")
        video = torch.randint(0, 256, (args.frames, 480, 640), dtype=torch.uint8, generator=g).cuda()
        first = torch.tensor([[320.0 - 96, 240.0 - 96, 320.0 + 96, 240.0 + 96]])
        pose = NetworkWithPointHead(enable_point_head=True, enable_uncertainty=False).cuda().eval()
        for name, kw in (("without localizer", {}), ("with localizer   ", {"localizer": net})):
            for graphed in (False, True):
                trk = E.ClosedLoopTracker(pose, graphed=graphed, **kw)
                trk.track(video[:8], first)
                ms = [1e3 * timed(lambda: trk.track(video, first))[0] / args.frames for _ in range(args.passes)]
                say(f"{name} {'graphed' if graphed else 'eager  '}: " + ", ".join(f"{v:7.3f}" for v in ms))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
