#!/usr/bin/env python3
"""Frames per second of closed-loop tracking (scripts/evaluate_stability.py closed-loop) at a user-sized case: a full-size mobilenetv1
with the landmark head, one video of T = 1000 frames of 480 x 640 uint8 resident in HBM, crop factors (1.0, 1.2).

    python tools/closed_loop_bench.py [--frames 1000] [--height 480] [--width 640] [--factors 1.0 1.2] [--reps 3] [--json out.json]

Three legs, every one warmed up, alternating inside one process, `reps` times each; host clock around work that ends in a synchronise:
  (a) loop    : the reference's loop (scripts/evaluate_stability.py:248-264) over `Predictor.predict_batch`, one predictor and one pass
                over the video per factor, batch 1, the predicted box read back with .cpu() and clamped on the host every frame
                (boxes that fail the tracker's validity rule are not taken over, so that both sides crop the same frames)
  (b) eager   : eval.ClosedLoopTracker(net, factors).track(frames, first_roi): all factors as lanes, no host read until the end
  (c) graphed : the same with graphed=True: one warm-up frame, one capture, T replays (both inside the timed call)
Frames per second count video frames (all factors tracked); ms per frame likewise.  The trajectory of (c) must equal that of (b)
bitwise; the check is printed.  Prints one JSON line at the end."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "neuralnet-tracker-traincode_amd"))
from trackertraincode import eval as E  # noqa: E402
from trackertraincode.neuralnets.models import NetworkWithPointHead  # noqa: E402


def loop_pass(predictors, frames, first, factors):
    """The parent commit's way.  frames [T,1,H,W] on the device; returns the boxes each frame was cropped with, per factor."""
    T, _, H, W = frames.shape
    out = []
    for p, f in zip(predictors, factors):
        roi, used = first.clone(), []
        for t in range(T):
            used.append(roi)
            pred = p.predict_batch(frames[t:t + 1], roi[None])
            x0, y0, x1, y1 = (float(v) for v in pred["roi"][0].cpu())
            c = [max(0.0, x0), max(0.0, y0), min(x1, float(W)), min(y1, float(H))]
            if all(np.isfinite([x0, y0, x1, y1])) and c[2] - c[0] > 0 and c[3] - c[1] > 0 and max(c[2] - c[0], c[3] - c[1]) * f >= 2:
                roi = torch.tensor(c, dtype=torch.float32)
        out.append(torch.stack(used))
    return torch.stack(out, 1)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--factors", type=float, nargs="+", default=[1.0, 1.2])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-graphed", action="store_true", default=False)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the MI355X")
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (args.frames, args.height, args.width), dtype=torch.uint8, generator=g).cuda()
    half = 0.2 * min(args.height, args.width)
    first = torch.tensor([0.5 * args.width - half, 0.5 * args.height - half, 0.5 * args.width + half, 0.5 * args.height + half])
    net = NetworkWithPointHead(enable_point_head=True, enable_uncertainty=False).cuda().eval()  # (the time does not depend on the weights)
    predictors = [E.Predictor(net, focus_roi_expansion_factor=f) for f in args.factors]
    eager, graphed = E.ClosedLoopTracker(net, factors=args.factors), E.ClosedLoopTracker(net, factors=args.factors, graphed=True)
    legs = {"loop": lambda: loop_pass(predictors, frames[:, None], first, args.factors), "eager": lambda: eager.track(frames, first[None])}
    if not args.skip_graphed:
        legs["graphed"] = lambda: graphed.track(frames, first[None])
    times, last = {k: [] for k in legs}, {}
    for k, fn in legs.items():  # warm-up: code objects, allocator, every shape
        fn()
    for _ in range(args.reps):
        for k, fn in legs.items():  # alternating
            t, last[k] = timed(fn)
            times[k].append(t)
    result = {"frames": args.frames, "frame_hw": [args.height, args.width], "factors": args.factors, "reps": args.reps, "legs": {}}
    for k, v in times.items():
        result["legs"][k] = {"fps_median": args.frames / float(np.median(v)), "fps_min": args.frames / max(v), "fps_max": args.frames / min(v),
                             "ms_per_frame_median": 1e3 * float(np.median(v)) / args.frames, "ms_per_frame_min": 1e3 * min(v) / args.frames,
                             "ms_per_frame_max": 1e3 * max(v) / args.frames, "seconds": v}
        r = result["legs"][k]
        print(f"{k:8s}: {r['fps_median']:9.1f} frames/s ({r['fps_min']:.1f} - {r['fps_max']:.1f}), {r['ms_per_frame_median']:.4f} ms/frame "
              f"({r['ms_per_frame_min']:.4f} - {r['ms_per_frame_max']:.4f})", flush=True)
    result["lost_frames_per_lane"] = last["eager"]["lost"].sum(0).tolist()
    result["loop_boxes_max_abs_difference_to_eager"] = float((last["loop"] - last["eager"]["roi_in"].cpu()).abs().max())
    print(f"lost frames per lane (eager): {result['lost_frames_per_lane']}; boxes of the loop against the tracker's: max |difference| "
          f"{result['loop_boxes_max_abs_difference_to_eager']:.3e} px (two float32 back-transformations in a feedback loop)")
    if "graphed" in last:
        same = all(torch.equal(last["eager"][k], last["graphed"][k]) for k in last["eager"].keys())
        result["graphed_equals_eager_bitwise"] = bool(same)
        print(f"graphed trajectory == eager trajectory, bitwise, every field, T = {args.frames}: {same}")
    line = json.dumps(result)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
