#!/usr/bin/env python3
"""Frames per second of the labelling pass (scripts/add_pose_pseudolabels.py's loop) at batch 512 with E = 1, 3, 5 full-size MobileNet
networks and the frames resident in HBM, against what the same job takes without eval.EnsemblePredictor: a loop of
`Predictor.predict_batch` per network, every prediction pulled to the host, numpy `quat_average` / `np.average` there.

    python tools/pseudolabel_bench.py [--frames 4096] [--batchsize 512] [--members 1 3 5] [--reps 5] [--size 256] [--json out.json]
    python tools/pseudolabel_bench.py --profile-pass 3        # one ensemble pass with E = 3 and nothing else (for rocprofv3 --kernel-trace --stats)

Both paths label the same frames with the same weights; they alternate inside one process, `reps` times each after a warm-up pass, and
a pass is timed with the host clock from its first launch to the end of its last synchronisation.  Medians and the min-max spread are
printed; the labels of the two paths are compared (they differ by float32 rounding: the loop back-transforms in torch, averages in
float64 on the host).  Prints one JSON line at the end."""
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
from trackertraincode.neuralnets.torchquaternion import quat_average  # noqa: E402

KEYS = ("pose", "coord", "pt3d_68", "shapeparam")


def make_frames(n, size, seed=0):
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (n, 1, size, size), dtype=torch.uint8, generator=g).cuda()
    c = 0.5 * size + (torch.rand(n, 2, generator=g) - 0.5) * 0.2 * size
    half = (0.25 + 0.1 * torch.rand(n, 1, generator=g)) * size
    return images, torch.cat([c - half, c + half], -1).cuda()


def make_nets(count):
    nets = []
    for seed in range(count):
        net = NetworkWithPointHead(enable_point_head=True, enable_uncertainty=False)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():  # members that disagree a little, like checkpoints of separate runs
            for p in net.parameters():
                p.add_(torch.randn(p.shape, generator=g) * 0.02 * p.abs().mean())
        nets.append(net.cuda().eval())
    return nets


def ensemble_pass(pred, images, rois, B):
    parts = {k: [] for k in KEYS}
    for lo in range(0, len(images), B):
        out = pred.predict_batch(images[lo:lo + B], rois[lo:lo + B])
        for k in KEYS:
            parts[k].append(out[k])
    return {k: torch.cat(v).cpu().numpy() for k, v in parts.items()}  # the one synchronisation


def loop_pass(preds, images, rois, B):
    """The parent commit's way: checkpoint by checkpoint over the whole set, results to the host, the average in numpy."""
    per_net = {k: [] for k in KEYS}
    for p in preds:
        outs = {k: [] for k in KEYS}
        for lo in range(0, len(images), B):
            out = p.predict_batch(images[lo:lo + B], rois[lo:lo + B])
            for k in KEYS:
                outs[k].append(out[k].cpu().numpy())
        for k in KEYS:
            per_net[k].append(np.concatenate(outs[k]))
    res = {k: np.average(np.stack(per_net[k]), axis=0) for k in KEYS[1:]}
    res["pose"] = quat_average(np.stack(per_net["pose"]))
    return res


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--batchsize", type=int, default=512)
    ap.add_argument("--members", type=int, nargs="*", default=[1, 3, 5])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=256, help="side of the synthetic frames in pixels")
    ap.add_argument("--json", type=str, default=None)
    ap.add_argument("--profile-pass", type=int, default=0, metavar="E", help="run one warm-up and one ensemble pass with E members, nothing else")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the MI355X")
    images, rois = make_frames(args.frames, args.size)
    nets = make_nets(max(args.members + [args.profile_pass]))
    if args.profile_pass:
        pred = E.EnsemblePredictor(nets[:args.profile_pass])
        for _ in range(2):
            ensemble_pass(pred, images, rois, args.batchsize)
        return
    result = {"frames": args.frames, "batchsize": args.batchsize, "frame_size": args.size, "reps": args.reps, "members": {}}
    for n in args.members:
        ens = E.EnsemblePredictor(nets[:n])
        singles = [E.Predictor(net, focus_roi_expansion_factor=1.2) for net in nets[:n]]
        runs = {"ensemble": lambda: ensemble_pass(ens, images, rois, args.batchsize), "loop": lambda: loop_pass(singles, images, rois, args.batchsize)}
        times, last = {k: [] for k in runs}, {}
        for k, fn in runs.items():  # warm-up: code objects, allocator, every shape of the pass
            fn()
        for _ in range(args.reps):
            for k, fn in runs.items():  # alternating
                t, last[k] = timed(fn)
                times[k].append(t)
        sign = np.sign((last["ensemble"]["pose"] * last["loop"]["pose"]).sum(-1, keepdims=True))
        diff = {k: float(np.abs(last["ensemble"][k] - last["loop"][k] * (sign if k == "pose" else 1.0)).max()) for k in KEYS}
        row = {k: {"fps_median": args.frames / float(np.median(v)), "fps_min": args.frames / max(v), "fps_max": args.frames / min(v),
                   "seconds_median": float(np.median(v))} for k, v in times.items()}
        row["speedup_median"] = float(np.median(times["loop"]) / np.median(times["ensemble"]))
        row["max_abs_difference"] = diff
        result["members"][str(n)] = row
        print(f"E={n}: ensemble {row['ensemble']['fps_median']:.0f} frames/s ({row['ensemble']['fps_min']:.0f}-{row['ensemble']['fps_max']:.0f}), "
              f"loop {row['loop']['fps_median']:.0f} ({row['loop']['fps_min']:.0f}-{row['loop']['fps_max']:.0f}), x{row['speedup_median']:.2f}; "
              f"max |difference| {diff}", flush=True)
    line = json.dumps(result)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
