#!/usr/bin/env python
"""Label a dataset shard with an ensemble of trained networks (reference: scripts/add_pose_pseudolabels.py): every checkpoint predicts
every frame, the predictions are averaged per frame - rotations with the reference's quat_average, coord / pt3d_68 / shapeparam with the
arithmetic mean - and the averages become the shard's labels (quats, coords, pt3d_68, shapeparams), ready for `--ds ...` mixes.

    python scripts/add_pose_pseudolabels.py data/wflw.npz -c run1/best.ckpt run2/best.ckpt run3/best.ckpt --output data/wflw_lp.npz
           [-b 512] [--dryrun] [-f] [--resample bilinear|area] [--max-rot-spread DEG] [--device cuda]

The frames are decoded once and stay resident in HBM (datasets/shards.load_resident_frames); all checkpoints are loaded once; every batch
is cropped ONCE and reduced on the device (trackertraincode.eval.EnsemblePredictor, csrc/ensemble.hip) - one pass over the data, one
synchronisation at the end.  Differences from the reference's command line: an .npz is not edited in place, so `--output PATH` names the
shard to write (default: the input, which then needs -f / --overwrite); `--resample` selects the crop's filter; `--max-rot-spread DEG`
drops frames whose members disagree by more than DEG degrees (mean geodesic angle to the average); `--hdf-group-name` has no meaning for
shards.  `--dryrun` labels the first 10 frames and writes a shard of those 10, which is why it refuses to write over its input.
The networks' unit quaternions `pose` are averaged after the back-transformation to image coordinates, not `unnormalized_quat` as in the
reference (see eval.EnsemblePredictor)."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from trackertraincode import eval as E  # noqa: E402
from trackertraincode.datasets.shards import load_resident_frames, write_pseudolabels  # noqa: E402
from trackertraincode.neuralnets import models  # noqa: E402
from trackertraincode.pipelines import Tag  # noqa: E402

LABEL_KEYS = ("pose", "coord", "pt3d_68", "shapeparam", "rot_spread", "mean_quat_norm", "coord_spread")
DRYRUN_FRAMES = 10


@torch.no_grad()
def label_frames(predictor: E.EnsemblePredictor, frames, count: int, batchsize: int) -> dict:
    """The ensemble's labels of the first `count` frames: device tensors, nothing synchronises here."""
    images, rois = frames.fields["image"], frames.fields["roi"].to(torch.float32)
    parts: dict = {}
    for lo in range(0, count, batchsize):
        hi = min(lo + batchsize, count)
        out = predictor.predict_batch(images[lo:hi], rois[lo:hi])
        for k in LABEL_KEYS:
            if k in out:
                parts.setdefault(k, []).append(out[k])
    return {k: torch.cat(v) for k, v in parts.items()}


def run(args) -> dict:
    output = args.output or args.filename
    same = os.path.abspath(output) == os.path.abspath(args.filename)
    if os.path.exists(output) and not args.overwrite:
        raise SystemExit(f"{output} exists: pass --overwrite / -f to replace it" + (" (the default output is the input file)" if same else ""))
    if args.dryrun and same:
        raise SystemExit(f"--dryrun writes a shard of the first {DRYRUN_FRAMES} frames: give it an --output other than the input")
    missing = [f for f in args.checkpoints if not os.path.isfile(f)]
    if missing or not args.checkpoints:
        raise SystemExit(f"checkpoints not found: {missing}" if missing else "no checkpoints given (-c)")
    print("Inferring from networks:", args.checkpoints)
    nets = [models.load_model(f).to(args.device).eval() for f in args.checkpoints]
    predictor = E.EnsemblePredictor(nets, focus_roi_expansion_factor=1.2, device=args.device, resample=args.resample)
    frames = load_resident_frames(args.filename, Tag.ONLY_POSE, device=args.device)
    total = len(frames)
    count = min(DRYRUN_FRAMES, total) if args.dryrun else total
    labels = {k: v.cpu().numpy() for k, v in label_frames(predictor, frames, count, args.batchsize).items()}  # the one synchronisation
    keep = np.arange(total) < count
    wild = int((labels["mean_quat_norm"] <= 0.5).sum())
    if args.max_rot_spread is not None:
        keep[:count] &= np.degrees(labels["rot_spread"].astype(np.float64)) <= args.max_rot_spread
    if count < total:  # the writer takes labels over all frames of the source; the rest is dropped by `keep`
        labels = {k: np.concatenate([v, np.zeros((total - count,) + v.shape[1:], v.dtype)]) for k, v in labels.items()}
    write_pseudolabels(args.filename, output, labels, keep=keep, overwrite=args.overwrite)
    dropped = count - int(keep.sum())
    print(f"{count} frames labelled by {len(nets)} networks; {wild} with a mean quaternion norm <= 0.5 (rotation predictions differ wildly); "
          f"{dropped} dropped (--max-rot-spread); {int(keep.sum())} written to {output}")
    return {"labelled": count, "wild": wild, "dropped": dropped, "written": int(keep.sum()), "output": output}


def make_parser():
    ap = argparse.ArgumentParser(description="Label a dataset shard with an ensemble of networks")
    ap.add_argument("filename", type=str, help="the dataset shard (.npz) to label")
    ap.add_argument("-c", "--checkpoints", help="model checkpoints", nargs="*", type=str, default=[])
    ap.add_argument("-b", "--batchsize", help="The batch size", type=int, default=512)
    ap.add_argument("--dryrun", default=False, action="store_true", help=f"label the first {DRYRUN_FRAMES} frames only")
    ap.add_argument("--overwrite", "-f", default=False, action="store_true", help="replace existing labels / an existing output file")
    ap.add_argument("--output", type=str, default=None, help="the shard to write (default: the input, which needs --overwrite)")
    ap.add_argument("--resample", default="bilinear", choices=["bilinear", "area"], help="the crop's resampler (label with the filter the networks were trained with)")
    ap.add_argument("--max-rot-spread", type=float, default=None, metavar="DEG",
                    help="drop frames whose mean geodesic angle between the members and their average exceeds DEG degrees")
    ap.add_argument("--device", default="cuda", type=str)
    return ap


def main(argv=None):
    return run(make_parser().parse_args(argv))


if __name__ == "__main__":
    main()
