#!/usr/bin/env python
"""Judge a tracker on a video before shipping it (reference: scripts/evaluate_stability.py).

    python scripts/evaluate_stability.py MODE DATA CHECKPOINT... [--factors 1.0 1.2] [--blinks a:b,c:d,...] [--output OUT.npz]
           [--graphed] [--seed N] [--device cuda] [--localizer CKPT [--reacquire-after K] [--face-threshold P]]

DATA is a pose shard (datasets/shards.decode_pose_shard) whose frames are one video in order; a CHECKPOINT argument may be a glob (the
reference's `_find_models`): its matches form one group whose runs are averaged.  Modes:

  closed-loop   every checkpoint tracks the video with `eval.ClosedLoopTracker` - each frame cropped around the box predicted on the
                previous one, all crop factors as lanes of one track, started from the shard's first box, the whole video enqueued before
                the one synchronisation (reference :248-264, which reads the box back per frame).  Prints the lost frames per lane.
                With --localizer CKPT (a LocalizerNet checkpoint: a plain state_dict file, as the reference's load_facelocalizer reads
                it, or {state_dict, class_name, config}) the face localizer runs on every frame and a lane that has been lost for
                --reacquire-after frames (3) restarts from its box if the face probability exceeds --face-threshold (0.5); prints the
                re-acquisitions per lane and writes g<g>/reacquired [C,T,L], g<g>/hasface [C,T], g<g>/loc_roi [C,T,4].
  open-loop     `Predictor.evaluate` with the stored boxes, per factor (:267-272).
  noise-resist  crops once with the predictor's own crop, adds N(0, (level / 256)^2) noise for the levels 0, 2, 8, 16, 32, 48, 64 from a
                seeded device generator (--seed) and prints the mean geodesic error in degrees per level and checkpoint, with average and
                standard deviation over the checkpoints (:434-471; the shard needs pose labels).

closed-loop / open-loop write to OUT.npz, per group g (the g-th CHECKPOINT argument): g<g>/hpb [T,L,3] (heading, pitch, bank in radians:
the reference's utils.as_hpb), g<g>/xy [T,L,2], g<g>/sz [T,L] - np.average over the group's checkpoints - g<g>/hpb_std, xy_std, sz_std
(np.std over them: the reference's PosesWithStd.from_poses) and g<g>/lost [C,T,L]; lanes are the crop factors in the order given.  With
--blinks they print the reference's blink-stability report (:229-245): per quantity the RMS over the blink boundaries x of
v[x - 5] - v[x + 5], averaged over the runs (checkpoints x factors) of a group, hpb in degrees; a boundary within 5 frames of either end of
the video is an error.  The `lost` rule of the tracker, the missing area resampling and the missing uncertainty fields: eval.ClosedLoopTracker.
Out of scope, refused with a reason: pitch-yaw, variation-resist, uncertainty-correlation (figures, or sets this package has no shard for)
and all plotting."""
from __future__ import annotations

import argparse
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from trackertraincode import eval as E  # noqa: E402
from trackertraincode import utils  # noqa: E402
from trackertraincode.datasets.batch import Batch, Metadata  # noqa: E402
from trackertraincode.datasets.shards import decode_pose_shard  # noqa: E402
from trackertraincode.neuralnets import models  # noqa: E402

NOISE_LEVELS = (0.0, 2.0, 8.0, 16.0, 32.0, 48.0, 64.0)  # reference :436
REFUSED = {"pitch-yaw": "a scatter plot over the reference's 'myself_yaw' and Biwi sections, sets this package has no shard for",
           "variation-resist": "a plot over the 'replicantface-stability' set, which this package has no shard for",
           "uncertainty-correlation": "a scatter plot of the uncertainty outputs, which the closed-loop path does not record; plotting is not built"}


def find_models(path: str) -> list:
    return [path] if os.path.isfile(path) else sorted(glob.glob(path))


def as_hpb(quats: np.ndarray) -> np.ndarray:
    """Heading, pitch, bank of quaternions [..., 4] (reference utils.as_hpb: Rotation.as_euler("YXZ"))."""
    from scipy.spatial.transform import Rotation

    q = np.asarray(quats, dtype=np.float64)
    return Rotation.from_quat(q.reshape(-1, 4)).as_euler("YXZ").reshape(q.shape[:-1] + (3,))


def parse_blinks(text: str) -> list:
    try:
        return [tuple(int(v) for v in part.split(":")) for part in text.split(",") if part]
    except ValueError:
        raise SystemExit(f"--blinks: expected a:b,c:d,..., got {text!r}")


def poses_of(pose, coord) -> dict:
    coord = np.asarray(coord, dtype=np.float64)
    return {"hpb": as_hpb(pose), "xy": coord[..., :2], "sz": coord[..., 2]}


class _Collect:
    """The pose and coord predictions of every batch (the reference's PredExtractor collection)."""

    def __init__(self):
        self.pose, self.coord = [], []

    def update(self, preds, targets):
        self.pose.append(preds["pose"])
        self.coord.append(preds["coord"])

    def compute(self):
        return torch.cat(self.pose).cpu().numpy(), torch.cat(self.coord).cpu().numpy()


def track_closed_loop(net, shard, args):
    frames = torch.from_numpy(shard["image"][:, 0])
    localizer = models.load_localizer(args.localizer) if args.localizer else None
    out = E.ClosedLoopTracker(net, factors=args.factors, device=args.device, graphed=args.graphed, localizer=localizer,
                              reacquire_after=args.reacquire_after, face_threshold=args.face_threshold).track(frames, shard["roi"][:1])
    extra = {k: out[k].cpu().numpy() for k in ("reacquired", "hasface", "loc_roi") if k in out}
    for k in ("hasface", "loc_roi"):  # one video: [T, 1(, 4)] -> [T(, 4)]
        if k in extra:
            extra[k] = extra[k][:, 0]
    return poses_of(out["pose"].cpu().numpy(), out["coord"].cpu().numpy()), out["lost"].cpu().numpy(), extra


def track_open_loop(net, shard, args):
    samples = [{"image": torch.from_numpy(im[0]), "roi": torch.from_numpy(r)} for im, r in zip(shard["image"], shard["roi"])]
    runs = [E.Predictor(net, focus_roi_expansion_factor=f, device=args.device).evaluate(_Collect(), samples) for f in args.factors]
    poses = poses_of(np.stack([p for p, _ in runs], 1), np.stack([c for _, c in runs], 1))
    return poses, np.zeros(poses["sz"].shape, dtype=bool), {}


def run_tracking(args, shard, tracker) -> dict:
    if args.blinks:  # refused before anything runs
        try:
            E.blink_stability(np.zeros(len(shard["image"])), args.blinks)
        except ValueError as e:
            raise SystemExit(f"--blinks: {e}")
    saved = {"factors": np.asarray(args.factors, np.float64)}
    for g, path in enumerate(args.checkpoints):
        files = find_models(path)
        if not files:
            raise SystemExit(f"no checkpoint matches {path!r}")
        print(f"Evaluating {path}. Found {len(files)} checkpoints.")
        runs = [tracker(models.load_model(f).to(args.device).eval(), shard, args) for f in files]
        for k in ("hpb", "xy", "sz"):
            stack = [poses[k] for poses, _, _ in runs]
            saved[f"g{g}/{k}"], saved[f"g{g}/{k}_std"] = np.average(stack, axis=0), np.std(stack, axis=0)
        saved[f"g{g}/lost"] = np.stack([lost for _, lost, _ in runs])
        for k in runs[0][2]:
            saved[f"g{g}/{k}"] = np.stack([extra[k] for _, _, extra in runs])
        for f, (_, lost, extra) in zip(files, runs):
            print(f"  {f}: lost frames per lane (factors {list(args.factors)}): {lost.sum(0).tolist()} of {lost.shape[0]}")
            if "reacquired" in extra:
                print(f"  {f}: re-acquisitions per lane: {extra['reacquired'].sum(0).tolist()}")
        if args.blinks:
            print(f"Checkpoint: {path}")
            for k in ("hpb", "sz", "xy"):  # the reference's order; a run = one checkpoint with one factor
                per_run = [E.blink_stability(poses[k][:, lane], args.blinks) for poses, _, _ in runs for lane in range(len(args.factors))]
                val = np.average(per_run, axis=0) * (utils.rad2deg if k == "hpb" else 1.0)
                print(f"\t {k:4s}: " + ", ".join(f"{x:0.2f}" for x in val))
    if args.output:
        np.savez(args.output, **saved)
        print(f"written to {args.output}")
    return saved


@torch.no_grad()
def run_noise_resist(args, shard) -> dict:
    if "pose" not in shard:
        raise SystemExit("noise-resist measures the rotation error: the shard has no pose labels")
    files = [f for path in args.checkpoints for f in (find_models(path) or [None])]
    if None in files:
        raise SystemExit(f"a CHECKPOINT argument matches no file: {args.checkpoints}")
    dev = torch.device(args.device)
    images, n = torch.from_numpy(shard["image"]).to(dev), len(shard["image"])
    table = []
    for f in files:
        predictor = E.Predictor(models.load_model(f), device=dev)
        # the predictor's own crop, once, with the rotation labels carried into the crop's frame
        crop = predictor._crop(Batch(Metadata(tuple(images.shape[-2:][::-1]), n), image=images, roi=torch.from_numpy(shard["roi"]).to(dev),
                                     pose=torch.from_numpy(shard["pose"]).to(dev)))
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed)
        row = []
        for level in NOISE_LEVELS:
            noisy = crop["image"] + (level / 256.0) * torch.randn(crop["image"].shape, generator=gen, device=dev, dtype=torch.float32)
            err = predictor.evaluate_cropped_normalized(E.GeodesicError(), [{"image": noisy, "pose": crop["pose"]}])
            row.append(float(err.mean().item()) * utils.rad2deg)
        table.append(row)
    table = np.asarray(table, dtype=np.float64)
    print("noise level : " + " ".join(f"{lv:8.1f}" for lv in NOISE_LEVELS))
    for f, row in zip(files, table):
        print(f"{os.path.basename(f)} : " + " ".join(f"{v:8.4f}" for v in row))
    print("average     : " + " ".join(f"{v:8.4f}" for v in np.average(table, axis=0)))
    print("std         : " + " ".join(f"{v:8.4f}" for v in np.std(table, axis=0)))
    saved = {"noise_levels": np.asarray(NOISE_LEVELS), "geodesic_deg": table}
    if args.output:
        np.savez(args.output, **saved)
    return saved


def make_parser():
    ap = argparse.ArgumentParser(description="Closed-loop / open-loop stability and noise resistance of pose networks on a video shard")
    ap.add_argument("mode", type=str, help="closed-loop | open-loop | noise-resist")
    ap.add_argument("data", type=str, help="the pose shard (.npz), frames in video order")
    ap.add_argument("checkpoints", nargs="+", type=str, help="model checkpoints; a glob forms one averaged group")
    ap.add_argument("--factors", nargs="+", type=float, default=[1.0, 1.2], help="crop enlargement factors (the reference's 1.0 and 1.2)")
    ap.add_argument("--blinks", type=parse_blinks, default=None, metavar="a:b,c:d", help="frame ranges with closed eyes: prints the blink-stability report")
    ap.add_argument("--output", type=str, default=None, help="the .npz to write")
    ap.add_argument("--graphed", action="store_true", default=False, help="closed-loop: replay one captured graph per frame")
    ap.add_argument("--localizer", type=str, default=None, metavar="CKPT", help="closed-loop: a LocalizerNet checkpoint; lost lanes restart from its box")
    ap.add_argument("--reacquire-after", type=int, default=3, help="closed-loop with --localizer: lost frames before a lane restarts")
    ap.add_argument("--face-threshold", type=float, default=0.5, help="closed-loop with --localizer: face probability a restart needs")
    ap.add_argument("--seed", type=int, default=0, help="noise-resist: seed of the device generator")
    ap.add_argument("--device", default="cuda", type=str)
    return ap


def main(argv=None):
    args = make_parser().parse_args(argv)
    if args.mode in REFUSED:
        raise SystemExit(f"mode {args.mode!r} is not built: {REFUSED[args.mode]}")
    if args.mode not in ("closed-loop", "open-loop", "noise-resist"):
        raise SystemExit(f"unknown mode {args.mode!r}: closed-loop, open-loop or noise-resist")
    if args.localizer and args.mode != "closed-loop":
        raise SystemExit(f"--localizer: mode {args.mode!r} crops every frame around a stored box and has no track to lose; the localizer "
                         "re-acquires lost lanes of closed-loop only")
    if args.localizer and not os.path.isfile(args.localizer):
        raise SystemExit(f"--localizer: no such file {args.localizer!r}")
    shard = decode_pose_shard(args.data)
    if args.mode == "noise-resist":
        return run_noise_resist(args, shard)
    return run_tracking(args, shard, track_closed_loop if args.mode == "closed-loop" else track_open_loop)


if __name__ == "__main__":
    main()
