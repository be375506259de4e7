#!/usr/bin/env python
"""Fit the deformable face model to the 2-D landmarks of a pseudo-labelled shard (reference: scripts/DsWflwFitFaceModel.ipynb and
scripts/DsLapaMegafaceFitFaceModel.ipynb - the readme's step after "Generate pseudo labels"): every frame's pose, position, size and 50
shape parameters are fitted to its 68 landmarks, and the results become the shard's labels quats, coords, pt3d_68 and shapeparams - what
Points3dLoss, ShapeParameterLoss and ShapePlausibilityLoss train on.

    python scripts/fit_face_model.py data_lp.npz --output data_fit.npz (--basis FILE.npz | --basis-from-checkpoint CKPT)
           [--fit-3d-projections] [-b 4096] [--max-objective X] [--drop-unconverged] [--dryrun] [-f] [--device cuda]

Start values are the shard's `quats` / `coords` (e.g. from add_pose_pseudolabels.py), targets its `pt2d_68`, or the xy of `pt3d_68` with
--fit-3d-projections; `rois` gives the view.  The basis is a file with arrays `keypts` [68,3] and `keyeigvecs` [50,68,3], or the
`landmarks.deformablekeypoints.*` buffers of a checkpoint.  The labels are read without decoding one image; every batch is one launch of
the fit on the device (facemodel/fitting.py, csrc/facefit.hip) and one synchronisation.  --max-objective X drops frames whose final
objective exceeds X, --drop-unconverged those whose status is not 0; --dryrun fits the first 10 frames and writes a shard of those 10.
The reference edits its HDF5 file in place (group "2dfit_v3"); a shard is rewritten (--output, default the input, which needs -f)."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from trackertraincode.datasets.shards import read_labels, write_face_fit  # noqa: E402
from trackertraincode.facemodel.fitting import STATUS_NAMES, FaceModelFitter  # noqa: E402

DRYRUN_FRAMES = 10
OUT_KEYS = ("pose", "coord", "pt3d_68", "shapeparam", "objective", "status", "iterations")


def make_fitter(args) -> FaceModelFitter:
    kw = dict(fit_3d_projections=args.fit_3d_projections, device=args.device)
    if args.basis_from_checkpoint:
        return FaceModelFitter.from_checkpoint(args.basis_from_checkpoint, **kw)
    with np.load(args.basis) as d:
        missing = [k for k in ("keypts", "keyeigvecs") if k not in d.files]
        if missing:
            raise SystemExit(f"{args.basis}: no {missing} (a basis file holds keypts [68,3] and keyeigvecs [50,68,3])")
        return FaceModelFitter(d["keypts"], d["keyeigvecs"], **kw)


def run(args) -> dict:
    output = args.output or args.filename
    same = os.path.abspath(output) == os.path.abspath(args.filename)
    if os.path.exists(output) and not args.overwrite:
        raise SystemExit(f"{output} exists: pass --overwrite / -f to replace it" + (" (the default output is the input file)" if same else ""))
    if args.dryrun and same:
        raise SystemExit(f"--dryrun writes a shard of the first {DRYRUN_FRAMES} frames: give it an --output other than the input")
    if bool(args.basis) == bool(args.basis_from_checkpoint):
        raise SystemExit("give the face-model basis with exactly one of --basis FILE.npz and --basis-from-checkpoint CKPT")
    labels = read_labels(args.filename)
    target_key = "pt3d_68" if args.fit_3d_projections else "pt2d_68"
    names = {"roi": "rois", "pose": "quats", "coord": "coords", "pt2d_68": "pt2d_68", "pt3d_68": "pt3d_68"}
    missing = [names[k] for k in ("roi", "pose", "coord", target_key) if k not in labels]
    if missing:
        raise SystemExit(f"{args.filename} lacks {missing}: the fit starts from quats / coords (scripts/add_pose_pseudolabels.py writes them), "
                         f"crops by rois and fits {names[target_key]}")
    fitter = make_fitter(args)
    total = len(labels["roi"])
    count = min(DRYRUN_FRAMES, total) if args.dryrun else total
    parts: dict = {k: [] for k in OUT_KEYS}
    for lo in range(0, count, args.batchsize):
        hi = min(lo + args.batchsize, count)
        out = fitter.fit(*(torch.from_numpy(np.ascontiguousarray(labels[k][lo:hi])) for k in ("roi", "pose", "coord", target_key)))
        for k in OUT_KEYS:
            parts[k].append(out[k].cpu().numpy())  # the batch's one synchronisation
    fitted = {k: np.concatenate(v) for k, v in parts.items()}
    status, objective = fitted["status"], fitted["objective"]
    keep = np.arange(total) < count
    if args.drop_unconverged:
        keep[:count] &= status == 0
    if args.max_objective is not None:
        keep[:count] &= objective <= args.max_objective
    counts = {int(s): int((status == s).sum()) for s in sorted(STATUS_NAMES)}
    quartiles = np.quantile(objective[np.isfinite(objective)], [0.0, 0.25, 0.5, 0.75, 1.0]).tolist() if np.isfinite(objective).any() else []
    print(f"{count} frames fitted; status: " + ", ".join(f"{counts[s]} {STATUS_NAMES[s]}" for s in counts))
    print("objective min / quartiles / max: " + " ".join(f"{q:.3e}" for q in quartiles))
    if count < total:  # the writer takes labels over all frames of the source; the rest is dropped by `keep`
        fitted = {k: np.concatenate([v, np.zeros((total - count,) + v.shape[1:], v.dtype)]) for k, v in fitted.items()}
    # (the fit replaces quats / coords and, with --fit-3d-projections, pt3d_68: those are present by construction, so only an existing
    # OUTPUT file needs -f, which was checked above)
    write_face_fit(args.filename, output, fitted, keep=keep, overwrite=True)
    dropped = count - int(keep.sum())
    print(f"{dropped} dropped (--max-objective / --drop-unconverged); {int(keep.sum())} written to {output}")
    return {"fitted": count, "status": counts, "quartiles": quartiles, "dropped": dropped, "written": int(keep.sum()), "output": output}


def make_parser():
    ap = argparse.ArgumentParser(description="Fit the deformable face model to the landmarks of a shard")
    ap.add_argument("filename", type=str, help="the dataset shard (.npz) with rois, quats, coords and pt2d_68")
    ap.add_argument("--output", type=str, default=None, help="the shard to write (default: the input, which needs --overwrite)")
    ap.add_argument("--basis", type=str, default=None, metavar="FILE.npz", help="face-model basis: arrays keypts [68,3] and keyeigvecs [50,68,3]")
    ap.add_argument("--basis-from-checkpoint", type=str, default=None, metavar="CKPT", help="take the basis from a checkpoint's landmark head")
    ap.add_argument("--fit-3d-projections", default=False, action="store_true", help="fit the xy of pt3d_68 with unit weights instead of pt2d_68")
    ap.add_argument("-b", "--batchsize", type=int, default=4096, help="samples per launch")
    ap.add_argument("--max-objective", type=float, default=None, metavar="X", help="drop frames whose final objective exceeds X")
    ap.add_argument("--drop-unconverged", default=False, action="store_true", help="drop frames whose fit did not converge (status != 0)")
    ap.add_argument("--dryrun", default=False, action="store_true", help=f"fit the first {DRYRUN_FRAMES} frames only")
    ap.add_argument("--overwrite", "-f", default=False, action="store_true", help="replace an existing output file")
    ap.add_argument("--device", default="cuda", type=str)
    return ap


def main(argv=None):
    args = make_parser().parse_args(argv)
    if args.batchsize < 1:
        raise SystemExit("--batchsize must be positive")
    return run(args)


if __name__ == "__main__":
    main()
