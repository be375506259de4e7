#!/usr/bin/env python3
"""Fits per second of the face-model fit on the device (ttk_facefit, csrc/facefit.hip) at a labelling-sized batch, next to the float64
restatement of the same objective minimised with scipy's BFGS on the host.

    python tools/facefit_bench.py [--batch 65536] [--unique 4096] [--passes 3] [--cpu-samples 256] [--json out.json]

Device leg: `unique` planted cases (tests/facefit_ref.planted_cases: synthetic basis, committed mixture, yaw up to +-70 degrees, start 0.1
rad off, landmark noise 0.005, 2-D weights) tiled to `batch` rows - rows are independent, so tiling changes nothing per row and keeps
the host-side generation short.  One warm-up launch, then `passes` launches timed with HIP events on the stream; median and range.
Host leg: facefit_ref.fit_scipy (two scipy BFGS stages, analytic gradient, float64 numpy) on the first `cpu-samples` cases, wall clock,
one thread of numpy.  The reference's own path (torchmin through autograd) cannot be timed: torchmin is not installed.
Also printed: status counts and iteration histograms of the device run, the evaluation counts of the restated optimiser on the host
samples (its iteration counts are the kernel's), and FIT_OBJ_MARGIN of tests/facefit_cases.py.  Prints one JSON line at the end."""
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
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)
import facefit_ref as R  # noqa: E402
from trackertraincode.facemodel.fitting import FaceModelFitter  # noqa: E402


def histogram(v, edges):
    h, _ = np.histogram(v, bins=edges)
    return {f"{edges[i]}-{edges[i + 1] - 1}": int(h[i]) for i in range(len(h)) if h[i]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--unique", type=int, default=4096)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--cpu-samples", type=int, default=256)
    ap.add_argument("--margin", action="store_true", help="also compute FIT_OBJ_MARGIN over the test cases (a few seconds of host time)")
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args(argv)

    m = R.synthetic_model()
    t0 = time.perf_counter()
    x0, y, w = R.planted_cases(m, args.unique, 2028)
    print(f"{args.unique} planted cases generated in {time.perf_counter() - t0:.1f} s; tiled to B = {args.batch}")
    reps = -(-args.batch // args.unique)
    tile = lambda a: torch.from_numpy(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:args.batch]).cuda()
    X, Y, W = tile(x0), tile(y), tile(w)
    fitter = FaceModelFitter(m.kp, m.eig)
    out = fitter.fit_normalized(X[:, :4], X[:, 4:7], Y, weights=W)  # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fitter.fit_normalized(X[:, :4], X[:, 4:7], Y, weights=W)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.array(ms)
    status, iters = out["status"].cpu().numpy(), out["iterations"].cpu().numpy()
    f = out["objective"].cpu().numpy()
    dev = {"batch": args.batch, "ms": [round(float(v), 3) for v in ms], "ms_median": round(float(np.median(ms)), 3),
           "fits_per_s_median": round(args.batch / (np.median(ms) * 1e-3)), "fits_per_s_range": [round(args.batch / (ms.max() * 1e-3)), round(args.batch / (ms.min() * 1e-3))],
           "us_per_fit": round(float(np.median(ms)) * 1e3 / args.batch, 3), "status": {int(s): int((status == s).sum()) for s in range(4)},
           "iterations_stage1": histogram(iters[:, 0], [0, 5, 10, 15, 20, 30, 51]), "iterations_stage2": histogram(iters[:, 1], [0, 10, 20, 30, 40, 60, 80, 101]),
           "objective_quartiles": [float(q) for q in np.quantile(f, [0, 0.25, 0.5, 0.75, 1])]}
    print(f"device: {dev['ms']} ms per launch of B = {args.batch}: median {dev['fits_per_s_median']} fits/s "
          f"(range {dev['fits_per_s_range']}), {dev['us_per_fit']} us per fit; status {dev['status']}")
    print(f"  iterations stage 1 {dev['iterations_stage1']}, stage 2 {dev['iterations_stage2']}")

    n = min(args.cpu_samples, args.unique)
    t0 = time.perf_counter()
    sc = [R.fit_scipy(m, x0[i], y[i], w[i]) for i in range(n)]
    t_scipy = time.perf_counter() - t0
    t0 = time.perf_counter()
    ours = [R.fit(m, x0[i], y[i], w[i]) for i in range(n)]
    t_ours = time.perf_counter() - t0
    ev = np.array([o["evaluations"] for o in ours])
    same = int(sum(tuple(iters[i]) == tuple(o["iterations"]) for i, o in enumerate(ours)))
    excess = max(float(f[i]) - s["f"] for i, s in enumerate(sc))
    cpu = {"samples": n, "scipy_ms_per_fit": round(t_scipy / n * 1e3, 2), "scipy_fits_per_s": round(n / t_scipy, 1),
           "restated_optimiser_ms_per_fit": round(t_ours / n * 1e3, 2), "evaluations_stage1": histogram(ev[:, 0], [0, 5, 10, 15, 20, 30, 60]),
           "evaluations_stage2": histogram(ev[:, 1], [0, 10, 20, 30, 40, 60, 80, 120]), "rows_with_the_kernels_iteration_counts": same,
           "largest_device_objective_above_scipy": excess}
    print(f"host: scipy BFGS restatement {cpu['scipy_ms_per_fit']} ms per fit ({cpu['scipy_fits_per_s']} fits/s, {n} samples, float64 numpy); "
          f"restated optimiser {cpu['restated_optimiser_ms_per_fit']} ms per fit")
    print(f"  evaluations stage 1 {cpu['evaluations_stage1']}, stage 2 {cpu['evaluations_stage2']}; {same} of {n} rows with the kernel's iteration counts; "
          f"device objective above scipy's by at most {excess:.3e}")
    res = {"device": dev, "host": cpu, "ratio_device_over_scipy": round(dev["fits_per_s_median"] / cpu["scipy_fits_per_s"], 1)}
    if args.margin:
        import facefit_cases as C

        res["FIT_OBJ_MARGIN"] = C.fit_obj_margin()
        print(f"FIT_OBJ_MARGIN (tests/facefit_cases.py) {res['FIT_OBJ_MARGIN']:.3e}")
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
