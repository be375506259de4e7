#!/usr/bin/env python3
"""Golden vectors for the ensemble average of the pseudo-labelling step: the reference's own `quat_average`
(neuralnets/torchquaternion.py:239-256) and `np.average` (scripts/add_pose_pseudolabels.py:124-127) on stacks of member predictions.

For E in (1, 2, 3, 5, 16) and N = 64 rows: float32 unit quaternions = a random base rotation times a rotation-vector perturbation of
sigma 0.05 rad, with a random sign per member and row, plus random coord / pt3d_68 / shapeparam stacks (pt3d_68 in whole pixels 0..255 stored as uint8 and
shapeparam in steps of 1/32, which keeps the compressed file below the size limit of a committed fixture).  The other inputs are stored
as float32, the reference's outputs as float64.  A row is redrawn while the two largest component sums of |q| are closer than 1e-2 * E or a member's
pivot component is below 1e-2 in magnitude: no float32 rounding can then change a sign decision, and every row is compared.

Build container only (it imports the reference through oracle/tools/ref_shims.py; nothing of the reference is copied).  Re-run with
    python tools/gen_golden_ensemble.py
Writes tests/golden/ensemble.npz."""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle", "tools"))
sys.path.insert(0, REPO)

import ref_shims  # noqa: E402

ref_shims.install()
from scipy.spatial.transform import Rotation  # noqa: E402
from trackertraincode.neuralnets.torchquaternion import quat_average  # noqa: E402

MEMBERS, N, SIGMA, SEED = (1, 2, 3, 5, 16), 64, 0.05, 2026


def draw_rows(rng, E, n):
    base = Rotation.random(n, random_state=rng)
    q = np.stack([(base * Rotation.from_rotvec(rng.normal(0.0, SIGMA, (n, 3)))).as_quat() for _ in range(E)])
    return (q * rng.choice([-1.0, 1.0], (E, n, 1))).astype(np.float32)


def decided(q):
    """Rows whose pivot and member signs no float32 rounding can change."""
    sums = np.sort(np.abs(q.astype(np.float64)).sum(0), axis=-1)
    pivot = np.argmax(np.abs(q.astype(np.float64)).sum(0), axis=-1)
    comp = np.take_along_axis(q, pivot[None, :, None], axis=-1)[..., 0]
    return (sums[:, -1] - sums[:, -2] >= 1e-2 * q.shape[0]) & (np.abs(comp).min(0) >= 1e-2)


if __name__ == "__main__":
    rng = np.random.default_rng(SEED)
    out, redrawn = {}, 0
    for E in MEMBERS:
        q = draw_rows(rng, E, N)
        while True:
            bad = np.flatnonzero(~decided(q))
            if not len(bad):
                break
            redrawn += len(bad)
            q[:, bad] = draw_rows(rng, E, len(bad))
        coord = np.concatenate([rng.uniform(0, 640, (E, N, 2)), rng.uniform(20, 200, (E, N, 1))], -1).astype(np.float32)
        # (27 x 64 x 204 random float32 do not fit a 1 MiB file: pt3d_68 is drawn in whole pixels 0..255 and stored as uint8, shapeparam in steps of 1/32)
        pts = rng.integers(0, 256, (E, N, 68, 3)).astype(np.uint8)
        shape = (np.rint(rng.normal(0, 1, (E, N, 50)) * 32) / 32).astype(np.float32)
        out[f"E{E}/pose"], out[f"E{E}/coord"], out[f"E{E}/pt3d_68"], out[f"E{E}/shapeparam"] = q, coord, pts, shape
        avg = quat_average(q.astype(np.float64))  # (a copy: the reference flips signs in place)
        pivot = np.argmax(np.abs(q.astype(np.float64)).sum(0), -1)
        print(f"E={E}: min pivot component {np.abs(np.take_along_axis(q, pivot[None, :, None], -1)).min():.3f}")
        out[f"E{E}/avg_pose"] = avg
        for k in ("coord", "pt3d_68", "shapeparam"):
            out[f"E{E}/avg_{k}"] = np.average(out[f"E{E}/{k}"].astype(np.float64), axis=0)
    path = os.path.join(REPO, "tests", "golden", "ensemble.npz")
    np.savez_compressed(path, members=np.array(MEMBERS, np.int32), **out)
    assert os.path.getsize(path) < 1024 * 1024, os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes;", redrawn, "rows redrawn")
