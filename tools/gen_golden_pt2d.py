#!/usr/bin/env python3
"""Golden vectors for 2-D landmarks under the crop: the reference's own `transform_keypoints` (datatransformation/tensors/affinetrafo.py:61-72,
its 2-D branch :70-71 over `transform_points` :51-52) applied to [68, 2] point sets, sample by sample as the reference's loaders do -

  crop transform (Affine2d.trs: scale, turn, shift)  ->  horizontal_flip_and_rot_90 with each of its six (rot_dir, do_flip) draws forced
  (batch/geometric.py:234-267, np.random patched as in oracle/tools/gen_golden_eval.py)  ->  position_normalization (normalize_batch)

Build container only (it imports the reference through oracle/tools/ref_shims.py; nothing of the reference is copied).  Re-run with
    python tools/gen_golden_pt2d.py
Writes tests/golden/augment_pt2d.npz (inputs are stored too), a few KB."""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle", "tools"))
sys.path.insert(0, REPO)

import ref_shims  # noqa: E402

torch = ref_shims.install()
from trackertraincode.datasets.batch import Batch, Metadata  # noqa: E402
from trackertraincode.datasets.dshdf5pose import FieldCategory  # noqa: E402
from trackertraincode.datatransformation.batch import geometric as G  # noqa: E402
from trackertraincode.datatransformation.tensors.affinetrafo import position_normalization, transform_keypoints  # noqa: E402
from trackertraincode.neuralnets.affine2d import Affine2d  # noqa: E402

N = 129
PER_CODE = 2  # samples per (rot_dir, do_flip) draw

if __name__ == "__main__":
    rng = np.random.default_rng(2025)
    norm = position_normalization(N, N)
    trs, codes, pts_in, crop_px, out = [], [], [], [], []
    for rot_dir in (-1, 0, 1):
        for do_flip in (0, 1):
            for _ in range(PER_CODE):
                pts = rng.uniform(10, 90, (68, 2)).astype(np.float32)
                tr = Affine2d.trs(translations=torch.tensor(rng.uniform(-20, 20, 2).astype(np.float32)),
                                  angles=torch.tensor(np.float32(rng.choice([-1.0, 0.0, 1.0]) * np.pi / 6)),
                                  scales=torch.tensor(np.float32(rng.uniform(1.0, 2.0))))
                in_crop = transform_keypoints(tr, torch.from_numpy(pts.copy()))
                sample = Batch(Metadata(N, 0, categories={"pt2d_68": FieldCategory.points}), {"pt2d_68": in_crop.clone()})
                G.np.random.randint = lambda lo, hi, _f=do_flip: 0 if _f else 1  # the two draws of :236-237
                G.np.random.choice = lambda a, p=None, _r=rot_dir: _r
                res = G.horizontal_flip_and_rot_90(0.01, sample)
                trs.append(tr.tensor().numpy())
                codes.append((rot_dir + 1) * 2 + do_flip)
                pts_in.append(pts)
                crop_px.append(in_crop.numpy())
                out.append(transform_keypoints(norm, res["pt2d_68"]).numpy())
    path = os.path.join(REPO, "tests", "golden", "augment_pt2d.npz")
    np.savez_compressed(path, N=np.int32(N), tr=np.stack(trs).astype(np.float32), code=np.array(codes, np.int32), pt2d_68=np.stack(pts_in),
                        crop_pt2d_68=np.stack(crop_px).astype(np.float32), out_pt2d_68=np.stack(out).astype(np.float32))
    assert os.path.getsize(path) < 64 * 1024, os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes")
