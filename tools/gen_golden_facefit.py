#!/usr/bin/env python3
"""Golden vectors for the face-model fit: the reference's own objective `DeformableHeadFitting.lossfunc` and point weights
`_make_target_points_and_weights` (scripts/DsWflwFitFaceModel.ipynb), evaluated in float64.

The notebook is read as JSON at run time.  Two of its code cells are executed in a prepared namespace: the cell that builds the index
lists face_left / face_right, and the cell that defines PosedDeformableHead and DeformableHeadFitting, cut before its last two statements
(which construct a fitter and fit a sample of a dataset that is not here).  The namespace holds the reference's own modules
(DeformableHeadKeypoints, GaussianMixture, rigid_transformation_25d, utils, Batch) through oracle/tools/ref_shims.py - the SYNTHETIC
68-keypoint basis of oracle/synth.py stands in for the missing BFM blob, the committed mixture for shapeparams_gmm.h5 - and a name-only
stand-in for torchmin, which is not installed: nothing here minimises.  One adaptation: the notebook passes a plain quaternion tensor to
rigid_transformation_25d, which in the reference's current modelcomponents.py takes a rotation object; the namespace's function wraps
the tensor in the reference's QuatRepr and calls the reference's function.  Nothing of the notebook's text is written anywhere: the
fixture holds arrays only.

  x [64,57], target [64,68,2], weight [64,68]   float32 inputs (the kernel's types), widened to float64 for the reference
  f [64]                                        lossfunc in float64
     rows 0..7 have a size within 0.03..0.08 (the size constraint dominates), rows 8..15 residuals far outside beta = 0.1, rows 16..23
     far inside, the rest mixed; rows 24..27 have every weight of one face side 0
  wpose [32,4], w2d [32,68], w3d [32,68]        start poses with headings over +-90 degrees, both signs at 1e-3 degrees and the identity,
                                                and the weights for 2-D targets and for fit_3d_projections

Build container only.  Re-run with  python tools/gen_golden_facefit.py ; writes tests/golden/facefit.npz."""
from __future__ import annotations

import ast
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle", "tools"))
sys.path.insert(0, REPO)

import ref_shims  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
torch = ref_shims.install(synthetic_bfm=True, gmm_npz=os.path.join(GOLD, "shapeparams_gmm.npz"))
torch.set_default_dtype(torch.float64)

from scipy.spatial.transform import Rotation  # noqa: E402
from trackertraincode import utils  # noqa: E402
from trackertraincode.datasets.batch import Batch  # noqa: E402
from trackertraincode.neuralnets import modelcomponents  # noqa: E402
from trackertraincode.neuralnets.rotrepr import QuatRepr  # noqa: E402

NOTEBOOK = os.path.join(ref_shims.REFERENCE_ROOT, "scripts", "DsWflwFitFaceModel.ipynb")
SEED, N, NW = 2027, 64, 32


def notebook_classes():
    with open(NOTEBOOK) as f:
        cells = ["".join(c["source"]) for c in json.load(f)["cells"] if c["cell_type"] == "code"]
    (lists,) = [c for c in cells if "face_left =" in c]
    (classes,) = [c for c in cells if "class DeformableHeadFitting" in c]
    ns = {"torch": torch, "np": np, "Rotation": Rotation, "utils": utils, "Batch": Batch, "torchmin": types.ModuleType("torchmin"),
          "DeformableHeadKeypoints": modelcomponents.DeformableHeadKeypoints, "GaussianMixture": modelcomponents.GaussianMixture,
          "rigid_transformation_25d": lambda q, t, s, pts: modelcomponents.rigid_transformation_25d(QuatRepr(q), t, s, pts)}
    exec(compile(lists, "<index-list cell>", "exec"), ns)
    tree = ast.parse(classes)
    tree.body = tree.body[:-2]
    exec(compile(tree, "<DeformableHeadFitting cell>", "exec"), ns)
    return ns


if __name__ == "__main__":
    ns = notebook_classes()
    fitter2d, fitter3d = ns["DeformableHeadFitting"](False), ns["DeformableHeadFitting"](True)
    rng = np.random.default_rng(SEED)

    q = rng.standard_normal((N, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    q *= rng.uniform(0.8, 1.25, (N, 1))  # not normalised: the norm constraint and the projection are exercised
    c = np.concatenate([rng.uniform(-0.2, 0.2, (N, 2)), rng.uniform(0.3, 0.8, (N, 1))], -1)
    c[:8, 2] = np.linspace(0.03, 0.08, 8)
    x = np.concatenate([q, c, rng.normal(0, 0.7, (N, 50))], -1).astype(np.float32)
    with torch.no_grad():
        pts = np.stack([fitter2d.evalheadmodel(torch.from_numpy(x[i].astype(np.float64))).numpy() for i in range(N)])
    spread = np.full(N, 0.08)
    spread[8:16], spread[16:24] = 0.6, 0.01
    target = (pts[..., :2] + rng.normal(0, 1, (N, 68, 2)) * spread[:, None, None]).astype(np.float32)
    weight = rng.uniform(0, 1, (N, 68)).astype(np.float32)
    weight[24:26, ns["face_left"]] = 0.0
    weight[26:28, ns["face_right"]] = 0.0
    with torch.no_grad():
        f = np.array([float(fitter2d.lossfunc(*(torch.from_numpy(a[i].astype(np.float64)) for a in (x, target, weight)))) for i in range(N)])
    res = np.abs(pts[..., :2] - target)
    print("residuals below beta per row block:", [(res[a:b] < 0.1).mean().round(3) for a, b in ((0, 8), (8, 16), (16, 24), (24, 64))])
    print("f: min %.4g max %.4g" % (f.min(), f.max()))

    head = np.concatenate([np.linspace(-90.0, 90.0, NW - 3), [-1e-3, 1e-3]])
    rots = Rotation.from_euler("YXZ", np.stack([head, rng.uniform(-25, 25, NW - 1), rng.uniform(-25, 25, NW - 1)], -1), degrees=True)
    wpose = np.concatenate([rots.as_quat(), [[0.0, 0.0, 0.0, 1.0]]])
    w2d = np.stack([fitter2d._make_target_points_and_weights({"pose": torch.from_numpy(p), "pt2d_68": torch.zeros(68, 2)})[1].numpy() for p in wpose])
    w3d = np.stack([fitter3d._make_target_points_and_weights({"pose": torch.from_numpy(p), "pt3d_68": torch.zeros(68, 3)})[1].numpy() for p in wpose])
    print("distinct weights (2-D):", np.unique(w2d.round(6)).size, "; all ones (3-D):", bool((w3d == 1).all()))

    path = os.path.join(GOLD, "facefit.npz")
    np.savez_compressed(path, x=x, target=target, weight=weight, f=f, wpose=wpose, w2d=w2d, w3d=w3d)
    assert os.path.getsize(path) < 1024 * 1024, os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes")
