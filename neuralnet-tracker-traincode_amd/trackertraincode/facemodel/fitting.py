"""Fit the deformable face model to 68 landmarks on the device (reference: scripts/DsWflwFitFaceModel.ipynb and
scripts/DsLapaMegafaceFitFaceModel.ipynb, class DeformableHeadFitting - the readme's step "fit the face model" between the pseudo
labels and the large-pose expansions).  The reference fits one sample at a time on the CPU with two BFGS runs of the third-party
torchmin; here a batch is one launch of ttk_facefit (csrc/facefit.hip, include/ttk.h): one workgroup per sample, float64 throughout,
the project's own two-stage BFGS (DESIGN.md 4.5.3 - a deliberate deviation, torchmin's iterates cannot be pinned without the package).

    fitter = FaceModelFitter.from_checkpoint("run/best.ckpt")            # or FaceModelFitter(keypts, keyeigvecs)
    out = fitter.fit(roi, pose, coord, pt2d_68)                            # image pixels in, image pixels out
    out["pose"], out["coord"], out["shapeparam"], out["pt3d_68"], out["objective"], out["status"], out["iterations"]
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
from torch import Tensor

from . import keypoints68 as KP

# the index lists of the notebook's third cell
FACE_LEFT = (KP.chin_left + KP.eyecorners_left + KP.eye_left_top + KP.eye_left_bottom + KP.uppermouth_left + KP.lowermouth_left
             + KP.brows_left + KP.nose_left)
FACE_RIGHT = (KP.chin_right + KP.eyecorners_right + KP.eye_right_top + KP.eye_right_bottom + KP.uppermouth_right + KP.lowermouth_right
              + KP.brows_right + KP.nose_right)
ANGLE_CUTOFF_JAW, ANGLE_CUTOFF_FACE_SIDE = 20.0 * math.pi / 180.0, 70.0 * math.pi / 180.0
FOCUS_ROI_FACTOR = 1.2  # the notebook's FocusRoi(224, extent_factor=1.2)
VIEW_SIZE = 224         # its crop size; it cancels out of the normalised coordinates (see FaceModelFitter.fit)
STATUS_NAMES = {0: "converged", 1: "iteration limit", 2: "line search failed", 3: "non-finite input"}


def _mask(indices) -> Tensor:
    m = torch.zeros(68, dtype=torch.bool)
    m[list(indices)] = True
    return m


def heading(pose: Tensor) -> Tensor:
    """`utils.as_hpb(Rotation.from_quat(pose))[0]` = as_euler("YXZ")[0]: with R = Ry(h) Rx(p) Rz(b), h = atan2(R02, R22)."""
    q = pose.to(torch.float64)
    q = q / q.norm(dim=-1, keepdim=True)
    i, j, k, w = q.unbind(-1)
    return torch.atan2(2.0 * (i * k + j * w), 1.0 - 2.0 * (i * i + j * j))


def facefit_point_weights(pose: Tensor, fit_3d_projections: bool = False) -> Tensor:
    """The point weights of `_make_target_points_and_weights` for a batch of start poses [B,4] -> float64 [B,68], statement by statement:
    ones; with 2-D targets the chin points x 0.1 (both lists hold point 8: x 0.01), then for a heading h < 0 the right face side is SET to
    max(0, 1 - |h| / 70 deg) and then the right chin to max(0, 1 - |h| / 20 deg) (which replaces the 0.1), mirrored for h > 0.
    fit_3d_projections: all ones."""
    B = pose.shape[0]
    w = torch.ones((B, 68), dtype=torch.float64, device=pose.device)
    if fit_3d_projections:
        return w
    dev = pose.device
    chin_l, chin_r, face_l, face_r = (_mask(ix).to(dev) for ix in (KP.chin_left, KP.chin_right, FACE_LEFT, FACE_RIGHT))
    w = torch.where(chin_l, w * 0.1, w)
    w = torch.where(chin_r, w * 0.1, w)
    h = heading(pose)
    jaw = (1.0 - h.abs() / ANGLE_CUTOFF_JAW).clamp_min(0.0)[:, None]
    side = (1.0 - h.abs() / ANGLE_CUTOFF_FACE_SIDE).clamp_min(0.0)[:, None]
    neg, pos = (h < 0)[:, None], (h > 0)[:, None]
    w = torch.where(neg & face_r, side, w)
    w = torch.where(neg & chin_r, jaw, w)
    w = torch.where(pos & face_l, side, w)
    w = torch.where(pos & chin_l, jaw, w)
    return w


class FaceModelFitter:
    """See the module docstring.  `keypts` [68,3], `keyeigvecs` [50,68,3]: the basis of DeformableHeadKeypoints.  `gmm`: None (the packaged
    shapeparams_gmm.npz), a path to such a file, or a modelcomponents.GaussianMixture with at most 16 components.  `iters`, `gtol`: the
    iteration limits and gradient tolerances (infinity norm) of the two stages - the reference's max_iter = 50 / 100 and tol = default /
    0.0005, read with scipy's conventions."""

    def __init__(self, keypts, keyeigvecs, gmm=None, fit_3d_projections: bool = False, device: str | torch.device = "cuda",
                 iters=(50, 100), gtol=(1e-5, 5e-4)):
        from ..neuralnets.modelcomponents import GaussianMixture

        kp = torch.as_tensor(np.asarray(keypts) if not torch.is_tensor(keypts) else keypts).detach().to(torch.float32).cpu()
        ev = torch.as_tensor(np.asarray(keyeigvecs) if not torch.is_tensor(keyeigvecs) else keyeigvecs).detach().to(torch.float32).cpu()
        if tuple(kp.shape) != (68, 3) or tuple(ev.shape) != (50, 68, 3):
            raise ValueError(f"FaceModelFitter: keypts must be [68,3] and keyeigvecs [50,68,3], got {tuple(kp.shape)} and {tuple(ev.shape)}")
        if not bool(kp.any()) and not bool(ev.any()):
            raise ValueError("FaceModelFitter: the face-model basis is all zero - the BFM blob (facemodel/bfm_keypoints.npz) is absent and nothing "
                             "set one (a checkpoint's landmarks.deformablekeypoints buffers, DeformableHeadKeypoints.set_basis)")
        if gmm is None:
            gmm = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shapeparams_gmm.npz")
        if isinstance(gmm, (str, os.PathLike)):
            gmm = GaussianMixture.from_npz(str(gmm))
        if not 1 <= gmm.n_components <= 16 or gmm.means.shape[-1] != 50:
            raise ValueError(f"FaceModelFitter: the mixture must have 1..16 components over 50 shape parameters, got {tuple(gmm.means.shape)}")
        if len(iters) != 2 or len(gtol) != 2 or min(iters) < 0 or not min(gtol) > 0:
            raise ValueError(f"FaceModelFitter: iters must be two non-negative limits and gtol two positive tolerances, got {iters} and {gtol}")
        self.device = torch.device(device)
        self.fit_3d_projections = bool(fit_3d_projections)
        self.iters, self.gtol = (int(iters[0]), int(iters[1])), (float(gtol[0]), float(gtol[1]))
        # the mixture's constants in float64, as ShapePlausibilityLoss prepares them
        w64, mu64, sinv64 = gmm.weights.to(torch.float64), gmm.means.to(torch.float64), gmm.scales_inv.to(torch.float64)
        ck = torch.log(w64) + torch.log(sinv64).sum(-1) - gmm.norm_constant.to(torch.float64)
        self.K = int(gmm.n_components)
        self._kp, self._ev = kp.contiguous().to(self.device), ev.contiguous().to(self.device)
        self._ck, self._mu, self._sinv = (t.contiguous().to(self.device) for t in (ck, mu64, sinv64))

    @classmethod
    def from_module(cls, module, **kw) -> "FaceModelFitter":
        """The basis of a DeformableHeadKeypoints module (or anything with `keypts` / `keyeigvecs` buffers)."""
        return cls(module.keypts, module.keyeigvecs, **kw)

    @classmethod
    def from_checkpoint(cls, path: str, **kw) -> "FaceModelFitter":
        """The basis from the `landmarks.deformablekeypoints.*` buffers of a checkpoint (neuralnets/io.py format, or a bare state dict)."""
        contents = torch.load(path, weights_only=True, map_location="cpu")
        sd = contents.get("state_dict", contents)
        names = ["landmarks.deformablekeypoints.keypts", "landmarks.deformablekeypoints.keyeigvecs"]
        missing = [n for n in names if n not in sd]
        if missing:
            raise ValueError(f"{path}: no {missing} in the checkpoint (a network without the landmark head?)")
        return cls(sd[names[0]], sd[names[1]], **kw)

    # ---- the two entry points ------------------------------------------------------------------
    def _model_args(self):
        from .. import _hip

        return tuple(_hip.ptr(t) for t in (self._kp, self._ev, self._ck, self._mu, self._sinv)) + (self.K,)

    def _f32(self, t, shape, what) -> Tensor:
        t = torch.as_tensor(t).to(self.device, torch.float32).contiguous()
        if tuple(t.shape[1:]) != shape:
            raise ValueError(f"FaceModelFitter: {what} must be [B,{','.join(map(str, shape))}], got {tuple(t.shape)}")
        return t

    def objective(self, x, target_xy, weights, n_free: int = 57):
        """f [B] and df/dx [B,57] (float64) at x [B,57]: ttk_facefit_objective, the device function the optimiser calls."""
        from .. import _hip

        x, y, w = self._f32(x, (57,), "x"), self._f32(target_xy, (68, 2), "target_xy"), self._f32(weights, (68,), "weights")
        B = x.shape[0]
        f = torch.empty((B,), dtype=torch.float64, device=self.device)
        g = torch.empty((B, 57), dtype=torch.float64, device=self.device)
        _hip.lib().call("ttk_facefit_objective", _hip.ptr(x), _hip.ptr(y), _hip.ptr(w), *self._model_args(), B, int(n_free), _hip.ptr(f), _hip.ptr(g))
        return f, g

    @torch.no_grad()
    def fit_normalized(self, pose, coord, target_xy, weights=None, shapeparam=None):
        """Fit in the crop's normalised [-1, 1] coordinates.  pose [B,4] (ijkw) and coord [B,3] are the start values, target_xy [B,68,2]
        the landmarks, weights [B,68] the point weights (default: facefit_point_weights of the start pose), shapeparam [B,50] the start
        shape (default zeros, as the reference starts).  One launch, no synchronisation.  Returns a Batch: pose (unit), coord, shapeparam,
        pt3d_68, objective_start, objective (float64), status (int32; STATUS_NAMES), iterations [B,2] (int32)."""
        from .. import _hip
        from ..datasets.batch import Batch, Metadata
        from ..datatransformation.tensors.affinetrafo import FieldCategory

        pose, coord = self._f32(pose, (4,), "pose"), self._f32(coord, (3,), "coord")
        y = self._f32(target_xy, (68, 2), "target_xy")
        B = pose.shape[0]
        s = torch.zeros((B, 50), dtype=torch.float32, device=self.device) if shapeparam is None else self._f32(shapeparam, (50,), "shapeparam")
        w = facefit_point_weights(pose, self.fit_3d_projections) if weights is None else weights
        w = self._f32(w, (68,), "weights")
        if not (coord.shape[0] == y.shape[0] == s.shape[0] == w.shape[0] == B):
            raise ValueError("FaceModelFitter: the inputs have different batch sizes")
        x0 = torch.cat([pose, coord, s], dim=-1).contiguous()
        x = torch.empty_like(x0)
        pts = torch.empty((B, 68, 3), dtype=torch.float32, device=self.device)
        f = torch.empty((B, 2), dtype=torch.float64, device=self.device)
        status = torch.empty((B,), dtype=torch.int32, device=self.device)
        iters = torch.empty((B, 2), dtype=torch.int32, device=self.device)
        _hip.lib().call("ttk_facefit", _hip.ptr(x0), _hip.ptr(y), _hip.ptr(w), *self._model_args(), B, self.iters[0], self.gtol[0],
                        self.iters[1], self.gtol[1], _hip.ptr(x), _hip.ptr(pts), _hip.ptr(f), _hip.ptr(status), _hip.ptr(iters))
        cats = {"pose": FieldCategory.quat, "coord": FieldCategory.xys, "pt3d_68": FieldCategory.points}
        return Batch(Metadata(0, B, categories=cats), pose=x[:, :4].contiguous(), coord=x[:, 4:7].contiguous(), shapeparam=x[:, 7:].contiguous(),
                     pt3d_68=pts, objective_start=f[:, 0].contiguous(), objective=f[:, 1].contiguous(), status=status, iterations=iters)

    def view_transform(self, roi: Tensor):
        """(integer view box [B,4], Affine2d image pixels -> the view's [-1, 1]) of the reference's FocusRoi(., 1.2): `_compute_view_roi`
        with scale 1.2 and no shift, rounded to integers - GeneralFocusRoi.transform_for, the arithmetic the crop uses."""
        from ..datatransformation.batch.geometric import GeneralFocusRoi, NoRoiRandomization
        from ..datatransformation.tensors.affinetrafo import position_normalization

        roi = torch.as_tensor(roi).to(self.device, torch.float32)
        params = NoRoiRandomization(FOCUS_ROI_FACTOR)(tuple(roi.shape[:-1]), device=self.device)
        view, tr = GeneralFocusRoi(None, VIEW_SIZE).transform_for(roi, params)
        return view, position_normalization(VIEW_SIZE, VIEW_SIZE).to(self.device) @ tr

    @torch.no_grad()
    def fit(self, roi, pose, coord, landmarks_xy):
        """Fit in image pixels: roi [B,4] the face boxes, pose [B,4] / coord [B,3] the start values (e.g. pseudo labels), landmarks_xy
        [B,68,2] (or [B,68,3], of which xy is used) the landmarks.  The labels are mapped into the [-1, 1] coordinates of the reference's
        FocusRoi(., 1.2) view with apply_affine2d, fitted, and mapped back as Predictor.to_image_coordinates maps predictions.  The view's
        pixel size cancels: box -> [0, N] -> [-1, 1] is the same map for every N (up to float32 rounding), no image is resampled.
        Returns the Batch of fit_normalized with pose, coord and pt3d_68 in image pixels, plus view_roi."""
        from ..datatransformation.tensors.affinetrafo import FieldCategory, apply_affine2d

        view, to_norm = self.view_transform(roi)
        pose = torch.as_tensor(pose).to(self.device, torch.float32)
        coord = torch.as_tensor(coord).to(self.device, torch.float32)
        xy = torch.as_tensor(landmarks_xy).to(self.device, torch.float32)[..., :2].contiguous()
        out = self.fit_normalized(apply_affine2d(to_norm, "pose", pose, FieldCategory.quat), apply_affine2d(to_norm, "coord", coord, FieldCategory.xys),
                                  apply_affine2d(to_norm, "pt2d_68", xy, FieldCategory.points))
        back = to_norm.inv()
        for k in ("pose", "coord", "pt3d_68"):
            out[k] = apply_affine2d(back, k, out[k], out.meta.categories[k])
        out["view_roi"] = view
        return out
