"""Evaluation path: `Predictor` (face box -> 129x129 crop -> network -> predictions in image coordinates) and the pose /
landmark error metrics (reference: trackertraincode/eval.py:158-252, 295-440; scripts/evaluate_pose_network.py).

The crop is produced on the MI355X by the affine-warp kernels of csrc/warp.hip (the same kernels as the training
augmentation, with the deterministic parameters of the reference's `FocusRoi`: enlargement 1.1, no shift, no rotation),
the network runs its eval-mode HIP path, and the back-transformation to image coordinates is the inverse of the crop
transform applied with `apply_affine2d`.  The reference crops with OpenCV (`croprescale_image_cv2`, area / linear
filters); this build resamples bilinearly like its `affine_transform_image_torch` - predictions on real images differ
from an OpenCV crop at the level of the resampling filter, which is why MAE parity is asserted against the CPU
oracle running the SAME resampling (tests/test_eval_gpu.py), not against stored reference numbers.
torchmetrics is not a dependency here: the metrics are small accumulators with the reference's names and formulas."""
from __future__ import annotations

from typing import Dict, List, NamedTuple

import numpy as np
import torch
from torch import Tensor

from . import _hip, utils
from .datasets.batch import Batch, Metadata
from .datatransformation.batch.geometric import NoRoiRandomization
from .datatransformation.gpu import GpuFocusRoiAugment
from .datatransformation.tensors.affinetrafo import FieldCategory, apply_affine2d, position_normalization
from .neuralnets import torchquaternion
from .neuralnets.affine2d import Affine2d


class Predictor:
    """`predict_batch(images, rois)`: images = list of uint8 tensors [H,W] / [H,W,1] / [H,W,3] (grey levels or RGB,
    any sizes) or one [B,1,H,W] tensor; rois [B,4] = (x0, y0, x1, y1) face boxes in pixels.  Returns a Batch with the
    network outputs mapped back to image coordinates: coord [B,3] (x, y, head size in pixels), pose [B,4], roi [B,4],
    pt3d_68 [B,68,3] (when the network has the landmark head) - reference :185-208."""

    def __init__(self, net: torch.nn.Module, focus_roi_expansion_factor: float = 1.1, device: str | torch.device = "cuda",
                 resample: str = "bilinear"):
        self._net = net.to(device).eval()
        self._device = torch.device(device)
        self._crop = GpuFocusRoiAugment(new_size=net.input_resolution, make_params=NoRoiRandomization(focus_roi_expansion_factor),
                                        resample=resample)

    @property
    def input_resolution(self) -> int:
        return self._net.input_resolution

    @staticmethod
    def _grey(img: Tensor) -> Tensor:
        if img.dim() == 3 and img.shape[-1] == 3:  # ITU-R 601 luma, as the training data is stored (grey 8 bit)
            w = torch.tensor([0.299, 0.587, 0.114], dtype=torch.float32, device=img.device)
            img = (img.to(torch.float32) * w).sum(-1).round().clamp(0, 255).to(torch.uint8)
        elif img.dim() == 3:
            img = img[..., 0]
        return img

    def crop_batch(self, images, rois: Tensor) -> Batch:
        """Normalised crops [B,1,N,N] (whitened) + the pixel transforms image -> crop used for the back-transformation."""
        rois = rois.to(self._device, torch.float32)
        if torch.is_tensor(images):
            groups = {tuple(images.shape[-2:]): list(range(images.shape[0]))}
            get = lambda i: images[i, 0]
        else:
            groups: Dict[tuple, List[int]] = {}
            for i, im in enumerate(images):
                groups.setdefault(tuple(self._grey(im).shape), []).append(i)
            get = lambda i: self._grey(images[i])
        B = rois.shape[0]
        N = self.input_resolution
        crops = torch.empty((B, 1, N, N), dtype=torch.float32, device=self._device)
        trs = torch.empty((B, 2, 3), dtype=torch.float32, device=self._device)
        for _, idx in groups.items():  # images of one size are warped together
            src = torch.stack([get(i).to(self._device) for i in idx])[:, None].contiguous()
            sub = Batch(Metadata(tuple(src.shape[-2:][::-1]), len(idx)), image=src, roi=rois[idx])
            out = self._crop(sub)
            crops[idx], trs[idx] = out["image"], out.transform
        return Batch(Metadata(N, B), image=crops, image_transform=trs)

    @torch.no_grad()
    def predict_batch(self, images, rois: Tensor) -> Batch:
        if self._device.type == "cuda":
            _hip.lib().clear_stale_error("the start of an evaluation batch")
        crop = self.crop_batch(images, rois)
        preds = self._net(crop["image"])
        return self.to_image_coordinates(preds, crop["image_transform"], self.input_resolution)

    @staticmethod
    def to_image_coordinates(preds, image_transform: Tensor, N: int) -> Batch:
        """Predictions in the crop's [-1, 1] coordinates -> image pixels (reference :199-206: unnormalize_batch, then the
        image_backtransform that FocusRoi stored = the inverse of the crop's point transform).  `image_transform`: [B, 2, 3] image pixels ->
        crop pixels.  Pinned to the reference by tests/golden/eval.npz (oracle/tools/gen_golden_eval.py)."""
        # image pixels -> crop pixels -> [-1, 1]: invert the whole chain for the predictions
        to_norm = position_normalization(N, N).to(image_transform.device) @ Affine2d(image_transform)
        back = to_norm.inv()
        cats = {"coord": FieldCategory.xys, "pose": FieldCategory.quat, "pt3d_68": FieldCategory.points, "roi": FieldCategory.roi}
        out = {}
        for k, c in cats.items():
            if k in preds:
                v = preds[k]
                out[k] = apply_affine2d(back, k, v.value if hasattr(v, "value") else v, c)
        for k in ("coord_scales", "pose_scales_tril", "shapeparam", "unnormalized_quat"):
            if k in preds:
                out[k] = preds[k]
        meta = Metadata(N, int(image_transform.shape[0]), categories=dict(cats))
        return Batch(meta, out)

    def evaluate(self, metric, samples, batchsize: int = 128):
        """`samples`: iterable of dicts with "image", "roi" and the labels the metric reads (reference :210-222)."""
        for chunk in utils.iter_batched(samples, batchsize):
            images = [s["image"] for s in chunk]
            keys = [k for k in chunk[0] if k != "image"]
            targets = Batch(Metadata(0, len(chunk)), {k: torch.stack([torch.as_tensor(s[k]) for s in chunk]).to(self._device) for k in keys})
            targets["image_hw"] = torch.as_tensor([tuple(im.shape[:2]) for im in images])  # what AlignedRotationErrorMetric("perspective") reads
            preds = self.predict_batch(images, targets["roi"])
            metric.update(preds, targets)
        return metric.compute()

    @torch.no_grad()
    def predict_cropped_normalized_batch(self, images: Tensor) -> Batch:
        """The network on crops that are already cut out, scaled to [B,1,N,N] and whitened (what `crop_batch` returns as "image");
        nothing is transformed back: the predictions stay in the crop's [-1, 1] coordinates (reference :228-243)."""
        if self._device.type == "cuda":
            _hip.lib().clear_stale_error("the start of an evaluation batch")
        preds = dict(self._net(images.to(self._device)))
        cats = {"coord": FieldCategory.xys, "pose": FieldCategory.quat, "pt3d_68": FieldCategory.points}
        return Batch(Metadata(int(images.shape[-1]), int(images.shape[0]), categories={k: c for k, c in cats.items() if k in preds}), preds)

    def evaluate_cropped_normalized(self, metric, batches):
        """`batches`: iterable of Batches (or dicts) with "image" = normalised crops and the labels the metric reads, in the crop's
        coordinates (reference :245-252)."""
        for batch in batches:
            metric.update(self.predict_cropped_normalized_batch(batch["image"]), batch)
        return metric.compute()


# ---------------------------------------------------------------------------------------------
# the face localizer (reference: neuralnets/models.py LocalizerNet; the reference tree holds no code that maps its boxes to pixels)
# ---------------------------------------------------------------------------------------------
class Localizer:
    """The face localizer on whole frames: `localize(frames)` takes uint8 or float32 grey-level frames [B, H, W] of any one size and
    returns a Batch with logit [B], hasface [B] (the sigmoid of the logit), roi [B, 4] in frame pixels, roi_normalized [B, 4] (the
    network's own box in the input's [-1, 1] coordinates) and letterbox [B, 3] = (s, ox, oy).  One ttk_localizer_input (letterbox into 224 x 288: uniform scale
    s = min(288 / W, 224 / H), centred with offsets ox, oy, exact area averages, outside the frame grey level 0, whitened like the pose
    crops) plus one LocalizerNet forward (csrc/localizer.hip); nothing is read on the host.

    The map from the network's box to pixels is THIS PROJECT'S convention - the reference tree has none: input pixels
    X = (x + 1) * 144, Y = (y + 1) * 112, frame pixels ((X - ox) / s, (Y - oy) / s); ttk_track_reacquire (csrc/localizer_math.h) rounds
    the same float32 steps."""

    MUL, ADD = 1.0 / 256.0, -0.5  # whitening of GpuFocusRoiAugment, as the pose crops

    def __init__(self, net: torch.nn.Module, device: str | torch.device = "cuda", threshold: float = 0.5):
        self._net = net.to(device).eval()
        self._device = torch.device(device)
        self.threshold = float(threshold)

    def run(self, frames: Tensor, t_dev: Tensor | None = None):
        """frames [S, T, H, W] on the device, contiguous; frame *t_dev of every sequence (None: frame 0) -> (out [S, 5], lb [S, 3] =
        (s, ox, oy)).  Enqueues only."""
        S, T, Hs, Ws = (int(v) for v in frames.shape)
        H, W = self._net.input_resolution
        x = torch.empty((S, 1, H, W), dtype=torch.float32, device=frames.device)
        lb = torch.empty((S, 3), dtype=torch.float32, device=frames.device)
        _hip.lib().call("ttk_localizer_input", _hip.fast_ptr(frames), int(frames.dtype == torch.uint8), S, T, Hs, Ws, _hip.fast_ptr(t_dev),
                        self.MUL, self.ADD, _hip.fast_ptr(x), _hip.fast_ptr(lb))
        return self._net(x), lb

    @staticmethod
    def to_frame_pixels(box: Tensor, lb: Tensor) -> Tensor:
        """box [B, 4] in [-1, 1], lb [B, 3] = (s, ox, oy) -> frame pixels, every float32 step rounded on its own."""
        half = box.new_tensor([144.0, 112.0, 144.0, 112.0])
        return ((box + 1.0) * half - lb[:, [1, 2, 1, 2]]) / lb[:, :1]

    @torch.no_grad()
    def localize(self, frames) -> Batch:
        frames = torch.as_tensor(frames)
        if frames.dim() != 3 or frames.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"Localizer.localize: frames are uint8 or float32 [B, H, W], got {frames.dtype} {tuple(frames.shape)}")
        _hip.lib().clear_stale_error("the start of a localizer batch")
        out, lb = self.run(frames.to(self._device).contiguous()[:, None])
        data = {"logit": out[:, 0], "hasface": torch.sigmoid(out[:, 0]), "roi": self.to_frame_pixels(out[:, 1:], lb),
                "roi_normalized": out[:, 1:], "letterbox": lb}
        return Batch(Metadata((int(frames.shape[2]), int(frames.shape[1])), int(frames.shape[0]), categories={"roi": FieldCategory.roi}), data)


# ---------------------------------------------------------------------------------------------
# closed-loop tracking (reference: scripts/evaluate_stability.py:229-264)
# ---------------------------------------------------------------------------------------------
TRACK_MAX_LANES = 16  # kTrackMaxLanes of csrc/track.hip


def track_box_is_valid(roi, factor: float, width: int, height: int) -> bool:
    """The validity rule of ttk_track_update (include/ttk.h) in float32: finite, and after the reference's clamp to the image w > 0, h > 0
    and max(w, h) * factor >= 2."""
    r = np.asarray(roi, dtype=np.float32)
    if not np.all(np.isfinite(r)):
        return False
    x0, y0 = np.maximum(np.float32(0), r[0]), np.maximum(np.float32(0), r[1])
    x1, y1 = np.minimum(r[2], np.float32(width)), np.minimum(r[3], np.float32(height))
    w, h = np.float32(x1 - x0), np.float32(y1 - y0)
    return bool(w > 0 and h > 0 and np.float32(np.maximum(w, h) * np.float32(factor)) >= 2)


class ClosedLoopTracker:
    """A network run over a video in closed loop (reference scripts/evaluate_stability.py:248-264): every frame is cropped around the box
    the network predicted on the previous frame, clamped to the image.  The loop-carried state - the current box of every lane and the
    frame counter - lives on the device: a frame is ttk_track_crop -> `net(crop)` in eval mode -> ttk_track_update (csrc/track.hip), no
    host read of anything until the last frame is enqueued, one synchronisation at the end.

    `track(frames, first_rois, lanes=None)`: frames uint8 or float32 [T,H,W] or [S,T,H,W] (grey levels; S equally sized videos, moved to
    the device once), first_rois [S,4] the box of frame 0 of every video, lanes a list of (sequence, factor) - independent trackers that
    share the network and advance in lockstep, 1 to 16 of them; default every sequence x every factor of the constructor, sequence-major.
    Returns a Batch, everything in image pixels as `Predictor.predict_batch` returns it: roi_in [T,L,4] (the box each frame was cropped
    with), roi [T,L,4], coord [T,L,3], pose [T,L,4], pt3d_68 [T,L,68,3] (networks with the landmark head), lost [T,L] (bool), and
    lane_seq [L] / lane_factor [L].

    The `lost` rule (a deliberate deviation: the reference has none - a box that leaves the image gives it a negative width and garbage
    from then on): the clamped predicted box becomes the next frame's box only if its four values are finite, the network's own box and
    the clamped one have a positive width and height, and max(w, h) * factor >= 2; otherwise lost[t, l] is set, the frame's predictions are still recorded, and the lane crops
    the next frame around its last good box.
    Not in closed loop: area-filtered resampling (ttk_area_crop has no fused form: `resample="area"` is refused) and the uncertainty
    outputs (`pose_scales_tril`, `coord_scales`), which are not recorded.

    `localizer` (a LocalizerNet; default None: the launches and the bits above): the face localizer runs on frame t of every sequence
    inside the same loop - ttk_localizer_input + its forward before the update, ttk_track_reacquire after it, all on one stream - and a
    lane that has been lost for `reacquire_after` frames restarts from the localizer's box, clamped to the image, if that box is valid by
    the rule above and the face probability exceeds `face_threshold`.  The localizer runs on every frame, needed or not: that keeps the
    loop free of host reads.  The Batch gains reacquired [T,L] (bool), hasface [T,S], loc_roi [T,S,4] (frame pixels, `Localizer`'s
    convention), and `first_rois` may be omitted: frame 0 of every sequence is localized once before the loop (one host read), and a
    sequence without a valid box above the threshold raises ValueError.

    graphed=True captures crop -> forward -> update once (after a warm-up frame on scratch state) and replays the graph T times; the
    device counter selects the frame.  A single-stream, linear graph; bitwise the eager trajectory."""

    def __init__(self, net: torch.nn.Module, factors=(1.0, 1.2), device: str | torch.device = "cuda", graphed: bool = False,
                 resample: str = "bilinear", localizer: torch.nn.Module | None = None, reacquire_after: int = 3, face_threshold: float = 0.5):
        if resample != "bilinear":
            raise ValueError(f"ClosedLoopTracker: resample={resample!r} is not available in closed loop - the fused crop (ttk_track_crop) "
                             "samples bilinearly; ttk_area_crop takes a host-side image base pointer and has no fused form")
        self._net = net.to(device).eval()
        self._device = torch.device(device)
        self._factors = tuple(float(f) for f in factors)
        self._graphed = bool(graphed)
        self._mul, self._add = 1.0 / 256.0, -0.5  # whitening of GpuFocusRoiAugment, as Predictor crops
        if int(reacquire_after) < 1:
            raise ValueError(f"ClosedLoopTracker: reacquire_after counts lost frames, at least 1, got {reacquire_after}")
        self._localizer = None if localizer is None else Localizer(localizer, device, face_threshold)
        self._reacquire_after, self._face_threshold = int(reacquire_after), float(face_threshold)

    @property
    def input_resolution(self) -> int:
        return self._net.input_resolution

    def _frame(self, st: dict) -> None:
        """Enqueues one frame: crop, forward, update.  No host read."""
        L, N = st["L"], st["N"]
        P, call = _hip.fast_ptr, _hip.lib().call
        S, T, Hs, Ws = st["frames"].shape
        call("ttk_track_crop", P(st["frames"]), st["u8"], S, T, Hs, Ws, P(st["lane_seq"]), P(st["lane_factor"]), P(st["roi_state"]), P(st["t"]),
             L, N, self._mul, self._add, P(st["view"]), P(st["tr"]), P(st["crop"]))
        preds = self._net(st["crop"])
        if "roi" not in preds:
            raise ValueError(f"ClosedLoopTracker: the network {type(self._net).__name__} has no box head output ('roi'): closed-loop "
                             f"tracking crops every frame around the predicted box (outputs: {sorted(preds)})")
        # named: the buffers must outlive the enqueue of the kernel that reads them
        st["keep"] = outs = [preds[k].to(torch.float32).contiguous() for k in ("roi", "coord", "pose")]
        pts = preds["pt3d_68"].to(torch.float32).contiguous() if st["traj_pts"] is not None else None
        outs.append(pts)
        if self._localizer is not None:  # on frame t of every sequence, before the update advances the counter; the same stream
            loc_out, lb = self._localizer.run(st["frames"], st["t"])
            outs += [loc_out, lb]
        call("ttk_track_update", P(outs[0]), P(outs[1]), P(outs[2]), P(pts), P(st["tr"]), P(st["t"]), L, N, T, Hs, Ws, P(st["lane_factor"]),
             P(st["roi_state"]), P(st["roi_in"]), P(st["roi"]), P(st["coord"]), P(st["pose"]), P(st["traj_pts"]), P(st["lost"]))
        if self._localizer is not None:
            call("ttk_track_reacquire", P(loc_out), P(lb), P(st["t"]), L, S, T, Hs, Ws, P(st["lane_seq"]), P(st["lane_factor"]), P(st["lost"]),
                 self._reacquire_after, self._face_threshold, P(st["roi_state"]), P(st["lost_run"]), P(st["reacquired"]), P(st["hasface"]),
                 P(st["loc_roi"]))

    def _first_boxes(self, frames: Tensor, lanes) -> Tensor:
        """Frame 0 of every sequence through the localizer: the start boxes [S, 4] (clamped to the image) on the host - the one host
        read before the loop.  A sequence without a valid box above the threshold raises."""
        S, _, Hs, Ws = frames.shape
        out, lb = self._localizer.run(frames, None)
        roi, hasface = Localizer.to_frame_pixels(out[:, 1:], lb).cpu(), torch.sigmoid(out[:, 0]).cpu()
        first = torch.stack([roi[:, 0].clamp(min=0.0), roi[:, 1].clamp(min=0.0), roi[:, 2].clamp(max=float(Ws)), roi[:, 3].clamp(max=float(Hs))], dim=1)
        for q in range(S):
            factors = [f for s_, f in lanes if s_ == q] or [1.0]
            ok = bool(torch.isfinite(roi[q]).all()) and all(track_box_is_valid(first[q].numpy(), f, Ws, Hs) for f in factors)
            if not (ok and float(hasface[q]) > self._face_threshold):
                raise ValueError(f"ClosedLoopTracker.track: the localizer finds no face to start from in frame 0 of sequence {q} "
                                 f"(box {roi[q].tolist()}, face probability {float(hasface[q]):.3f}, threshold {self._face_threshold})")
        return first

    @torch.no_grad()
    def track(self, frames, first_rois=None, lanes=None) -> Batch:
        dev = self._device
        frames = torch.as_tensor(frames)
        if frames.dim() == 3:
            frames = frames[None]
        if frames.dim() != 4 or frames.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"ClosedLoopTracker.track: frames are uint8 or float32 [T,H,W] or [S,T,H,W], got {frames.dtype} {tuple(frames.shape)}")
        S, T, Hs, Ws = (int(v) for v in frames.shape)
        if first_rois is None and self._localizer is None:
            raise ValueError("ClosedLoopTracker.track: without a localizer the box of frame 0 of every sequence is needed (first_rois)")
        if first_rois is not None:
            first = torch.as_tensor(first_rois, dtype=torch.float32).reshape(-1, 4).cpu()
            if first.shape[0] != S:
                raise ValueError(f"ClosedLoopTracker.track: first_rois has {first.shape[0]} boxes for {S} sequences")
        if lanes is None:
            lanes = [(s, f) for s in range(S) for f in self._factors]
        lanes = [(int(s), float(f)) for s, f in lanes]
        L = len(lanes)
        if not 1 <= L <= TRACK_MAX_LANES:
            raise ValueError(f"ClosedLoopTracker.track: 1 to {TRACK_MAX_LANES} lanes (sequence x factor), got {L}")
        frames = frames.to(dev).contiguous()
        if first_rois is None:  # frame 0 of every sequence through the localizer: the one host read before the loop
            if T < 1:
                raise ValueError("ClosedLoopTracker.track: no frames")
            _hip.lib().clear_stale_error("the start of a closed-loop track")
            first = self._first_boxes(frames, [(s, f) for s, f in lanes if 0 <= s < S])
        for i, (s, f) in enumerate(lanes):
            if not 0 <= s < S:
                raise ValueError(f"ClosedLoopTracker.track: lane {i} follows sequence {s}, but there are {S}")
            if not track_box_is_valid(first[s].numpy(), f, Ws, Hs):
                raise ValueError(f"ClosedLoopTracker.track: the first box {first[s].tolist()} of sequence {s} is not a valid start for lane {i} "
                                 f"(factor {f}) on {Ws} x {Hs} frames: finite, inside the image with positive width and height, max(w, h) * factor >= 2")
        if T < 1:
            raise ValueError("ClosedLoopTracker.track: no frames")
        _hip.lib().clear_stale_error("the start of a closed-loop track")  # once per track, not once per frame
        N = self.input_resolution
        f32 = dict(dtype=torch.float32, device=dev)
        lane_seq = torch.tensor([s for s, _ in lanes], dtype=torch.int32, device=dev)
        lane_factor = torch.tensor([f for _, f in lanes], **f32)
        start = first[[s for s, _ in lanes]].to(dev).contiguous()
        with_pts = bool(getattr(self._net, "enable_point_head", False))
        st = {"L": L, "N": N, "frames": frames, "u8": int(frames.dtype == torch.uint8), "lane_seq": lane_seq,
              "lane_factor": lane_factor, "roi_state": start.clone(), "t": torch.zeros((), dtype=torch.int32, device=dev),
              "view": torch.empty((L, 4), dtype=torch.int32, device=dev), "tr": torch.empty((L, 2, 3), **f32),
              "crop": torch.empty((L, 1, N, N), **f32), "roi_in": torch.zeros((T, L, 4), **f32), "roi": torch.zeros((T, L, 4), **f32),
              "coord": torch.zeros((T, L, 3), **f32), "pose": torch.zeros((T, L, 4), **f32),
              "traj_pts": torch.zeros((T, L, 68, 3), **f32) if with_pts else None, "lost": torch.zeros((T, L), dtype=torch.uint8, device=dev)}
        if self._localizer is not None:
            st.update(lost_run=torch.zeros((L,), dtype=torch.int32, device=dev), reacquired=torch.zeros((T, L), dtype=torch.uint8, device=dev),
                      hasface=torch.zeros((T, S), **f32), loc_roi=torch.zeros((T, S, 4), **f32))
        if self._graphed:
            self._replay(st, start, T)
        else:
            for _ in range(T):
                self._frame(st)
        torch.cuda.synchronize(dev)  # the one synchronisation
        if int(st["t"].item()) != T:
            raise RuntimeError(f"ClosedLoopTracker.track: the device counter stands at {int(st['t'].item())} after {T} frames")
        out = {"roi_in": st["roi_in"], "roi": st["roi"], "coord": st["coord"], "pose": st["pose"], "lost": st["lost"].bool(),
               "lane_seq": lane_seq, "lane_factor": lane_factor}
        if with_pts:
            out["pt3d_68"] = st["traj_pts"]
        if self._localizer is not None:
            out.update(reacquired=st["reacquired"].bool(), hasface=st["hasface"], loc_roi=st["loc_roi"])
        cats = {"coord": FieldCategory.xys, "pose": FieldCategory.quat, "pt3d_68": FieldCategory.points, "roi": FieldCategory.roi,
                "roi_in": FieldCategory.roi}
        return Batch(Metadata(N, T, categories={k: c for k, c in cats.items() if k in out}), out)

    def _replay(self, st: dict, start: Tensor, T: int) -> None:
        """One warm-up frame on a side stream (its writes - row 0, the state, the counter - are undone), one capture of a frame, T replays."""
        with _hip.CAPTURE_LOCK:
            side = torch.cuda.Stream(device=self._device)
            side.wait_stream(torch.cuda.current_stream(self._device))
            with torch.cuda.stream(side):
                self._frame(st)
                st["roi_state"].copy_(start)
                st["t"].zero_()
                if self._localizer is not None:
                    st["lost_run"].zero_()
            torch.cuda.current_stream(self._device).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self._frame(st)
        # (the capture enqueued nothing: the counter is still 0; every row the warm-up wrote is written again by replay 0)
        for _ in range(T):
            graph.replay()
        st["graph"] = graph  # alive until the caller has synchronised


def blink_stability(values, blinks, margin: int = 5) -> np.ndarray:
    """The reference's blink-stability figure (scripts/evaluate_stability.py:229-245) for one run: `values` [T] or [T, C], one quantity
    over the frames of a video (hpb, xy or sz); `blinks` (a, b) frame ranges with the eyes closed.  For every blink boundary x - all
    starts, then all ends - the difference v[x - margin] - v[x + margin]; returns the RMS over the boundaries, [C] (or [1]).  A boundary
    within `margin` frames of either end of the video is an error, not a silent skip (the reference would wrap around or raise)."""
    v = np.asarray(values, dtype=np.float64)
    xs = np.asarray([a for a, _ in blinks] + [b for _, b in blinks], dtype=np.int64)
    if xs.size == 0:
        raise ValueError("blink_stability: no blinks given")
    bad = xs[(xs - margin < 0) | (xs + margin >= len(v))]
    if bad.size:
        raise ValueError(f"blink_stability: blink boundaries {bad.tolist()} lie within {margin} frames of the ends of a {len(v)}-frame video")
    return np.atleast_1d(np.sqrt(np.mean(np.square(v[xs - margin] - v[xs + margin]), axis=0)))


class EnsemblePredictor(Predictor):
    """Several networks on ONE crop, averaged on the device (reference: scripts/add_pose_pseudolabels.py:54-127, which runs a `Predictor`
    per checkpoint - cropping every batch once per network - and averages on the host).  `predict_batch(images, rois)` takes what
    `Predictor.predict_batch` takes, crops once, runs every network in eval mode on that crop into slot e of preallocated [E, B, ...]
    buffers and reduces them with one launch of ttk_ensemble_reduce (csrc/ensemble.hip): every member is mapped to image coordinates as
    `to_image_coordinates` maps it, then rotations are averaged with the reference's `quat_average` (neuralnets/torchquaternion.py:239-256)
    and coord / pt3d_68 / shapeparam with the arithmetic mean.  Returns a Batch with pose [B,4], coord [B,3], pt3d_68 [B,68,3] and shapeparam
    [B,S] (the last two only when EVERY network has the landmark head), and the agreement of the members: rot_spread [B] (mean geodesic
    angle to the average, radians), mean_quat_norm [B] (length of the sign-aligned mean before normalisation; the reference warns where it
    is <= 0.5), coord_spread [B,3] (population standard deviation of x, y, size in pixels).

    Deliberate deviation from the reference script: it averages `unnormalized_quat`, which its Predictor does not transform back to image
    coordinates (the script's own FIXME) and which networks built with --enable-6drot do not have.  Here the networks' `pose` (unit
    quaternions) is averaged AFTER the back-transformation, so the average is a rotation in the image frame for every head type."""

    def __init__(self, nets, focus_roi_expansion_factor: float = 1.2, device: str | torch.device = "cuda", resample: str = "bilinear"):
        nets = list(nets)
        if not 1 <= len(nets) <= 16:
            raise ValueError(f"an ensemble has 1 to 16 networks, got {len(nets)}")
        if len({n.input_resolution for n in nets}) != 1:
            raise ValueError(f"the networks of an ensemble share one crop: input resolutions {[n.input_resolution for n in nets]} differ")
        super().__init__(nets[0], focus_roi_expansion_factor, device, resample)
        self._nets = [n.to(device).eval() for n in nets]
        self._with_points = all(getattr(n, "enable_point_head", False) for n in self._nets)
        self._buffers: dict = {}

    def _slots(self, B: int, S: int) -> dict:
        """[E, B, ...] input slots and the outputs of the reduction for one batch size (allocated once)."""
        key = (B, S)
        if key not in self._buffers:
            E, f = len(self._nets), dict(dtype=torch.float32, device=self._device)
            b = {"pose": torch.empty((E, B, 4), **f), "coord": torch.empty((E, B, 3), **f)}
            if self._with_points:
                b["pt3d_68"], b["shapeparam"] = torch.empty((E, B, 68, 3), **f), torch.empty((E, B, S), **f)
            self._buffers[key] = b
        return self._buffers[key]

    @torch.no_grad()
    def predict_batch(self, images, rois: Tensor) -> Batch:
        _hip.lib().clear_stale_error("the start of an ensemble batch")
        crop = self.crop_batch(images, rois)
        x, B, N = crop["image"], int(rois.shape[0]), self.input_resolution
        slots = None
        for e, net in enumerate(self._nets):
            preds = net(x)
            if slots is None:
                slots = self._slots(B, int(preds["shapeparam"].shape[-1]) if self._with_points else 0)
            for k, buf in slots.items():
                buf[e].copy_(preds[k])
        back = (position_normalization(N, N).to(self._device) @ Affine2d(crop["image_transform"])).inv().tensor().contiguous()
        f = dict(dtype=torch.float32, device=self._device)
        out = {"pose": torch.empty((B, 4), **f), "coord": torch.empty((B, 3), **f)}
        if self._with_points:
            out["pt3d_68"], out["shapeparam"] = torch.empty((B, 68, 3), **f), torch.empty_like(slots["shapeparam"][0])
        stats = torch.empty((B, 5), **f)
        P = _hip.ptr
        _hip.lib().call("ttk_ensemble_reduce", P(slots["pose"]), P(slots["coord"]), P(slots.get("pt3d_68")), P(slots.get("shapeparam")), P(back),
                        len(self._nets), B, int(out["shapeparam"].shape[-1]) if self._with_points else 0, P(out["pose"]), P(out["coord"]),
                        P(out.get("pt3d_68")), P(out.get("shapeparam")), P(stats))
        out["rot_spread"], out["mean_quat_norm"], out["coord_spread"] = stats[:, 0], stats[:, 1], stats[:, 2:]
        cats = {"coord": FieldCategory.xys, "pose": FieldCategory.quat, "pt3d_68": FieldCategory.points}
        return Batch(Metadata(N, B, categories={k: c for k, c in cats.items() if k in out}), out)


# ---------------------------------------------------------------------------------------------
# metrics (reference :295-440)
# ---------------------------------------------------------------------------------------------
class _SimpleConcatenatingErrorMetric:
    def __init__(self):
        self.error: list[Tensor] = []

    def update(self, preds: Batch, targets: Batch) -> None:
        self.error.append(self.compute_on_batch(preds, targets))

    def compute_on_batch(self, preds: Batch, targets: Batch) -> Tensor:
        raise NotImplementedError()

    def compute(self) -> Tensor:
        return torch.cat(self.error)

    def reset(self):
        self.error = []


class LabelExtractor(_SimpleConcatenatingErrorMetric):
    def __init__(self, key):
        super().__init__()
        self._key = key

    def compute_on_batch(self, preds, targets):
        return targets[self._key]


class PredExtractor(LabelExtractor):
    def compute_on_batch(self, preds, targets):
        return preds[self._key]


class GeodesicError(_SimpleConcatenatingErrorMetric):
    def compute_on_batch(self, preds, targets):
        return torchquaternion.geodesicdistance(targets["pose"], preds["pose"])


def _angle_errors(euler1, euler2):
    v1 = np.stack([np.cos(euler1), np.sin(euler1)], axis=-1)
    v2 = np.stack([np.cos(euler2), np.sin(euler2)], axis=-1)
    return np.arccos(np.clip(np.sum(v1 * v2, axis=-1), -1.0, 1.0))


def _quat_to_aflw3d_rotations(quats: Tensor):
    return np.array([utils.inv_aflw_rotation_conversion(q) for q in utils.convert_to_rot(quats.detach().cpu().numpy())])


def _aflw3d_euler_errors(quats1: Tensor, quats2: Tensor) -> Tensor:
    return torch.from_numpy(_angle_errors(_quat_to_aflw3d_rotations(quats1), _quat_to_aflw3d_rotations(quats2))).to(quats1.device)


class EulerAngleErrors(_SimpleConcatenatingErrorMetric):
    """|pitch|, |yaw|, |roll| differences in the AFLW2000-3D convention, radians, [B,3]."""

    def compute_on_batch(self, preds, targets):
        return _aflw3d_euler_errors(preds["pose"], targets["pose"])


class NormalizedXYSError(_SimpleConcatenatingErrorMetric):
    def compute_on_batch(self, preds, targets):
        x0, y0, x1, y1 = targets["roi"].unbind(-1)
        return torch.abs(preds["coord"] - targets["coord"]) / (x1 - x0)[:, None]


def _eval_keypoints(pred: Tensor, gt: Tensor, dims=3):
    assert pred.shape == gt.shape and pred.shape[-1] == 3
    pred, gt = pred.clone(), gt.clone()
    pred[:, :, 2] -= torch.mean(pred[:, :, 2], dim=-1, keepdim=True)
    gt[:, :, 2] -= torch.mean(gt[:, :, 2], dim=-1, keepdim=True)
    dist = torch.mean(torch.norm(pred[:, :, :dims] - gt[:, :, :dims], dim=-1), dim=-1)
    bbox = torch.sqrt((gt[:, :, 0].amax(1) - gt[:, :, 0].amin(1)) * (gt[:, :, 1].amax(1) - gt[:, :, 1].amin(1)))
    return dist / bbox


class UnweightedKptNME(_SimpleConcatenatingErrorMetric):
    def __init__(self, dimensions=3):
        super().__init__()
        self.dims = dimensions

    def compute_on_batch(self, preds, targets):
        return _eval_keypoints(preds["pt3d_68"], targets["pt3d_68"], self.dims)


class KptNmeResults(NamedTuple):
    bin_30_nme: float
    bin_60_nme: float
    bin_90_nme: float
    avg_nme: float


class KptNME:
    """Landmark NME binned by |yaw| of the label: 0-30, 30-60, 60-90 degrees (reference :407-440)."""

    def __init__(self, dimensions=3):
        self.dims, self.error, self.masks = dimensions, [], []

    def update(self, preds, targets):
        pyr = _quat_to_aflw3d_rotations(targets["pose"])
        yaw = np.abs(pyr[:, 1]) * 180.0 / np.pi
        self.masks.append(torch.from_numpy(np.stack([(a <= yaw) & (yaw < b) for a, b in ((0.0, 30.0), (30.0, 60.0), (60.0, 90.0))], -1)))
        self.error.append(_eval_keypoints(preds["pt3d_68"], targets["pt3d_68"], self.dims).cpu())

    def compute(self) -> KptNmeResults:
        errors, masks = torch.cat(self.error), torch.cat(self.masks).unbind(-1)
        bins = [torch.mean(errors[m]).item() for m in masks]
        return KptNmeResults(*bins, float(np.average(bins)))


def pose_error_table(euler_errors: Tensor, geodesic: Tensor) -> dict:
    """The summary row scripts/evaluate_pose_network.py prints: MAE per angle and their mean in degrees (reference
    scripts/evaluate_pose_network.py:205-291)."""
    e = euler_errors.detach().cpu().numpy() * utils.rad2deg
    mae = e.mean(0)
    return {"pitch": float(mae[0]), "yaw": float(mae[1]), "roll": float(mae[2]), "mae": float(mae.mean()),
            "geodesic": float(geodesic.detach().cpu().numpy().mean() * utils.rad2deg)}


# ---------------------------------------------------------------------------------------------
# rotation errors after an alignment of the predictions (reference :443-600; scripts/evaluate_pose_network.py --alignment-scheme)
# ---------------------------------------------------------------------------------------------
def compute_mean_rotation(rots, tol=0.0001, max_iter=100000):
    """Karcher mean of scipy Rotations inside the ball of radius pi/2 (the OPAL paper's evaluator, reference :447-459): start at the first
    one, move along the mean tangent vector until it is shorter than `tol`."""
    from scipy.spatial.transform import Rotation

    rots = rots[rots.magnitude() < np.pi / 2]
    mean = rots[0]
    for _ in range(max_iter):
        step = np.mean((mean.inv() * rots).as_rotvec(), axis=0)
        if np.linalg.norm(step) < tol:
            break
        mean = mean * Rotation.from_rotvec(step)
    return mean


def compute_opal_paper_alignment(pose_pred: Tensor, pose_target: Tensor, cluster_ids) -> Tensor:
    """Predictions with the mean offset to the labels removed, separately for every cluster id (the recorded individuals of Biwi):
    P <- P * mean(T^-1 P)^-1 (reference :462-482).  CPU tensors."""
    from scipy.spatial.transform import Rotation

    assert pose_pred.device.type == "cpu" and pose_target.device.type == "cpu"
    cluster_ids = np.asarray(cluster_ids)
    out = torch.empty_like(pose_pred)
    for cid in np.unique(cluster_ids):
        mask = cluster_ids == cid
        pred, target = Rotation.from_quat(pose_pred[mask].numpy()), Rotation.from_quat(pose_target[mask].numpy())
        offset = compute_mean_rotation(target.inv() * pred)
        out[torch.from_numpy(mask)] = torch.from_numpy((pred * offset.inv()).as_quat()).to(pose_pred.dtype)
    return out


class PerspectiveCorrector:
    """The network sees a face off the optical axis under the angle of its viewing ray; this rotates the predicted pose from the ray's frame
    into the camera frame (reference :485-544).  `fov`: horizontal field of view in degrees."""

    def __init__(self, fov):
        self._fov = fov
        self.f = 1.0 / np.tan(fov * np.pi / 180.0 * 0.5)

    def corrected_rotation(self, image_sizes: Tensor, coord: Tensor, pose: Tensor) -> Tensor:
        """image_sizes [B, 2] = (width, height); coord [B, 3] in pixels; pose [B, 4]."""
        half = 0.5 * image_sizes
        xy = (coord[..., :2] - half) / half[0]  # (the reference divides by the FIRST row's half size: all images of a set share one size)
        ray = torch.cat([xy, torch.as_tensor(self.f, device=xy.device, dtype=xy.dtype).expand_as(xy[..., :1])], dim=-1)
        return torchquaternion.mult(torchquaternion.from_matrix(self._make_look_at_matrix(ray)), pose)

    @staticmethod
    def _make_look_at_matrix(pos: Tensor) -> Tensor:
        """Columns x, y, z with z along `pos` and x kept horizontal."""
        z = pos / torch.norm(pos, dim=-1, keepdim=True)
        x = torch.cross(*torch.broadcast_tensors(pos.new_tensor([0.0, 1.0, 0.0]), z), dim=-1)
        x = x / torch.norm(x, dim=-1, keepdim=True)
        y = torch.cross(z, x, dim=-1)
        y = y / torch.norm(x, dim=-1, keepdim=True)  # (x is already unit length: the reference's normalisation of y is a no-op)
        return torch.stack([x, y, z], dim=-1)


class AlignedRotationErrorMetric:
    """Euler-angle or geodesic errors after `correction_mode` "perspective" (needs the image sizes: targets["image_hw"] [B, 2] as
    Predictor.evaluate provides it, or targets["image"] as a list of [H, W(, C)] frames) or "opal23" (needs targets["individual"]) -
    reference :547-600."""

    def __init__(self, error_mode, correction_mode, fov=None):
        assert error_mode in ("euler", "geo") and correction_mode in ("perspective", "opal23")
        self._error_mode, self._correction_mode, self._fov = error_mode, correction_mode, fov
        self.reset()

    def reset(self):
        self.image_sizes, self.target_quats, self.pred_quats, self.pred_coord, self.individual = [], [], [], [], []

    def update(self, preds: Batch, targets: Batch) -> None:
        self.target_quats.append(targets["pose"].cpu())
        self.pred_quats.append(preds["pose"].cpu())
        self.pred_coord.append(preds["coord"].cpu())
        if self._correction_mode == "perspective":
            hw = targets["image_hw"] if "image_hw" in targets else torch.as_tensor([tuple(t.shape[:2]) for t in targets["image"]])
            self.image_sizes.append(torch.as_tensor(hw).cpu())  # (h, w)
        else:
            self.individual.append(torch.as_tensor(targets["individual"]).cpu())

    def compute(self) -> Tensor:
        target, pred, coord = torch.cat(self.target_quats), torch.cat(self.pred_quats), torch.cat(self.pred_coord)
        if self._correction_mode == "perspective":
            wh = torch.flip(torch.cat(self.image_sizes), dims=(-1,))
            pred = PerspectiveCorrector(self._fov).corrected_rotation(wh, coord, pred)
        else:
            pred = compute_opal_paper_alignment(pred, target, torch.cat(self.individual).numpy())
        if self._error_mode == "euler":
            return _aflw3d_euler_errors(pred, target)
        return torchquaternion.geodesicdistance(pred, target)
