"""Converted pose-dataset shards -> frames resident in HBM.

The reference reads its training sets from HDF5 files through h5py in DataLoader worker processes and decodes one JPEG per sample
with OpenCV (datasets/dshdf5.py:59-336, dshdf5pose.py:198-256; file list pipelines.py:120-300).  This image has neither h5py nor
OpenCV in its default interpreter, and the MI355X path wants the frames on the GPU anyway (datasets/resident.py), so the job is
split:

  oracle/tools/h5_to_npz.py   (build container, /opt/conda python with h5py) one .h5 -> one .npz shard: the JPEG blobs untouched
                              (`image_bytes` + `image_lengths`, or raw `images`) and the label arrays under their HDF5 names
  decode_pose_shard()         here: PIL decodes every blob to grey uint8 ONCE, frames are zero-padded to a common size (labels
                              are pixel coordinates: padding right / bottom does not move them), names are mapped as the reference
                              maps them (dshdf5pose.py:34-46: rois -> roi, coords -> coord, quats -> pose, shapeparams -> shapeparam),
                              and the half-pixel offset of cell-centred pixels (batch/normalization.py:83-90: + 0.5 on the xy of
                              `coord` and `pt3d_68`) is applied
  load_resident_frames()      the decoded shard as a ResidentFrames on the device, with its task Tag
"""
from __future__ import annotations

import io

import numpy as np
import torch

from .resident import ResidentFrames

# dshdf5pose.py:33-46 (its whitelist :168-180 also names semseg / seg_image, which no pose dataset of the training script carries)
_NAME_MAP = {"rois": "roi", "coords": "coord", "quats": "pose", "pt3d_68": "pt3d_68", "pt2d_68": "pt2d_68", "shapeparams": "shapeparam", "hasface": "hasface"}


def _to_grey(im: np.ndarray) -> np.ndarray:
    """Raw frames with a colour axis -> grey with the luma weights the JPEG path uses (PIL "L" = ITU-R 601: 299/587/114 per mille,
    what cv2.imdecode(..., IMREAD_GRAYSCALE) of the reference computes too), rounded to nearest."""
    if im.ndim == 2:
        return np.asarray(im, dtype=np.uint8)
    rgb = np.asarray(im[..., :3], dtype=np.float32)
    return np.clip(np.rint(rgb @ np.array([0.299, 0.587, 0.114], np.float32)), 0, 255).astype(np.uint8)


def _decode_grey(blob: bytes) -> np.ndarray:
    from PIL import Image  # (Pillow is in the image; OpenCV is not)

    return np.asarray(Image.open(io.BytesIO(blob)).convert("L"), dtype=np.uint8)


def _decode_labels(d, half_pixel_offset: bool) -> dict:
    """The label arrays of an opened shard under their Batch names, with the half-pixel offset: decode_pose_shard without the images."""
    out = {}
    for src, dst in _NAME_MAP.items():
        if src in d.files:
            v = np.asarray(d[src])
            out[dst] = v.astype(np.float32) if v.dtype.kind == "f" else v
    # who is in a frame (reference dshdf5pose.py:221-236): from the sequence boundaries, else the stored array
    if "sequence_starts" in d.files:
        starts = np.asarray(d["sequence_starts"]).astype(np.int32)
        out["individual"] = np.concatenate([np.full(b - a, i, dtype=np.int32) for i, (a, b) in enumerate(zip(starts[:-1], starts[1:]))])
    elif "individual" in d.files:
        out["individual"] = np.asarray(d["individual"]).astype(np.int32)
    if half_pixel_offset:
        if "coord" in out:
            out["coord"] = out["coord"].copy()
            out["coord"][:, :2] += 0.5
        for k in ("pt3d_68", "pt2d_68"):
            if k in out:
                out[k] = out[k].copy()
                out[k][..., :2] += 0.5
    return out


def decode_pose_shard(path: str, half_pixel_offset: bool = True) -> dict:
    """{"image": uint8 [N,1,H,W] (zero-padded to the largest frame), "image_size": int32 [N,2] (w, h), labels...}"""
    d = np.load(path)
    if "image_bytes" in d.files:
        lengths = d["image_lengths"].astype(np.int64)
        offs = np.concatenate([[0], np.cumsum(lengths)])
        blob = d["image_bytes"]
        frames = [_decode_grey(blob[offs[i]:offs[i + 1]].tobytes()) for i in range(len(lengths))]
    elif "images" in d.files:
        imgs = d["images"]
        frames = [_to_grey(im) for im in imgs]
    else:
        raise ValueError(f"{path}: neither image_bytes/image_lengths nor images")
    H, W = max(f.shape[0] for f in frames), max(f.shape[1] for f in frames)
    image = np.zeros((len(frames), 1, H, W), np.uint8)
    for i, f in enumerate(frames):
        image[i, 0, :f.shape[0], :f.shape[1]] = f
    out = {"image": image, "image_size": np.array([[f.shape[1], f.shape[0]] for f in frames], np.int32)}
    out.update(_decode_labels(d, half_pixel_offset))
    n = {len(v) for v in out.values()}
    if len(n) != 1:
        raise ValueError(f"{path}: fields of different lengths")
    return out


def read_labels(path: str, half_pixel_offset: bool = True) -> dict:
    """The labels of a shard as decode_pose_shard returns them (names mapped, float32, `individual`, half-pixel offset) without decoding
    one image: what a tool that only re-labels a shard needs (scripts/fit_face_model.py)."""
    with np.load(path) as d:
        if "image_lengths" not in d.files and "images" not in d.files:
            raise ValueError(f"{path}: neither image_bytes/image_lengths nor images")
        out = _decode_labels(d, half_pixel_offset)
    n = {len(v) for v in out.values()}
    if len(n) > 1:
        raise ValueError(f"{path}: fields of different lengths")
    return out


def load_resident_frames(path: str, tag, device="cuda", coord_convention_id: int = 0, half_pixel_offset: bool = True) -> ResidentFrames:
    shard = decode_pose_shard(path, half_pixel_offset)
    fields = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in shard.items() if k != "image_size"}
    fields["coord_convention_id"] = torch.full((len(shard["image"]),), int(coord_convention_id), dtype=torch.int32, device=device)
    return ResidentFrames(tag, fields)


# ---------------------------------------------------------------------------------------------
# pseudo-labels (reference: scripts/add_pose_pseudolabels.py:131-156 writes them into the HDF5 file in place; a shard is rewritten)
# ---------------------------------------------------------------------------------------------
_LABEL_ARRAYS = {"pose": "quats", "coord": "coords", "pt3d_68": "pt3d_68", "shapeparam": "shapeparams"}  # Batch name -> HDF5 name
_STAT_ARRAYS = {"rot_spread": "pseudolabel_rot_spread", "mean_quat_norm": "pseudolabel_mean_quat_norm", "coord_spread": "pseudolabel_coord_spread"}
_FIT_ARRAYS = {"objective": "facefit_objective", "status": "facefit_status", "iterations": "facefit_iterations"}  # face-model fit


def write_pseudolabels(src: str, dst: str, labels: dict, keep=None, overwrite: bool = False) -> str:
    """The shard `src` with the labels of an ensemble (eval.EnsemblePredictor) written to `dst` (may be `src`).

    `labels`: Batch names -> arrays / tensors over ALL frames of `src`: "pose" [N,4] and "coord" [N,3] (image pixels, cell-centred as the
    predictor returns them), optionally "pt3d_68" [N,68,3], "shapeparam" [N,S] and the statistics "rot_spread" [N], "mean_quat_norm" [N],
    "coord_spread" [N,3].  They are stored under their HDF5 names (quats, coords, pt3d_68, shapeparams; the statistics as pseudolabel_*,
    which decode_pose_shard does not read) with the half-pixel offset undone (- 0.5 on the xy of coord and pt3d_68), so that
    decode_pose_shard(dst) returns what was passed in.  Every other array of the shard is copied untouched, image blobs byte for byte.
    `keep`: boolean frame mask; dropped frames leave every per-frame array (the reference's filter_dataset.filter_file_by_frames) - like
    it, a shard with `sequence_starts` is refused when frames are dropped.  Label arrays the shard already has, and an existing `dst`,
    are replaced only with overwrite=True.  The write goes to a temporary file next to `dst`, then os.replace: no partial shard."""
    return _rewrite_labels(src, dst, labels, _STAT_ARRAYS, ("pose", "coord"), ".pseudolabels-", keep, overwrite)


def write_face_fit(src: str, dst: str, labels: dict, keep=None, overwrite: bool = False) -> str:
    """The shard `src` with the labels of a face-model fit (facemodel.fitting.FaceModelFitter.fit) written to `dst`: write_pseudolabels'
    machinery - the same half-pixel rule, `keep`, temporary file + os.replace and refusals - for "pose" [N,4], "coord" [N,3], "pt3d_68"
    [N,68,3] and "shapeparam" [N,50] (all four required: they are what the fit is run for), stored as quats, coords, pt3d_68, shapeparams,
    and optionally "objective" [N], "status" [N], "iterations" [N,2], stored as facefit_objective (float32), facefit_status and
    facefit_iterations (int32), which decode_pose_shard does not read."""
    return _rewrite_labels(src, dst, labels, _FIT_ARRAYS, ("pose", "coord", "pt3d_68", "shapeparam"), ".facefit-", keep, overwrite)


def _rewrite_labels(src, dst, labels, extra_arrays, required, tmp_prefix, keep, overwrite) -> str:
    import os
    import tempfile

    def host(v):
        return np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v)

    unknown = set(labels) - set(_LABEL_ARRAYS) - set(extra_arrays)
    if unknown or any(k not in labels for k in required):
        need = " and ".join(repr(k) for k in required) if len(required) == 2 else ", ".join(repr(k) for k in required)
        raise ValueError(f"labels need {need} and may hold {sorted(set(_LABEL_ARRAYS) | set(extra_arrays))}; got {sorted(labels)}")
    with np.load(src) as d:
        arrays = {k: d[k] for k in d.files}
    if "image_lengths" in arrays:
        n = len(arrays["image_lengths"])
    elif "images" in arrays:
        n = len(arrays["images"])
    else:
        raise ValueError(f"{src}: neither image_bytes/image_lengths nor images")
    new = {}
    for k, v in labels.items():
        v = host(v)
        v = v.astype(np.int32) if k in ("status", "iterations") else v.astype(np.float32)
        if len(v) != n:
            raise ValueError(f"labels[{k!r}] has {len(v)} rows, {src} has {n} frames")
        if k in ("coord", "pt3d_68"):
            v = v.copy()
            v[..., :2] -= np.float32(0.5)
        new[_LABEL_ARRAYS.get(k) or extra_arrays[k]] = v
    present = sorted(set(new) & set(arrays))
    if not overwrite and (present or os.path.exists(dst)):
        raise FileExistsError((f"{dst} exists" if os.path.exists(dst) else f"{src} already has {present}") + ": pass overwrite=True to replace")
    if keep is not None:
        keep = host(keep).astype(bool)
        if keep.shape != (n,):
            raise ValueError(f"keep has shape {keep.shape}, {src} has {n} frames")
        if not keep.all() and "sequence_starts" in arrays:
            raise ValueError(f"{src} has sequence_starts: frames of a sequence dataset cannot be dropped")
    arrays.update(new)
    if keep is not None and not keep.all():
        if "image_bytes" in arrays:
            lengths = arrays["image_lengths"].astype(np.int64)
            offs = np.concatenate([[0], np.cumsum(lengths)])
            blob = arrays.pop("image_bytes")
            pieces = [blob[offs[i]:offs[i + 1]] for i in np.flatnonzero(keep)]
            kept_blob = np.concatenate(pieces) if pieces else blob[:0]
        arrays = {k: (v[keep] if v.ndim >= 1 and len(v) == n else v) for k, v in arrays.items()}
        if "image_lengths" in arrays:
            arrays["image_bytes"] = kept_blob
    fd, tmp = tempfile.mkstemp(dir=os.path.dirname(os.path.abspath(dst)), prefix=tmp_prefix, suffix=".npz")
    try:
        with os.fdopen(fd, "wb") as f:
            np.savez(f, **arrays)
        os.replace(tmp, dst)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise
    return dst
