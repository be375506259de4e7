"""numpy restatement of ttk_ensemble_reduce (csrc/ensemble.hip): every member of an ensemble mapped from the crop's [-1, 1] coordinates to
image pixels (datatransformation/tensors/affinetrafo.py: transform_coord, transform_keypoints, transform_rot), then the reference's
quat_average (neuralnets/torchquaternion.py:239-256) for the rotations, the arithmetic mean for coord / pt3d_68 / shapeparam, and the five
statistics of the kernel.  float64 by default; `dtype=np.float32` runs the same statements in float32 (the yardstick of the statistic that
goes through atan2).  Held to the reference's own quat_average / np.average and to the repository's apply_affine2d by
tests/test_ensemble_ref.py."""
import numpy as np

TINY = np.finfo(np.float32).tiny  # FLT_MIN: the kernel divides the mean quaternion by max(|mean|, FLT_MIN)


def flip_map():
    from trackertraincode.facemodel.keypoints68 import flip_map as fm

    return np.asarray(fm, dtype=np.int64)


def qmul(u, v):
    """Hamilton product, components (i, j, k, w)."""
    ui, uj, uk, uw = np.moveaxis(u, -1, 0)
    vi, vj, vk, vw = np.moveaxis(v, -1, 0)
    return np.stack([ui * vw + uw * vi - uk * vj + uj * vk, uj * vw + uk * vi + uw * vj - ui * vk,
                     uk * vw - uj * vi + ui * vj + uw * vk, uw * vw - ui * vi - uj * vj - uk * vk], -1)


def back_transform(back, pose, coord, pts=None, dtype=np.float64):
    """back [B,2,3]; pose [E,B,4], coord [E,B,3], pts [E,B,68,3] or None -> the members in image coordinates."""
    m = np.asarray(back, dtype=dtype)
    pose, coord = np.asarray(pose, dtype=dtype), np.asarray(coord, dtype=dtype)
    a, b, tx, c, d, ty = m[:, 0, 0], m[:, 0, 1], m[:, 0, 2], m[:, 1, 0], m[:, 1, 1], m[:, 1, 2]
    det = a * d - b * c
    scale = np.sqrt(a * a + b * b + c * c + d * d) / np.sqrt(dtype(2.0))
    x, y, s = coord[..., 0], coord[..., 1], coord[..., 2]
    coord_t = np.stack([a * x + b * y + tx, c * x + d * y + ty, scale * s], -1)
    sg = np.sign(det)
    alpha = np.arctan2(-b, d)
    zero = np.zeros_like(alpha)
    zrot = np.stack([zero, zero, np.sin(alpha / 2) * sg, np.cos(alpha / 2)], -1)
    pose_t = qmul(np.broadcast_to(zrot, pose.shape), pose) * np.stack([np.ones_like(sg), sg, sg, np.ones_like(sg)], -1)
    pts_t = None
    if pts is not None:
        pts = np.asarray(pts, dtype=dtype)
        e = lambda v: v[None, :, None]
        px, py, pz = pts[..., 0], pts[..., 1], pts[..., 2]
        pts_t = np.stack([e(a) * px + e(b) * py + e(tx), e(c) * px + e(d) * py + e(ty), e(np.sqrt(np.abs(det))) * pz], -1)
        mirrored = det < 0
        if mirrored.any():
            pts_t[:, mirrored] = pts_t[:, mirrored][:, :, flip_map(), :]
    return pose_t.astype(dtype), coord_t.astype(dtype), None if pts_t is None else pts_t.astype(dtype)


def quat_average(quats):
    """[E,N,4] -> (normalised mean [N,4], |mean| [N], pivot [N], sign-aligned members [E,N,4])."""
    pivot = np.argmax(np.abs(quats).sum(0), axis=-1)
    neg = np.take_along_axis(quats, pivot[None, :, None], axis=-1)[..., 0] < 0
    aligned = np.where(neg[..., None], -quats, quats)
    mean = aligned.mean(0, dtype=quats.dtype)
    norm = np.linalg.norm(mean, axis=-1)
    return mean / np.maximum(norm, quats.dtype.type(TINY))[:, None], norm, pivot, aligned


def geodesic(q, members):
    """Angle of conj(q) * member: 2 atan2(|ijk|, |w|) (torchquaternion.geodesicdistance)."""
    d = qmul(np.broadcast_to(q * np.array([-1, -1, -1, 1], q.dtype), members.shape), members)
    return 2 * np.arctan2(np.linalg.norm(d[..., :3], axis=-1), np.abs(d[..., 3]))


def ensemble_reduce(pose, coord, pts, shape, back, dtype=np.float64):
    """The whole reduction.  Returns pose [B,4], coord [B,3], pts [B,68,3] / shape [B,S] (None where the input is), stats [B,5] and, under
    "members", the transformed members (pose, coord, pts) the averages were taken over."""
    pose_t, coord_t, pts_t = back_transform(back, pose, coord, pts, dtype)
    q, norm, pivot, _ = quat_average(pose_t)
    cm = coord_t.mean(0, dtype=dtype)
    stats = np.concatenate([geodesic(q, pose_t).mean(0, dtype=dtype)[:, None], norm[:, None],
                            np.sqrt(((coord_t - cm) ** 2).mean(0, dtype=dtype))], -1)
    return {"pose": q, "coord": cm, "pts": None if pts_t is None else pts_t.mean(0, dtype=dtype),
            "shape": None if shape is None else np.asarray(shape, dtype=dtype).mean(0, dtype=dtype), "stats": stats.astype(dtype),
            "pivot": pivot, "members": (pose_t, coord_t, pts_t)}
