"""numpy restatement of the closed-loop tracker's frame step (csrc/track.hip): the integer view box and the crop transform of ttk_track_crop,
and the update of ttk_track_update - `back` = (norm(N) o tr)^-1 in closed form from a float32 `tr`, the labels under it (the formulas of
tests/ensemble_ref.py: datatransformation/tensors/affinetrafo.py transform_coord / transform_keypoints / transform_rot, + transform_roi), the
reference's clamp (scripts/evaluate_stability.py:257-259), the validity rule and the flow of state and counter over several frames.
float64 by default.  Held to `Predictor.to_image_coordinates`, to the reference's four-line clamp and - `blink_stability_direct` - to the
reference's blink report by tests/test_track_ref.py."""
import numpy as np

import ensemble_ref as ER

F32 = np.float32


def view_roi_f32(roi, factor):
    """ttk_view_roi with translation (0, 0) in float32, operation by operation (every one a correctly rounded IEEE operation on both sides):
    the int32 box [L,4], and the values before the rounding to integers in float64 (for the tie margins the chain test asserts)."""
    r, f = np.asarray(roi, F32), np.asarray(factor, F32)
    x0, y0, x1, y1 = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    bw, bh = x1 - x0, y1 - y0
    cx, cy = F32(0.5) * (x1 + x0), F32(0.5) * (y1 + y0)
    hs = (np.maximum(bw, bh) * f) * F32(0.5)
    pre = np.stack([(cx - hs) + F32(0), (cy - hs) + F32(0), (cx + hs) + F32(0), (cy + hs) + F32(0)], -1)
    assert pre.dtype == F32
    return np.rint(pre).astype(np.int32), pre.astype(np.float64)


def roi_transform(view, N, dtype=np.float64):
    """ttk_roi_transform without a rotation: tr [L,2,3] maps the integer view box onto [0, N]^2.  In float32 this is bitwise the kernel's
    result (one division and one product per entry; the rotation part multiplies by 1 and adds zeros)."""
    v = np.asarray(view).astype(dtype)
    sx, sy = dtype(N) / (v[:, 2] - v[:, 0]), dtype(N) / (v[:, 3] - v[:, 1])
    z = np.zeros_like(sx)
    return np.stack([np.stack([sx, z, -v[:, 0] * sx], -1), np.stack([z, sy, -v[:, 1] * sy], -1)], 1).astype(dtype)


def back_from_tr(tr, N, dtype=np.float64):
    """(norm(N) o tr)^-1, norm(N): x -> x 2 / N - 1; tr [L,2,3] image pixels -> crop pixels."""
    m = np.asarray(tr).astype(dtype)
    s = dtype(2.0) / dtype(N)
    a, b, tx, c, d, ty = s * m[:, 0, 0], s * m[:, 0, 1], s * m[:, 0, 2] - 1, s * m[:, 1, 0], s * m[:, 1, 1], s * m[:, 1, 2] - 1
    det = a * d - b * c
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    return np.stack([np.stack([ia, ib, -(ia * tx + ib * ty)], -1), np.stack([ic, id_, -(ic * tx + id_ * ty)], -1)], 1).astype(dtype)


def roi_under(back, roi, dtype=np.float64):
    """transform_roi (affinetrafo.py:91-104): the bounding box of the four transformed corners."""
    m, r = np.asarray(back).astype(dtype), np.asarray(roi).astype(dtype)
    xs, ys = r[:, [0, 2, 0, 2]], r[:, [1, 1, 3, 3]]
    px = m[:, 0, 0, None] * xs + m[:, 0, 1, None] * ys + m[:, 0, 2, None]
    py = m[:, 1, 0, None] * xs + m[:, 1, 1, None] * ys + m[:, 1, 2, None]
    with np.errstate(invalid="ignore"):
        return np.stack([np.fmin.reduce(px, -1), np.fmin.reduce(py, -1), np.fmax.reduce(px, -1), np.fmax.reduce(py, -1)], -1)


def clamp(roi, Ws, Hs):
    """(max(0, x0), max(0, y0), min(x1, Ws), min(y1, Hs)); NaN-ignoring like fmaxf / fminf (non-finite boxes are invalid before it matters)."""
    r = np.asarray(roi)
    z = r.dtype.type(0)
    return np.stack([np.fmax(z, r[:, 0]), np.fmax(z, r[:, 1]), np.fmin(r[:, 2], r.dtype.type(Ws)), np.fmin(r[:, 3], r.dtype.type(Hs))], -1)


def valid(roi_t, cand, factor, roi_pred=None):
    """The validity rule: the back-transformed box finite (before the clamp), the candidate with w > 0, h > 0 and max(w, h) factor >= 2,
    and - the back-transformed box being a bounding box of corners, which re-sorts an inverted prediction - the network's own box ordered."""
    w, h = cand[:, 2] - cand[:, 0], cand[:, 3] - cand[:, 1]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(roi_t).all(-1) & (w > 0) & (h > 0) & (np.maximum(w, h) * np.asarray(factor).astype(cand.dtype) >= 2)
        if roi_pred is not None:
            p = np.asarray(roi_pred)
            ok &= (p[:, 2] > p[:, 0]) & (p[:, 3] > p[:, 1])
    return ok


def update(roi, coord, pose, pts, tr, N, Ws, Hs, factor, roi_state, dtype=np.float64):
    """One ttk_track_update: the outputs of row t, the candidate, `lost` and the next state."""
    back = back_from_tr(tr, N, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        pose_t, coord_t, pts_t = ER.back_transform(back, np.asarray(pose)[None], np.asarray(coord)[None], None if pts is None else np.asarray(pts)[None], dtype)
        roi_t = roi_under(back, roi, dtype)
    cand = clamp(roi_t, Ws, Hs)
    ok = valid(roi_t, cand, factor, roi)
    state = np.where(ok[:, None], cand, np.asarray(roi_state).astype(dtype))
    return {"back": back, "roi": roi_t, "coord": coord_t[0], "pose": pose_t[0], "pts": None if pts_t is None else pts_t[0], "cand": cand, "lost": ~ok,
            "state": state}


def track(first, factor, preds, N, Ws, Hs, dtype=np.float64):
    """The loop over frames with a fixed table of "predictions" preds[t] = (roi, coord, pose, pts or None) in the crop's coordinates:
    crop geometry from the state (stored as float32, as the device stores it), update, next frame.  Returns per-frame lists."""
    state, t, out = np.asarray(first).astype(dtype), 0, []
    for roi, coord, pose, pts in preds:
        state32 = state.astype(F32)
        view, pre = view_roi_f32(state32, factor)
        tr32 = roi_transform(view, N, F32)
        u = update(roi, coord, pose, pts, tr32, N, Ws, Hs, factor, state, dtype)
        u.update(roi_in=state, view=view, view_pre=pre, tr=tr32, t=t)
        out.append(u)
        state, t = u["state"], t + 1
    return out, t


def blink_stability_direct(values, blinks):
    """scripts/evaluate_stability.py:229-237 for one run and one quantity, as the reference writes it."""
    xs = np.asarray([a for a, b in blinks] + [b for a, b in blinks], dtype=np.int64)
    lefts, rights = xs - 5, xs + 5
    vals = np.asarray(values)
    return np.atleast_1d(np.sqrt(np.mean(np.square(vals[lefts] - vals[rights]), axis=0)))
