"""Cases, launches and error bounds of the closed-loop tracker's kernel tests (tests/test_track_kernels_gpu.py, test_closed_loop_gpu.py):
ttk_track_crop / ttk_track_update through the C-ABI on guarded buffers, the first against the three launches it replaces (bitwise, no
tolerance), the second against tests/track_ref.py in float64 on the same float32 inputs.

Tolerances of ttk_track_update, per output and per row (u = 2^-24, first order in u; every factor counts the roundings on the path, every
magnitude is a sum of absolute operand products, evaluated in float64 from the row's own inputs).  With tr = (m0 m1 m2; m3 m4 m5), s = 2 / N:

  A = norm o tr       s carries 1 rounding, a = s m0 (b, c, d alike) one more: |da| <= 2 u |a|.
                      tx = s m2 - 1: 2 roundings on |s m2|, 1 on the difference: e_t(x) = 3 u (|s m2| + 1); ty alike.
  det = a d - b c     each product 2 + 2 + 1 roundings, the difference 1: |d det| <= 6 u (|a d| + |b c|) = 6 kappa u |det|,
                      kappa = (|a d| + |b c|) / |det|.
  R^-1                ia = d / det (ib, ic, id alike): 2 + 6 kappa + 1 roundings: rho = 3 + 6 kappa, |d ia| <= rho u |ia|.
  itx = -(ia tx + ib ty)   products: operand errors rho u |ia tx| + |ia| e_t(x) (and the ib ty term), + 1 rounding each, + 1 for the sum:
                      e_i(x) = (rho + 2) u (|ia tx| + |ib ty|) + |ia| e_t(x) + |ib| e_t(y); ity alike with ic, id.
  x, y of coord / pt3d_68 / the box corners   x' = ia x + ib y + itx: products rho + 1 roundings, two sums on terms <= the total magnitude:
                      |err| <= (rho + 3) u (|ia x| + |ib y|) + e_i(x) + 2 u |itx|          (y' alike)
                      The box is the min / max over its four corners: exact selections, 1-Lipschitz -> the maximum of the corners' bounds.
  size of coord       sqrt(ia^2 + ib^2 + ic^2 + id^2) 0.70710678f size: squares 2 rho + 1 on positive terms, 3 sums, halved by the root
                      (rho + 2), + 1 (root) + 2 (the rounded constant and its product) + 1 (times size): |err| <= (rho + 6) u |size'|
  z of pt3d_68        sqrt|ia id - ib ic| z: the determinant (2 rho + 2) kappa roundings (kappa of R^-1 equals kappa of A), halved,
                      + 1 (root) + 1 (product): |err| <= ((rho + 1) kappa + 2) u |z'|
  pose                z-rotation by alpha = atan2f(-ib, id): the operands carry rho u each, d atan2(y, x) = (x dy - y dx) / (x^2 + y^2)
                      <= rho u; + 6 ulp of atan2 (the device library's documented accuracy, as tests/ensemble_cases.py): err alpha <=
                      rho u + 6 2^-23 |alpha|; eps_s = 0.5 err alpha + 4 2^-23 for sin / cos of the half angle; a component is
                      z_w q_x +- z_k q_y: |err| <= sqrt(2) |q| (eps_s + 4 u)
  candidate / state   the clamp is 1-Lipschitz: the bound of the box.
Sign and validity decisions are compared exactly; the inputs keep det, w, h and max(w, h) f - 2 further from their thresholds than these
bounds (asserted on the CPU in the tests: a condition on the inputs, not a tolerance)."""
import math

import numpy as np
import torch

import ensemble_ref as ER
import track_ref as TR
from head_loss_cases import EPS24, GUARD, Guarded

U = EPS24
FILL_I32, FILL_U8 = -7777, 0xEE


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class IntGuarded:
    """Guarded for integer buffers: filled with a sentinel, GUARD elements longer than the kernel may write."""

    def __init__(self):
        self.bufs = {}

    def __call__(self, name, numel, dtype, fill, init=None):
        full = torch.full((numel + GUARD,), fill, dtype=dtype, device="cuda")
        if init is not None:
            full[:numel] = torch.as_tensor(init, dtype=dtype).reshape(-1).cuda()
        self.bufs[name] = (full, numel, fill)
        return full.data_ptr()

    def get(self, name):
        full, numel, _ = self.bufs[name]
        return full[:numel]

    def guard_intact(self, name):
        full, numel, fill = self.bufs[name]
        return bool((full[numel:] == fill).all())


# ---------------------------------------------------------------------------------------------
# ttk_track_crop
# ---------------------------------------------------------------------------------------------
def crop_case(L, dtype, seed, S=2, T=3, Hs=40, Ws=56):
    """Frames and L lanes mixing both sequences and the factors 1.0 / 1.2 / 0.9; boxes inside the frame, straddling each border and
    larger than the frame (zero padding), cycled over the lanes."""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (S, T, Hs, Ws), dtype=np.uint8) if dtype == "u8" else _f32(rng.uniform(0, 255, (S, T, Hs, Ws)))
    boxes = [[14.3, 9.6, 39.2, 31.1], [-6.5, 8.0, 17.25, 30.5], [38.0, 10.5, 63.5, 33.0], [16.0, -9.5, 40.0, 12.75], [15.5, 27.0, 41.0, 49.5],
             [-12.0, -20.0, 70.0, 58.0], [20.25, 12.5, 30.75, 20.0]]
    roi = _f32([boxes[i % len(boxes)] for i in range(L)])
    roi += _f32(rng.uniform(-0.2, 0.2, roi.shape))
    return {"frames": frames, "lane_seq": np.arange(L, dtype=np.int32) % S, "lane_factor": _f32([(1.0, 1.2, 0.9)[i % 3] for i in range(L)]),
            "roi_state": roi, "S": S, "T": T, "Hs": Hs, "Ws": Ws, "L": L}


def run_crop(case, N, t, L=None):
    """One ttk_track_crop on guarded buffers -> (Guarded floats, IntGuarded ints)."""
    from trackertraincode._hip import lib, ptr

    Lc = case["L"]
    dev = {k: torch.from_numpy(case[k]).cuda() for k in ("frames", "lane_seq", "lane_factor")}
    out, ints = Guarded(), IntGuarded()
    state = out("roi_state", Lc * 4)
    out.get("roi_state").copy_(torch.from_numpy(case["roi_state"]).reshape(-1))
    args = (ptr(dev["frames"]), int(case["frames"].dtype == np.uint8), case["S"], case["T"], case["Hs"], case["Ws"], ptr(dev["lane_seq"]),
            ptr(dev["lane_factor"]), state, ints("t", 1, torch.int32, FILL_I32, [t]), Lc if L is None else L, N, 1.0 / 256.0, -0.5,
            ints("view", Lc * 4, torch.int32, FILL_I32), out("tr", Lc * 6), out("crop", Lc * N * N))
    lib().call("ttk_track_crop", *args)
    torch.cuda.synchronize()
    return out, ints


def three_launches(case, N, t):
    """ttk_view_roi, ttk_roi_transform (null angles), ttk_affine_warp on the frames (lane_seq[l], t): what ttk_track_crop replaces."""
    from trackertraincode._hip import lib, ptr

    L = case["L"]
    roi, f = torch.from_numpy(case["roi_state"]).cuda(), torch.from_numpy(case["lane_factor"]).cuda()
    src = torch.from_numpy(case["frames"][case["lane_seq"], t]).cuda().contiguous()
    zero = torch.zeros((L, 2), dtype=torch.float32, device="cuda")
    view = torch.empty((L, 4), dtype=torch.int32, device="cuda")
    tr = torch.empty((L, 2, 3), dtype=torch.float32, device="cuda")
    crop = torch.empty((L, 1, N, N), dtype=torch.float32, device="cuda")
    lib().call("ttk_view_roi", ptr(roi), ptr(f), ptr(zero), 0.3, L, ptr(view))
    lib().call("ttk_roi_transform", ptr(view), None, L, N, ptr(tr))
    lib().call("ttk_affine_warp", ptr(src), int(src.dtype == torch.uint8), L, case["Hs"], case["Ws"], ptr(tr), ptr(crop), N, 1.0 / 256.0, -0.5)
    torch.cuda.synchronize()
    return view, tr, crop


# ---------------------------------------------------------------------------------------------
# ttk_track_update
# ---------------------------------------------------------------------------------------------
def flip_tr(tr, N):
    """The crop mirrored left-right: x -> N - x composed onto tr (det < 0: the flip map)."""
    out = tr.copy()
    out[0] = -tr[0]
    out[0, 2] += N
    return out


def update_case(L, seed, pts=True, N=129, T=5, Hs=96, Ws=128, special=True):
    """Network outputs in the crop's [-1, 1] coordinates and transforms as the tracker makes them (axis-aligned, from integer view boxes);
    with `special` and L >= 3, lane 1 is rotated by 0.4 rad about the crop centre and lane 2 mirrored."""
    rng = np.random.default_rng(seed)
    half = rng.uniform(14.0, 30.0, L)
    cx, cy = rng.uniform(40.0, Ws - 40.0, L), rng.uniform(35.0, Hs - 35.0, L)
    state = _f32(np.stack([cx - half, cy - half, cx + half, cy + half], -1))
    factor = _f32([(1.0, 1.2, 0.9)[i % 3] for i in range(L)])
    view, _ = TR.view_roi_f32(state, factor)
    tr = TR.roi_transform(view, N, np.float32)
    if special and L >= 3:
        c, s, h = math.cos(0.4), math.sin(0.4), 0.5 * N
        rot = np.array([[c, -s, h - (c * h - s * h)], [s, c, h - (s * h + c * h)], [0, 0, 1]])
        tr[1] = _f32((rot @ np.vstack([tr[1].astype(np.float64), [0, 0, 1]]))[:2])
        tr[2] = flip_tr(tr[2], N)
    ctr, sz = rng.uniform(-0.25, 0.25, (L, 2)), rng.uniform(0.3, 0.5, (L, 2))
    q = rng.standard_normal((L, 4))
    return {"roi": _f32(np.concatenate([ctr - sz, ctr + sz], -1)), "coord": _f32(np.concatenate([ctr, rng.uniform(0.3, 0.6, (L, 1))], -1)),
            "pose": _f32(q / np.linalg.norm(q, axis=-1, keepdims=True)), "pts": _f32(rng.uniform(-1.1, 1.1, (L, 68, 3))) if pts else None,
            "tr": tr, "lane_factor": factor, "roi_state": state, "L": L, "N": N, "T": T, "Hs": Hs, "Ws": Ws}


def run_update(case, t, L=None, with_traj_pts=None):
    """One ttk_track_update on guarded buffers."""
    from trackertraincode._hip import lib, ptr

    Lc, T = case["L"], case["T"]
    dev = {k: None if case[k] is None else torch.from_numpy(case[k]).cuda() for k in ("roi", "coord", "pose", "pts", "tr", "lane_factor")}
    out, ints = Guarded(), IntGuarded()
    state = out("roi_state", Lc * 4)
    out.get("roi_state").copy_(torch.from_numpy(case["roi_state"]).reshape(-1))
    traj_pts = (case["pts"] is not None) if with_traj_pts is None else with_traj_pts
    args = (ptr(dev["roi"]), ptr(dev["coord"]), ptr(dev["pose"]), ptr(dev["pts"]), ptr(dev["tr"]), ints("t", 1, torch.int32, FILL_I32, [t]),
            Lc if L is None else L, case["N"], T, case["Hs"], case["Ws"], ptr(dev["lane_factor"]), state, out("roi_in", T * Lc * 4),
            out("traj_roi", T * Lc * 4), out("traj_coord", T * Lc * 3), out("traj_pose", T * Lc * 4),
            out("traj_pts", T * Lc * 204) if traj_pts else None, ints("lost", T * Lc, torch.uint8, FILL_U8))
    lib().call("ttk_track_update", *args)
    torch.cuda.synchronize()
    return out, ints


def update_bounds(case, r):
    """The per-row bounds of the module docstring; `r` = track_ref.update(...) in float64.  Returns arrays shaped like the outputs."""
    m, N = case["tr"].astype(np.float64), case["N"]
    s = 2.0 / N
    a, b, c, d = s * m[:, 0, 0], s * m[:, 0, 1], s * m[:, 1, 0], s * m[:, 1, 1]
    tx, ty = s * m[:, 0, 2] - 1, s * m[:, 1, 2] - 1
    e_tx, e_ty = 3 * U * (np.abs(s * m[:, 0, 2]) + 1), 3 * U * (np.abs(s * m[:, 1, 2]) + 1)
    det = a * d - b * c
    kappa = (np.abs(a * d) + np.abs(b * c)) / np.abs(det)
    rho = 3 + 6 * kappa
    bk = r["back"]
    ia, ib, itx, ic, id_, ity = bk[:, 0, 0], bk[:, 0, 1], bk[:, 0, 2], bk[:, 1, 0], bk[:, 1, 1], bk[:, 1, 2]
    e_ix = (rho + 2) * U * (np.abs(ia * tx) + np.abs(ib * ty)) + np.abs(ia) * e_tx + np.abs(ib) * e_ty
    e_iy = (rho + 2) * U * (np.abs(ic * tx) + np.abs(id_ * ty)) + np.abs(ic) * e_tx + np.abs(id_) * e_ty

    def xy(x, y):  # [L] or [L,P] -> bounds of x', y'
        e = (lambda v: v) if x.ndim == 1 else (lambda v: v[:, None])
        x, y = np.abs(x.astype(np.float64)), np.abs(y.astype(np.float64))
        return ((e(rho) + 3) * U * (e(np.abs(ia)) * x + e(np.abs(ib)) * y) + e(e_ix) + 2 * U * e(np.abs(itx)),
                (e(rho) + 3) * U * (e(np.abs(ic)) * x + e(np.abs(id_)) * y) + e(e_iy) + 2 * U * e(np.abs(ity)))

    bd = {"det_margin": np.abs(det) - 6 * kappa * U * np.abs(det)}
    cx, cy = xy(case["coord"][:, 0], case["coord"][:, 1])
    bd["coord"] = np.stack([cx, cy, (rho + 6) * U * np.abs(r["coord"][:, 2])], -1)
    roi = case["roi"]
    with np.errstate(invalid="ignore"):
        bx, by = xy(np.nan_to_num(roi[:, [0, 2, 0, 2]], nan=0.0, posinf=0.0, neginf=0.0), np.nan_to_num(roi[:, [1, 1, 3, 3]], nan=0.0, posinf=0.0, neginf=0.0))
    bd["roi"] = np.stack([bx.max(-1), by.max(-1), bx.max(-1), by.max(-1)], -1)
    if case["pts"] is not None:
        px, py = xy(case["pts"][..., 0], case["pts"][..., 1])
        mir = det < 0
        px[mir], py[mir] = px[mir][:, ER.flip_map()], py[mir][:, ER.flip_map()]
        bd["pts"] = np.stack([px, py, (((rho + 1) * kappa + 2) * U)[:, None] * np.abs(r["pts"][..., 2])], -1)
    alpha = np.abs(np.arctan2(-ib, id_))
    eps_s = 0.5 * (rho * U + 6 * 2.0 ** -23 * alpha) + 4 * 2.0 ** -23
    with np.errstate(invalid="ignore"):
        n = np.linalg.norm(np.nan_to_num(case["pose"].astype(np.float64)), axis=-1)
    bd["pose"] = (math.sqrt(2.0) * n * (eps_s + 4 * U))[:, None] * np.ones(4)
    return bd


def decisions_are_safe(case, r, bd):
    """w, h and max(w, h) f - 2 of every finite candidate lie further from their thresholds than the row's bound; det keeps its sign."""
    assert np.all(bd["det_margin"] > 0), "det too close to 0 for its sign to be decided"
    cand, f = r["cand"], case["lane_factor"].astype(np.float64)
    pred = case["roi"].astype(np.float64)
    with np.errstate(invalid="ignore"):  # (a non-finite or inverted prediction is decided by exact comparisons of the inputs)
        fin = np.isfinite(r["roi"]).all(-1) & np.isfinite(pred).all(-1) & (pred[:, 2] > pred[:, 0]) & (pred[:, 3] > pred[:, 1])
    w, h = cand[:, 2] - cand[:, 0], cand[:, 3] - cand[:, 1]
    bw, bh = bd["roi"][:, 0] + bd["roi"][:, 2], bd["roi"][:, 1] + bd["roi"][:, 3]
    thr = np.maximum(w, h) * f - 2
    bt = np.maximum(bw, bh) * f + 2 * U * np.abs(thr + 2)
    assert np.all(np.abs(w[fin]) > bw[fin]) and np.all(np.abs(h[fin]) > bh[fin]) and np.all(np.abs(thr[fin]) > bt[fin]), \
        "a validity decision sits inside the rounding bound of its row: choose other inputs"


def within(name, got, ref, bound):
    if ref.size == 0:
        return
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), f"{name}: non-finite entries differ"
    err = np.abs(np.where(fin, got - np.where(fin, ref, 0), 0.0))
    bound = np.broadcast_to(bound, err.shape)
    worst = float((err[fin] / np.maximum(bound[fin], 1e-300)).max()) if fin.any() else 0.0
    print(f"  {name}: max |err| {err.max():.3e}, worst err / bound {worst:.3f}")
    assert np.all(err[fin] <= bound[fin]), f"{name}: |err| {err.max():.3e} exceeds its bound ({worst:.2f} x)"
