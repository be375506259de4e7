"""Cases, launches and error bounds of the ttk_ensemble_reduce tests (tests/test_ensemble_gpu.py, test_ensemble_predictor_gpu.py): the kernel through
the C-ABI on guarded buffers against tests/ensemble_ref.py in float64 on the same float32 inputs.

Tolerances, per output (u = 2^-24, first order in u with one rounding of slack for the higher orders; `mean_e` = mean over the members):

  x, y of pt3d_68 / coord   a member is a x + b y + t: two products and two sums, <= 4 roundings on terms of magnitude T_e = |a||x| + |b||y| + |t|.
                            The serial sum adds E - 1 roundings on partial sums <= sum_e T_e, the division by E one more:
                              |err| <= (E + 5) u mean_e T_e          (a coordinate near 1000 px over 16 members: 1.3e-3 px)
  z of pt3d_68              z sqrt|det|: det = a d - b c carries 3 roundings on |a d| + |b c| = kappa |det|, halved by the square root, + 1 for
                            the root, + 1 for the product: |err| <= (1.5 kappa + 2 + E + 1) u mean_e |z_e|
  size of coord             sqrt(a^2 + b^2 + c^2 + d^2) 0.70710678f s: 4 roundings on a sum of positive terms, halved, + 1 (root) + 2 (the rounded
                            constant and its product) + 1 (times s) = 6 relative: |err| <= (E + 7) u mean_e |size_e|
  shapeparam                no transform: (E + 1) u mean_e |s_e|
  pose                      z-rotation (0, 0, sg sin(alpha/2), cos(alpha/2)), alpha = atan2f(-b, d): the OpenCL accuracy the device library
                            documents is 6 ulp for atan2 and 4 ulp for sin / cos, so |err alpha| <= 6 2^-23 |alpha| and
                            eps_s = 0.5 |err alpha| + 4 2^-23 for either entry.  A transformed component is z_w q_x +- z_k q_y (+ exact zeros):
                            operand error eps_s (|q_x| + |q_y|) <= sqrt(2) |q_e| eps_s plus <= 4 roundings on the same magnitude:
                              delta_e = sqrt(2) |q_e| (eps_s + 4 u);   mean: delta = mean_e delta_e + E u mean_e |q_e|.
                            Normalisation: the Jacobian of v / |v| has norm 1 / |v| and the 4-vector error is <= 2 delta; |v| (4 roundings on
                            positive terms, halved, + 1) and the division add 4 u: |err pose| <= 2 delta / |mean| + 5 u
  stats[1] = |mean|         2 delta + 3 u |mean|
  stats[2..4] = std         std is a seminorm of the residuals r_e = x_e - mean: |err std| <= max_e |err r_e| + own roundings.  err r_e <= 4 u T_e
                            (member) + (E + 5) u T_max (mean) + 2 u T_max (the difference) = (E + 11) u T_max for x, y and (E + 15) u max_e |size_e|
                            for the size (6 and E + 7 instead of 4 and E + 5); squares, sum, division, root: (E + 4) u std
  stats[0] = geodesic       through atan2 of a square root: E_hip <= K["trans"] E_ref + FLOOR of tests/head_loss_cases.py, E_ref the error of the
                            float32 run of ensemble_ref against its float64 run, maxima over the rows of a case

Sign decisions: every drawn row keeps 1e-2 E between the two largest component sums of |q| of the TRANSFORMED members and 1e-2 in every member's
pivot component (rows are redrawn until they do), far above any float32 rounding; the exact tie is compared up to the global sign."""
import math

import numpy as np
import torch

import ensemble_ref as ER
from head_loss_cases import EPS24, FLOOR, K, Guarded
from util import gpu_section

U = EPS24
SEED_FAR = 35  # two of its three rows have |mean| = 0.48, 0.49 (float64, tests/ensemble_ref.py)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def _rotvec_quat(r):
    a = np.linalg.norm(r, axis=-1, keepdims=True)
    return np.concatenate([r / a * np.sin(0.5 * a), np.cos(0.5 * a)], -1)


def make_back(rng, B, mirrored=()):
    """Normalised crop -> image pixels: rotation, scale and shift per row; rows in `mirrored` flip x first (det < 0)."""
    ang, sc = rng.uniform(-math.pi, math.pi, B), rng.uniform(40.0, 200.0, B)
    sh = rng.uniform(50.0, 900.0, (B, 2))
    m = np.stack([np.stack([sc * np.cos(ang), -sc * np.sin(ang), sh[:, 0]], -1), np.stack([sc * np.sin(ang), sc * np.cos(ang), sh[:, 1]], -1)], 1)
    for b in mirrored:
        m[b, :, 0] *= -1.0
    return _f32(m)


def decided(pose_t):
    sums = np.sort(np.abs(pose_t).sum(0), axis=-1)
    pivot = np.argmax(np.abs(pose_t).sum(0), axis=-1)
    comp = np.take_along_axis(pose_t, pivot[None, :, None], axis=-1)[..., 0]
    return (sums[:, -1] - sums[:, -2] >= 1e-2 * pose_t.shape[0]) & (np.abs(comp).min(0) >= 1e-2)


def draw_pose(rng, E, B, back, sigma=0.05, signs=True):
    """Unit quaternions around a random base rotation per row, random member signs; rows are redrawn until their sign decisions are safe."""
    def draw(n):
        if sigma is None:  # members uniform on the sphere: nothing in common
            return _f32(_unit(rng.standard_normal((E, n, 4))))
        base = _unit(rng.standard_normal((n, 4)))
        q = np.stack([ER.qmul(base, _rotvec_quat(rng.normal(0.0, sigma, (n, 3)))) for _ in range(E)])
        return _f32(q * (rng.choice([-1.0, 1.0], (E, n, 1)) if signs else 1.0))

    q = draw(B)
    for _ in range(100):
        bad = np.flatnonzero(~decided(ER.back_transform(back, q, np.zeros((E, B, 3)))[0]))
        if not len(bad):
            return q
        q[:, bad] = draw(len(bad))
    raise AssertionError("no decided rows drawn")


def make_case(B, E, seed, S=50, pts=True, shape=True, mirrored=None, sigma=0.05):
    rng = np.random.default_rng(seed)
    back = make_back(rng, B, (B - 1,) if mirrored is None else mirrored)
    return {"back": back, "pose": draw_pose(rng, E, B, back, sigma), "coord": _f32(rng.uniform(-1, 1, (E, B, 3)) * [1, 1, 0.4] + [0, 0, 0.5]),
            "pts": _f32(rng.uniform(-1.2, 1.2, (E, B, 68, 3))) if pts else None, "shape": _f32(rng.normal(0, 1, (E, B, S))) if shape else None}


def run(inp, E=None):
    """One launch on guarded output buffers -> (Guarded, dict of numpy outputs)."""
    from trackertraincode._hip import lib, ptr

    Ein, B = inp["pose"].shape[:2]
    S = 0 if inp["shape"] is None else inp["shape"].shape[-1]
    dev = {k: None if v is None else torch.from_numpy(v).cuda() for k, v in inp.items()}
    out = Guarded()
    args = (ptr(dev["pose"]), ptr(dev["coord"]), ptr(dev["pts"]), ptr(dev["shape"]), ptr(dev["back"]), Ein if E is None else E, B, S,
            out("pose", B * 4), out("coord", B * 3), out("pts", B * 204) if inp["pts"] is not None else None,
            out("shape", B * S) if inp["shape"] is not None else None, out("stats", B * 5))
    lib().call("ttk_ensemble_reduce", *args)
    torch.cuda.synchronize()
    return out


def outputs(out, inp):
    B = inp["pose"].shape[1]
    got = {"pose": out.np("pose", B, 4), "coord": out.np("coord", B, 3), "stats": out.np("stats", B, 5)}
    got["pts"] = out.np("pts", B, 68, 3) if inp["pts"] is not None else None
    got["shape"] = out.np("shape", B, -1) if inp["shape"] is not None else None
    return {k: None if v is None else v.astype(np.float64) for k, v in got.items()}


def bounds(inp, r):
    """The per-output error bounds of the module docstring."""
    E, B = inp["pose"].shape[:2]
    m = inp["back"].astype(np.float64)
    a, b, tx, c, d, ty = m[:, 0, 0], m[:, 0, 1], m[:, 0, 2], m[:, 1, 0], m[:, 1, 1], m[:, 1, 2]
    det = a * d - b * c
    pose_t, coord_t, pts_t = r["members"]

    def mag_xy(xy):  # [E,B,...,2] -> T_e of x and y
        e = (lambda v: v[None, :]) if xy.ndim == 3 else (lambda v: v[None, :, None])
        x, y = np.abs(xy[..., 0].astype(np.float64)), np.abs(xy[..., 1].astype(np.float64))
        return np.stack([e(np.abs(a)) * x + e(np.abs(b)) * y + e(np.abs(tx)), e(np.abs(c)) * x + e(np.abs(d)) * y + e(np.abs(ty))], -1)

    bd = {}
    Tc = mag_xy(inp["coord"][..., :2])
    size = np.abs(coord_t[..., 2])
    bd["coord"] = np.concatenate([(E + 5) * U * Tc.mean(0), ((E + 7) * U * size.mean(0))[:, None]], -1)
    if inp["pts"] is not None:
        Tp = mag_xy(inp["pts"][..., :2])
        mir = det < 0
        Tp[:, mir] = Tp[:, mir][:, :, ER.flip_map(), :]
        kappa = (np.abs(a * d) + np.abs(b * c)) / np.abs(det)
        bz = ((1.5 * kappa + 2 + E + 1) * U)[:, None] * np.abs(pts_t[..., 2]).mean(0)
        bd["pts"] = np.concatenate([(E + 5) * U * Tp.mean(0), bz[..., None]], -1)
    if inp["shape"] is not None:
        bd["shape"] = (E + 1) * U * np.abs(inp["shape"].astype(np.float64)).mean(0)
    alpha = np.abs(np.arctan2(-b, d))
    eps_s = 0.5 * 6 * 2.0 ** -23 * alpha + 4 * 2.0 ** -23
    n = np.linalg.norm(inp["pose"].astype(np.float64), axis=-1)
    delta = (math.sqrt(2.0) * n * (eps_s + 4 * U)).mean(0) + E * U * n.mean(0)
    norm = r["stats"][:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):  # (a zero mean: its row is asserted on its own)
        bd["pose"] = (2 * delta / norm + 5 * U)[:, None] * np.ones(4)
    bd["norm"] = 2 * delta + 3 * U * norm
    std = r["stats"][:, 2:]
    bd["std"] = np.concatenate([(E + 11) * U * Tc.max(0), ((E + 15) * U * size.max(0))[:, None]], -1) + (E + 4) * U * std
    return bd


def within(name, got, ref, bound, up_to_sign=False):
    err = np.abs(got - ref)
    if up_to_sign:
        err = np.where((np.abs(got + ref).sum(-1) < np.abs(got - ref).sum(-1))[:, None], np.abs(got + ref), err)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"  {name}: max |err| {err.max():.3e}, worst err / bound {worst:.3f}")
    assert np.all(err <= bound), f"{name}: |err| {err.max():.3e} exceeds its bound ({worst:.2f} x)"


def compare(got, inp, what, up_to_sign=False, scale=1.0):
    """Outputs of the kernel (float64 copies) against ensemble_ref on `inp`; `scale` widens every bound by a stated factor (callers that
    compare two float32 paths with each other).  Returns the float64 reference."""
    r = ER.ensemble_reduce(inp["pose"], inp["coord"], inp["pts"], inp["shape"], inp["back"])
    r32 = ER.ensemble_reduce(inp["pose"], inp["coord"], inp["pts"], inp["shape"], inp["back"], dtype=np.float32)
    bd = bounds(inp, r)
    print(what)
    within("pose", got["pose"], r["pose"], scale * bd["pose"], up_to_sign)
    within("coord", got["coord"], r["coord"], scale * bd["coord"])
    if inp["pts"] is not None:
        within("pts", got["pts"], r["pts"], scale * bd["pts"])
    if inp["shape"] is not None:
        within("shape", got["shape"], r["shape"], scale * bd["shape"])
    within("mean norm", got["stats"][:, 1], r["stats"][:, 1], scale * bd["norm"])
    within("coord spread", got["stats"][:, 2:], r["stats"][:, 2:], scale * bd["std"])
    e_hip, e_ref = np.abs(got["stats"][:, 0] - r["stats"][:, 0]).max(), np.abs(r32["stats"][:, 0].astype(np.float64) - r["stats"][:, 0]).max()
    print(f"  geodesic: E_hip {e_hip:.3e}, E_ref {e_ref:.3e}")
    assert e_hip <= K["trans"] * e_ref + FLOOR, f"geodesic spread: E_hip {e_hip:.3e} > {K['trans']} x E_ref {e_ref:.3e} + floor"
    return r


def check(inp, what, up_to_sign=False):
    """One launch on guarded buffers, the guard words, and every output against float64."""
    with gpu_section():
        out = run(inp)
    out.check(what)
    got = outputs(out, inp)
    return got, compare(got, inp, what, up_to_sign)
