"""Case table of the per-row tests of the heads and loss kernels (tests/test_head_loss_cases.py on the CPU,
tests/test_loss_rows_gpu.py and tests/test_heads_rows_gpu.py on the GPU).

Deterministic builders (fixed seeds, float32 arrays) of row classes that sit on the branches of csrc/head_math.h and
csrc/loss_math.h: every class is a group of GROUP rows, a table is the concatenation of its classes, and `Table.cycle(n)` repeats a
table to n rows.  `LOSS_OPS` lists every single-op entry point of csrc/losses.hip (and ttk_diag_scale_*) with its rows and its
formula in the CPU oracle (oracle/refmodel.py), written once for any dtype: the float64 evaluation is the reference, the float32
evaluation is the yardstick of what the formula itself loses at the kernels' precision (`class_errors`, `assert_within`)."""
import math
import os

import numpy as np
import torch

from oracle import refmodel as R

GROUP = 16
EPS24 = 2.0 ** -24
FLOOR = 4 * EPS24  # a few roundings of the output itself, for classes where the float32 oracle happens to be exact
# E_hip <= K * E_ref + FLOOR: one K for the polynomial kinds, one for the chains through atan2 / log / exp / sin / cos (all of the heads).
# Twice the worst ratio measured on the MI355X, rounded up (tables in tests/test_loss_rows_gpu.py and tests/test_heads_rows_gpu.py).
K = {"poly": 5, "trans": 8}
TIE_GAP = 1.0e-3  # from_matrix: below this gap between the two largest arguments fp32 and float64 may differentiate different branches
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Table:
    """Rows of named float32 arrays (first axis = row) and the class name of every row."""

    def __init__(self, cls, **arrays):
        self.cls = np.asarray(cls)
        self.a = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
        assert all(len(v) == len(self.cls) for v in self.a.values())

    def __len__(self):
        return len(self.cls)

    def cycle(self, n):
        idx = np.arange(n) % len(self)
        return Table(self.cls[idx], **{k: v[idx] for k, v in self.a.items()})

    def rows(self, name):
        return np.flatnonzero(self.cls == name)


def concat(tables):
    keys = tables[0].a.keys()
    return Table(np.concatenate([t.cls for t in tables]), **{k: np.concatenate([t.a[k] for t in tables]) for k in keys})


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _qmul(u, v):
    ui, uj, uk, uw = np.moveaxis(u, -1, 0)
    vi, vj, vk, vw = np.moveaxis(v, -1, 0)
    return np.stack([ui * vw + uw * vi - uk * vj + uj * vk, uj * vw + uk * vi + uw * vj - ui * vk,
                     uk * vw - uj * vi + ui * vj + uw * vk, uw * vw - ui * vi - uj * vj - uk * vk], -1)


def _rotvec_quat(r):
    """exp of a rotation vector (float64): (axis sin(a/2), cos(a/2))"""
    a = np.linalg.norm(r, axis=-1, keepdims=True)
    axis = np.where(a > 0, r / np.where(a > 0, a, 1.0), 0.0)
    return np.concatenate([axis * np.sin(0.5 * a), np.cos(0.5 * a)], -1)


# ---- quaternion pairs (q, t) -------------------------------------------------------------------------------------------------
ANGLES = {"angle_1e-1": 1e-1, "angle_1e-2": 1e-2, "angle_1e-3": 1e-3, "angle_1e-4": 1e-4, "angle_0.9deg": math.radians(0.9),
          "angle_1.1deg": math.radians(1.1), "angle_pi-1e-3": math.pi - 1e-3}


def quat_pairs():
    rng = np.random.default_rng(101)
    g = GROUP
    tabs = []
    q = _unit(rng.standard_normal((g, 4)))
    tabs.append(Table(["generic"] * g, q=_f32(q), t=_f32(_unit(rng.standard_normal((g, 4))))))
    q = _f32(_unit(rng.standard_normal((g, 4))))
    tabs.append(Table(["same"] * g, q=q, t=q.copy()))
    q = _f32(_unit(rng.standard_normal((g, 4))))
    tabs.append(Table(["negated"] * g, q=q, t=-q))
    # exact half turns about x, y, z (and their negatives): the real part of conj(q) * t is exactly 0
    e = np.eye(4, dtype=np.float32)
    t = np.stack([e[i % 3] * (1.0 if (i // 3) % 2 == 0 else -1.0) for i in range(g)])
    tabs.append(Table(["half_turn"] * g, q=np.tile(e[3], (g, 1)), t=_f32(t)))
    for name, ang in ANGLES.items():
        q = _unit(rng.standard_normal((g, 4)))
        t = _qmul(q, _rotvec_quat(ang * _unit(rng.standard_normal((g, 3)))))
        tabs.append(Table([name] * g, q=_f32(q), t=_f32(t)))
    return concat(tabs)


ZERO_QUAT_CLASSES = ("same", "negated", "half_turn")  # geodesic distance and gradient exactly 0


# ---- rotation matrices ---------------------------------------------------------------------------------------------------------
def from_matrix_args(m):
    d0, d1, d2 = m[..., 0, 0], m[..., 1, 1], m[..., 2, 2]
    return np.maximum(np.stack([-d0 - d1 + d2, -d0 + d1 - d2, d0 - d1 - d2, d0 + d1 + d2], -1).astype(np.float64) + 1.0, 1.0e-6)


def tie_rows(m):
    """Rows whose two largest from_matrix arguments differ by less than TIE_GAP: value-only, no gradient comparison."""
    a = np.sort(from_matrix_args(m), -1)
    return (a[..., 3] - a[..., 2]) < TIE_GAP


def rot_matrices():
    rng = np.random.default_rng(102)
    g = GROUP
    z = _f32(rng.standard_normal((512, 6)))
    m = R.rot6d_to_matrix(torch.from_numpy(z)).numpy()
    a = np.sort(from_matrix_args(m), -1)
    keep = (a[:, 3] - a[:, 2]) > 1.0e-2  # generic rows are clear of the branch boundary
    picks = np.argmax(from_matrix_args(m), -1)
    sel = np.concatenate([np.flatnonzero(keep & (picks == p))[:g // 4] for p in range(4)])
    assert len(sel) == g and set(picks[sel].tolist()) == {0, 1, 2, 3}
    sel = sel[np.argsort(np.arange(g) % 4, kind="stable")]  # interleave the picks
    eye = np.eye(3, dtype=np.float32)
    diag = np.stack([np.diag(d).astype(np.float32) for d in ([1, -1, -1], [-1, 1, -1], [-1, -1, 1])])
    perm = np.stack([eye[[1, 2, 0]], eye[[2, 0, 1]]])
    tq = _f32(_unit(rng.standard_normal((4 * g, 4))))
    return Table(["generic"] * g + ["identity"] * g + ["half_turn_diag"] * g + ["four_way_tie"] * g,
                 m=np.concatenate([m[sel], np.tile(eye, (g, 1, 1)), diag[np.arange(g) % 3], perm[np.arange(g) % 2]]), t=tq)


# ---- 6D rotation features, quaternion head rows, triangular-scale rows ------------------------------------------------------------
def rot6d_features():
    rng = np.random.default_rng(103)
    g = GROUP
    gen = _f32(rng.standard_normal((g, 6)) * 0.7)
    col = _f32(rng.standard_normal((g, 6)) * 0.7)
    col[:, 3:] = col[:, :3] * 1.5
    tiny = _f32(rng.standard_normal((g, 6)) * 0.7)
    tiny[:, :3] = _f32(_unit(rng.standard_normal((g, 3))) * 3.0e-7)
    return Table(["generic"] * g + ["collinear"] * g + ["tiny_x"] * g, z=np.concatenate([gen, col, tiny]))


FALLBACK_6D_CLASSES = ("collinear", "tiny_x")


def quat_head_rows():
    rng = np.random.default_rng(104)
    g = GROUP
    clamp = np.tile(np.array([0, 0, 0, -20], np.float32), (g, 1))
    return Table(["generic"] * g + ["norm_clamp"] * g, z=np.concatenate([_f32(rng.standard_normal((g, 4)) * 0.7), clamp]))


def tri_scale_rows():
    rng = np.random.default_rng(105)
    g = GROUP
    return Table(["generic"] * g + ["floor"] * g + ["large"] * g,
                 x=np.concatenate([_f32(rng.standard_normal((g, 7)) * 0.7), np.full((g, 7), -30, np.float32), _f32(rng.uniform(5, 20, (g, 7)))]))


# ---- lower-triangular scales with residuals at 0, 1 and 100 sigma -----------------------------------------------------------------
def tril_cases():
    """L [.,3,3] and d = L (k u), |u| = 1: Mahalanobis distance k.  The far outlier is on the uniform branch of the mixture."""
    rng = np.random.default_rng(106)
    g = GROUP
    tabs = []
    for name, diag in (("generic", None), ("sharp", 1.0e-3), ("wide", 1.0e3)):
        for k in (0, 1, 100):
            L = np.zeros((g, 3, 3))
            dg = rng.uniform(0.3, 1.5, (g, 3)) if diag is None else np.full((g, 3), diag)
            L[:, [0, 1, 2], [0, 1, 2]] = dg
            L[:, 1, 0], L[:, 2, 0], L[:, 2, 1] = rng.normal(0, 0.3, (3, g)) * dg.mean(-1)
            L = _f32(L)
            d = np.einsum("nij,nj->ni", L.astype(np.float64), k * _unit(rng.standard_normal((g, 3))))
            tabs.append(Table([f"{name}/{k}sigma"] * g, L=L, d=_f32(d)))
    return concat(tabs)


def nllcoord_cases():
    rng = np.random.default_rng(107)
    t = tril_cases()
    c = _f32(rng.standard_normal((len(t), 3)) * 0.3)
    return Table(t.cls, c=c, t=_f32(c + t.a["d"]), L=t.a["L"])


def nllrot_cases():
    """Every quaternion-pair class under generic scales, and every scale class with the rotation delta as the residual (a rotation
    vector cannot be longer than pi: residuals beyond 3 rad are shortened to 3 rad).  Without sharp/1sigma: a float32 unit quaternion
    resolves a rotation to about 1e-7 rad, 1e-4 sigma of the sharp scale, so that row's residual - the input, not the arithmetic - is
    uncertain beyond the element-wise tolerances of the host-math check; sharp/0sigma (t == q, exact) and sharp/100sigma stay."""
    rng = np.random.default_rng(108)
    qp, tr = quat_pairs(), tril_cases()
    keep = tr.cls != "sharp/1sigma"
    tr = Table(tr.cls[keep], **{k: v[keep] for k, v in tr.a.items()})
    gen = tr.rows("generic/1sigma")
    a = Table(["pair/" + c for c in qp.cls], q=qp.a["q"], t=qp.a["t"], L=tr.a["L"][gen[np.arange(len(qp)) % len(gen)]])
    r = tr.a["d"].astype(np.float64)
    nr = np.linalg.norm(r, axis=-1, keepdims=True)
    r = np.where(nr > 3.0, r * 3.0 / np.maximum(nr, 1e-30), r)
    q = _unit(rng.standard_normal((len(tr), 4)))
    b = Table(["scale/" + c for c in tr.cls], q=_f32(q), t=_f32(_qmul(q, _rotvec_quat(r))), L=tr.a["L"])
    return concat([a, b])


# ---- element-wise rows -----------------------------------------------------------------------------------------------------------
def elem_rows(n, D, beta, seed):
    """p, t [n, D]; row class r: every element of the row has |p - t| at that multiple of beta (random signs)."""
    rng = np.random.default_rng(seed)
    names = ["generic", "zero", "0.5beta", "0.99beta", "1.01beta", "10beta"]
    mult = {"zero": 0.0, "0.5beta": 0.5, "0.99beta": 0.99, "1.01beta": 1.01, "10beta": 10.0}
    cls = np.array([names[(r // GROUP) % len(names)] for r in range(n)])
    t = _f32(rng.standard_normal((n, D)) * 0.5)
    e = rng.standard_normal((n, D)) * beta
    sign = rng.choice([-1.0, 1.0], (n, D))
    for r in range(n):
        if cls[r] != "generic":
            e[r] = sign[r] * mult[cls[r]] * beta
    p = _f32(t.astype(np.float64) + e)
    p[cls == "zero"] = t[cls == "zero"]
    return Table(cls, p=p, t=t)


def dist_rows(n, shape, seed):
    """mu, scale, x [n, *shape] for the Normal / Laplace likelihoods; row classes: generic, x == mu, scale 1e-3, scale 1e3."""
    rng = np.random.default_rng(seed)
    names = ["generic", "x_eq_mu", "scale_1e-3", "scale_1e3"]
    cls = np.array([names[(r // GROUP) % len(names)] for r in range(n)])
    full = (n,) + tuple(shape)
    mu = _f32(rng.standard_normal(full))
    sg = rng.uniform(0.3, 2.0, full)
    z = rng.standard_normal(full)
    bc = (slice(None),) + (None,) * len(shape)
    sg = np.where((cls == "scale_1e-3")[bc], 1.0e-3, np.where((cls == "scale_1e3")[bc], 1.0e3, sg))
    sg = _f32(sg)
    x = _f32(mu + sg.astype(np.float64) * z)
    x = np.where((cls == "x_eq_mu")[bc], mu, x)
    return Table(cls, mu=mu, sg=sg, x=_f32(x))


def quatreg_rows():
    rng = np.random.default_rng(109)
    g = GROUP
    unit = _f32(_unit(rng.standard_normal((g, 4))))
    tiny = np.tile(np.array([0, 0, 0, math.exp(-20.0)], np.float32), (g, 1))
    return Table(["generic"] * g + ["unit"] * g + ["tiny"] * g, q=np.concatenate([_f32(rng.standard_normal((g, 4))), unit, tiny]))


def gmm_rows():
    rng = np.random.default_rng(110)
    g = GROUP
    return Table(["generic"] * g + ["zeros"] * g + ["magnitude_20"] * g,
                 x=np.concatenate([_f32(0.5 * rng.standard_normal((g, 50))), np.zeros((g, 50), np.float32), _f32(20.0 * _unit(rng.standard_normal((g, 50))))]))


def diag_scale_rows(n):
    """hidden [n + 1]: the shared multiplier h[0], then one element per "row"."""
    x = tri_scale_rows()
    el = Table(np.repeat(x.cls[::GROUP], GROUP), h=np.concatenate([x.a["x"][x.rows(c), 1] for c in x.cls[::GROUP]])).cycle(n)
    return el.cls, np.concatenate([np.array([0.3], np.float32), el.a["h"]])


def cotangent(shape, seed=9):
    return _f32(np.random.default_rng(seed).standard_normal(shape))


class ShapeGmm64:
    """oracle.refmodel.ShapeGmm without its final cast to float32, and with the posteriors."""

    def __init__(self):
        self.g = R.ShapeGmm(os.path.join(GOLDEN, "shapeparams_gmm.npz"))
        g = self.g
        self.K = int(g.w.shape[0])
        self.ck = (torch.log(g.w) + torch.log(g.sinv).sum(-1) - g.normc).numpy().copy()  # what the host hands the kernel
        self.mu, self.sinv, self.fudge = g.mu.numpy().copy(), g.sinv.numpy().copy(), float(g.fudge)

    def __call__(self, x):
        g = self.g
        e = -0.5 * ((x.double()[:, None, :] - g.mu) * g.sinv).square().sum(-1)
        a = torch.log(g.w) + e + torch.log(g.sinv).sum(-1) - g.normc
        return -torch.logsumexp(a, -1) * g.fudge, torch.softmax(a, -1)


# =====================================================================================================================================
# the single-op entry points: rows + oracle formula
# =====================================================================================================================================
class LossOp:
    """name: id of the case; entry: C-ABI stem (ttk_<entry>_fwd / _bwd); group: "poly" or "trans" (atan2 / log / exp chains);
    make(n) -> (cls [n], inputs {name: float32 array}); fn(inputs as tensors of one dtype) -> output [n] or [n, w];
    wrt: the inputs the backward entry point differentiates, in the order of its output arguments; prm: integer / float arguments."""

    def __init__(self, name, entry, group, make, fn, wrt, prm=None, no_grad_rows=None):
        self.name, self.entry, self.group, self.make, self.fn, self.wrt, self.prm = name, entry, group, make, fn, wrt, prm or {}
        self.no_grad_rows = no_grad_rows  # inputs -> bool [n]: rows left out of the gradient comparison

    def __repr__(self):
        return self.name


def _tab(builder, *names):
    def make(n):
        t = builder().cycle(n)
        return t.cls, {k: t.a[k] for k in names}
    return make


def _weights(D, seed=7):
    w = _f32(np.random.default_rng(seed).uniform(0.2, 1.5, D))
    if D >= 3:
        w[1] = 0.0  # the kernels skip zero-weight columns
    return w


def _elem_op(kind, D, beta):
    code = {"l2": 0, "l1": 1, "smooth_l1": 2}[kind]

    def make(n):
        t = elem_rows(n, D, beta, seed=200 + D)
        return t.cls, {"p": t.a["p"], "t": t.a["t"], "colw": _weights(D)}

    def fn(i):
        return (R.elem_distance(kind, i["p"], i["t"], beta) * i["colw"][None, :]).sum(-1)

    return LossOp(f"elem/{kind}/beta{beta}/D{D}", "loss_elem", "poly", make, fn, ("p",), {"D": D, "kind": code, "beta": beta})


def _mse_rows_op(D):
    def make(n):
        t = elem_rows(n, D, 1.0, seed=300 + D)
        return t.cls, {"p": t.a["p"], "t": t.a["t"]}

    return LossOp(f"mse_rows/D{D}", "loss_mse_rows", "poly", make, lambda i: (i["p"] - i["t"]).square().mean(-1), ("p",), {"D": D})


def _mse_cols_op(c0, Dc, Dt):
    def make(n):
        t = elem_rows(n, Dt, 1.0, seed=400 + Dt + c0)
        return t.cls, {"p": t.a["p"], "t": t.a["t"]}

    return LossOp(f"mse_cols/c{c0}_{Dc}_of_{Dt}", "loss_mse_cols", "poly", make,
                  lambda i: (i["p"][:, c0:c0 + Dc] - i["t"][:, c0:c0 + Dc]).square().mean(-1), ("p",), {"Dt": Dt, "c0": c0, "Dc": Dc})


CHIN, EYE = 0.8, 0.0


def _points_op(dim):
    def make(n):
        t = elem_rows(n, 204, 1.0, seed=500 + dim)
        return t.cls, {"p": t.a["p"].reshape(n, 68, 3), "t": t.a["t"].reshape(n, 68, 3)}

    return LossOp(f"points/dim{dim}", "loss_points", "poly", make,
                  lambda i: R.loss_points3d({"pt3d_68": i["p"]}, {"pt3d_68": i["t"]}, dim), ("p",), {"dim": dim})


def _dist_op(dist, points, dim=3, per=204):
    entry = {"gaussian": "loss_normal", "laplace": "loss_laplace"}[dist]
    shape = (68, 3) if points else (per,)

    def make(n):
        t = dist_rows(n, shape, seed=600 + per + dim)
        return t.cls, {"mu": t.a["mu"], "sg": t.a["sg"], "x": t.a["x"]}

    if points:
        fn = lambda i: R.loss_nllpoints3d_dist({"pt3d_68": i["mu"], "pt3d_68_scales": i["sg"]}, {"pt3d_68": i["x"]}, dist, dim, CHIN, EYE)
    else:
        fn = lambda i: -R._dist_logprob(dist)(i["x"], i["mu"], i["sg"]).mean(-1)
    name = f"{dist}/points{dim}" if points else f"{dist}/per{per}"
    return LossOp(name, entry, "trans", make, fn, ("mu", "sg"), {"per": per, "points": int(points), "dim": dim})


def _diag_scale_make(n):
    cls, h = diag_scale_rows(n)
    return cls, {"h": h}


LOSS_OPS = [
    LossOp("rot", "loss_rot", "poly", _tab(quat_pairs, "q", "t"), lambda i: R.loss_rot({"rot": i["q"]}, {"pose": i["t"]}), ("q",)),
    LossOp("rot_geodesic", "loss_rot_geodesic", "trans", _tab(quat_pairs, "q", "t"),
           lambda i: R.loss_rot_smooth_geodesic({"rot": i["q"]}, {"pose": i["t"]}), ("q",)),
    LossOp("rot6d", "loss_rot6d", "poly", _tab(rot_matrices, "m", "t"), lambda i: R.loss_rot6d({"rot": i["m"]}, {"pose": i["t"]}), ("m",)),
    LossOp("ortho6d", "loss_ortho6d", "poly", _tab(rot6d_features, "z"), lambda i: R.loss_ortho6d({"unnormalized_6drepr": i["z"]}, None), ("z",)),
    LossOp("mat_to_quat", "mat_to_quat", "poly", _tab(rot_matrices, "m"), lambda i: R.matrix_to_quat(i["m"]), ("m",),
           no_grad_rows=lambda i: tie_rows(i["m"])),
    LossOp("quatreg", "loss_quatreg", "poly", _tab(quatreg_rows, "q"), lambda i: R.loss_quatreg({"unnormalized_quat": i["q"]}, None), ("q",)),
    LossOp("nllrot", "loss_nllrot", "trans", _tab(nllrot_cases, "q", "t", "L"),
           lambda i: R.loss_nllrot({"rot": i["q"], "pose_scales_tril": i["L"]}, {"pose": i["t"]}), ("q", "L")),
    LossOp("nllcoord", "loss_nllcoord", "trans", _tab(nllcoord_cases, "c", "t", "L"),
           lambda i: R.loss_nllcoord({"coord": i["c"], "coord_scales": i["L"]}, {"coord": i["t"]}), ("c", "L")),
    LossOp("diag_scale", "diag_scale", "trans", _diag_scale_make, lambda i: R.diagonal_scale_parameter(i["h"]), ("h",)),
    *[_mse_rows_op(D) for D in (1, 3, 4, 50, 64, 65, 204)],
    *[_mse_cols_op(*w) for w in ((0, 2, 3), (2, 1, 3), (0, 3, 3), (60, 70, 204))],
    *[_points_op(dim) for dim in (2, 3)],
    *[_dist_op(dist, True, dim=dim) for dist in ("gaussian", "laplace") for dim in (2, 3)],
    *[_dist_op(dist, False, per=per) for dist in ("gaussian", "laplace") for per in (4, 50, 65)],
    *[_elem_op("smooth_l1", D, 0.1) for D in (1, 3, 4, 50, 64, 65, 204)],
    *[_elem_op(kind, D, 1.0) for kind in ("l2", "l1", "smooth_l1") for D in (3, 65)],
]
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000)


def oracle(op, inputs, dtype):
    """(output, {input name: gradient}, gv) of `op` in `dtype` on the CPU, as float64 arrays; gv: the fixed random cotangent of the output."""
    t = {k: torch.from_numpy(v).to(dtype) for k, v in inputs.items()}
    for k in op.wrt:
        t[k].requires_grad_(True)
    out = op.fn(t)
    gv = cotangent(tuple(out.shape))
    (out * torch.from_numpy(gv).to(out.dtype)).sum().backward()
    return out.detach().double().numpy(), {k: t[k].grad.double().numpy() for k in op.wrt}, gv


# =====================================================================================================================================
# the comparison
# =====================================================================================================================================
def _rows2d(a, n):
    return np.asarray(a, np.float64).reshape(n, -1)


def zero_rows(ref64, n):
    """Rows whose float64 reference is exactly zero in every element."""
    return ~_rows2d(ref64, n).any(-1)


def class_errors(got, ref64, cls, skip=None):
    """{class: max over its rows of max|got - ref64| / s_row}, s_row = max|ref64| of the row floored by the class median of that.
    Rows whose reference is exactly zero (they are asserted to be exactly zero instead) and rows in `skip` are left out."""
    n = len(cls)
    got, ref = _rows2d(got, n), _rows2d(ref64, n)
    mag = np.abs(ref).max(-1)
    err = np.abs(got - ref).max(-1)
    use = mag > 0
    if skip is not None:
        use &= ~skip
    out = {}
    for c in dict.fromkeys(cls.tolist()):
        rows = np.flatnonzero((cls == c) & use)
        if len(rows):
            s = np.maximum(mag[rows], np.median(mag[rows]))
            out[c] = float((err[rows] / s).max())
    return out


def excess_ratio(e_hip, e_ref):
    """The K that `assert_within` would need: (E_hip - FLOOR) / E_ref (0 inside the floor, inf if the yardstick is exact and E_hip is not)."""
    over = e_hip - FLOOR
    if over <= 0:
        return 0.0
    return over / e_ref if e_ref > 0 else float("inf")


def assert_within(e_hip, e_ref, K, what, report=None):
    """E_hip <= K * E_ref + FLOOR for every class; prints both figures first."""
    worst = 0.0
    for c in e_hip:
        r = excess_ratio(e_hip[c], e_ref[c])
        worst = max(worst, r)
        print(f"ROWS {what} class={c} E_hip={e_hip[c]:.3e} E_ref={e_ref[c]:.3e} ratio={r:.2f}")
    if report is not None:
        report.append((what, worst))
    for c in e_hip:
        assert e_hip[c] <= K * e_ref[c] + FLOOR, f"{what} class {c}: E_hip {e_hip[c]:.3e} > {K} x E_ref {e_ref[c]:.3e} + {FLOOR:.1e}"


# =====================================================================================================================================
# the heads: configurations, edge rows of z, the oracle on a given z, and the C-ABI calls with guarded buffers
# =====================================================================================================================================
HEAD_CONFIGS = [(1, 1, 0, 1), (0, 1, 0, 1), (0, 0, 0, 1), (1, 1, 1, 1), (0, 0, 1, 1), (1, 1, 0, 0), (1, 1, 1, 0)]  # unc, pt, rot6d, use_offset
HEAD_OUT = {"roi": 4, "coord": 3, "rot": None, "qu": None, "Lc": 9, "Lr": 9, "pts": 204, "shp": 50}


def head_nz(unc, pt, rot6d):
    return 11 + 2 * rot6d + 14 * unc + 50 * pt


def head_outputs(cfg):
    """kernel output -> (name in the oracle's output dict, floats per sample), in the order of ttk_heads_fwd's arguments"""
    unc, pt, rot6d, _ = cfg
    o = {"roi": ("roi", 4), "coord": ("coord", 3), "rot": ("rot", 9 if rot6d else 4),
         "qu": ("unnormalized_6drepr", 6) if rot6d else ("unnormalized_quat", 4)}
    if unc:
        o["Lc"], o["Lr"] = ("coord_scales", 9), ("pose_scales_tril", 9)
    if pt:
        o["pts"], o["shp"] = ("pt3d_68", 204), ("shapeparam", 50)
    return o


def head_edge_rows(cfg, seed=120):
    """(cls [n], z [n, NZ]): generic rows of z whose rotation rows (and, with uncertainty, triangular-scale rows) are the edge classes."""
    unc, pt, rot6d, _ = cfg
    rng = np.random.default_rng(seed)
    rot = rot6d_features() if rot6d else quat_head_rows()
    tri = tri_scale_rows()
    n = 96
    NZ = head_nz(unc, pt, rot6d)
    z = _f32(rng.standard_normal((n, NZ)) * 0.7)
    r = np.arange(n)
    w = 6 if rot6d else 4
    z[:, 7:7 + w] = rot.a["z"][r % len(rot)]
    cls = rot.cls[r % len(rot)].astype(object)
    if unc:
        z[:, 7 + w:14 + w] = tri.a["x"][(r // 2) % len(tri)]
        z[:, 14 + w:21 + w] = tri.a["x"][(r // 2 + GROUP) % len(tri)]
        cls = cls + "/" + tri.cls[(r // 2) % len(tri)]
    return np.array([str(c) for c in cls]), z


def identity_state(cfg, Prow, Pkrow, dtype):
    """State whose linear layers pick rows of z (tests/test_host_math.py::_identity_state, any head layout, any dtype): heads_forward(st, z)
    then is the head arithmetic on z.  The pose offsets are per-sample rows (set_id = arange(B)), so their gradients are per sample."""
    unc, pt, rot6d, _ = cfg
    NZ = head_nz(unc, pt, rot6d)
    eye = torch.eye(NZ, dtype=dtype)
    st = {}

    def lin(prefix, lo, n):
        st[prefix + ".weight"] = eye[lo:lo + n].clone()
        st[prefix + ".bias"] = torch.zeros(n, dtype=dtype)

    w = 6 if rot6d else 4
    lin("boxnet.linear", 0, 4)
    lin("posnet.linear_xy", 4, 2)
    lin("posnet.linear_size", 6, 1)
    lin("quatnet.linear", 7, w)
    if unc:
        lin("posnet.scales.neck.lin", 7 + w, 7)
        lin("quatnet.uncertainty_net.neck.lin", 14 + w, 7)
        md = torch.tensor([np.float32(1e-6)] * 3 + [0.0] * 3).to(dtype)  # the kernels' 1.0e-6f
        st["posnet.scales.min_diag"], st["quatnet.uncertainty_net.min_diag"] = md, md.clone()
        st["boxnet.scales.hidden_scale"] = torch.zeros(5, dtype=dtype)
        st["landmarks.point_distrib_scales.hidden_scale"] = torch.zeros(69, dtype=dtype)
        st["landmarks.shape_distrib_scales.hidden_scale"] = torch.zeros(51, dtype=dtype)
    st["local_pose_offset.p"] = torch.from_numpy(Prow).to(dtype).requires_grad_(True)
    st["local_pose_offset_kpts.p"] = torch.from_numpy(Pkrow).to(dtype).requires_grad_(True)
    if pt:
        from oracle.synth import synthetic_keypoint_buffers

        kp, ke = synthetic_keypoint_buffers()
        st["landmarks.deformablekeypoints.keypts"] = torch.from_numpy(kp).to(dtype)
        st["landmarks.deformablekeypoints.keyeigvecs"] = torch.from_numpy(ke).to(dtype)
        lin("landmarks.shapenet", 7 + w + (14 if unc else 0), 50)
    return st


def heads_oracle(cfg, z, Prow, Pkrow, ups, dtype):
    """Head arithmetic of the oracle on given z [B, NZ] in `dtype`: ({kernel output: [B, w] float64}, dz [B, NZ], dprow [B, 8])."""
    unc, pt, rot6d, use_offset = cfg
    B = z.shape[0]
    st = identity_state(cfg, Prow, Pkrow, dtype)
    zt = torch.from_numpy(z).to(dtype).requires_grad_(True)
    out = R.heads_forward(st, zt, torch.arange(B), enable_point_head=bool(pt), enable_uncertainty=bool(unc),
                          use_local_pose_offset=bool(use_offset), training=True, enable_6drot=bool(rot6d))
    names = head_outputs(cfg)
    sum((out[o].reshape(B, -1) * torch.from_numpy(ups[k]).to(dtype)).sum() for k, (o, _) in names.items()).backward()
    g = lambda t: t.grad.double().numpy() if t.grad is not None else np.zeros((B, 4))
    dprow = np.concatenate([g(st["local_pose_offset.p"]), g(st["local_pose_offset_kpts.p"])], 1)
    return {k: out[o].detach().double().reshape(B, -1).numpy() for k, (o, _) in names.items()}, zt.grad.double().numpy(), dprow


GUARD = 64


class Guarded:
    """Output buffers of one launch: NaN-filled, GUARD elements longer than the kernel may write."""

    def __init__(self):
        self.bufs = {}

    def __call__(self, name, numel, dtype=torch.float32):
        full = torch.full((numel + GUARD,), float("nan"), dtype=dtype, device="cuda")
        self.bufs[name] = (full, numel)
        return full.data_ptr()

    def get(self, name):
        full, numel = self.bufs[name]
        return full[:numel]

    def np(self, name, *shape):
        return self.get(name).cpu().numpy().reshape(*shape)

    def check(self, what):
        for name, (full, numel) in self.bufs.items():
            assert bool(full[numel:].isnan().all()), f"{what}: {name} written past its {numel} elements"
            assert not bool(full[:numel].isnan().any()), f"{what}: {name} not written completely (or NaN)"


class HeadsProblem:
    """Inputs of one ttk_heads_fwd / ttk_heads_bwd case on the device."""

    def __init__(self, cfg, B, F, seed=0, ids="random", feat=None, picker=False):
        from oracle.synth import synthetic_keypoint_buffers

        unc, pt, rot6d, use_offset = cfg
        rng = np.random.default_rng(seed)
        self.cfg, self.B, self.F, self.NZ = cfg, B, F, head_nz(unc, pt, rot6d)
        NZ = self.NZ
        self.feat = _f32(np.abs(rng.standard_normal((B, F))) * 0.5) if feat is None else feat
        if picker:  # z = feat[:, :NZ]
            self.W, self.b = np.eye(NZ, F, dtype=np.float32), np.zeros(NZ, np.float32)
        else:
            self.W, self.b = _f32(rng.standard_normal((NZ, F)) / math.sqrt(F)), _f32(rng.standard_normal(NZ) * 0.3)
        self.absent = 5
        if ids is None:
            self.ids = None
        else:
            i = rng.integers(0, 7, B)
            self.ids = (i + (i >= self.absent)).astype(np.int32)  # 0..7 without `absent`
        self.P, self.Pk = _f32(rng.standard_normal((8, 4)) * 0.3), _f32(rng.standard_normal((8, 4)) * 0.3)
        self.kp, self.eig = synthetic_keypoint_buffers()
        self.ups = {k: _f32(rng.standard_normal((B, w))) for k, (_, w) in head_outputs(cfg).items()}
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(getattr(self, k))).cuda() for k in ("feat", "W", "b", "P", "Pk", "kp", "eig")}
        self.dev["ids"] = None if self.ids is None else torch.from_numpy(self.ids).cuda()
        self.dev_ups = {k: torch.from_numpy(v).cuda() for k, v in self.ups.items()}

    def rows_of(self, M):
        """Per-sample rows of the offset parameters [8, 4] -> [B, 4]"""
        return M[np.zeros(self.B, np.int64) if self.ids is None else self.ids]

    def forward(self):
        from trackertraincode._hip import lib, ptr

        unc, pt, rot6d, use_offset = self.cfg
        d, B, out = self.dev, self.B, Guarded()
        z = out("z", B * self.NZ)
        o = {k: out(k, B * w) for k, (_, w) in head_outputs(self.cfg).items()}
        lib().call("ttk_heads_fwd", ptr(d["feat"]), ptr(d["W"]), ptr(d["b"]), ptr(d["ids"]), ptr(d["P"]), ptr(d["Pk"]), ptr(d["kp"]), ptr(d["eig"]),
                   B, self.F, self.NZ, unc, pt, use_offset, rot6d, z, o["roi"], o["coord"], o["rot"], o["qu"], o.get("Lc"), o.get("Lr"),
                   o.get("pts"), o.get("shp"))
        return out

    def backward(self, z):
        """z: device tensor [B * NZ] (the forward's own)"""
        from trackertraincode._hip import lib, ptr

        unc, pt, rot6d, use_offset = self.cfg
        d, B, out, u = self.dev, self.B, Guarded(), self.dev_ups
        g = lambda k: ptr(u[k]) if k in u else None
        dz, dprow, dfeat = out("dz", B * self.NZ), out("dprow", B * 8), out("dfeat", B * self.F)
        dW, db = out("dW", self.NZ * self.F), out("db", self.NZ)
        dP, dPk = (out("dP", 32), out("dPk", 32)) if use_offset else (None, None)
        lib().call("ttk_heads_bwd", ptr(d["feat"]), ptr(d["W"]), ptr(z), ptr(d["ids"]), ptr(d["P"]), ptr(d["Pk"]), ptr(d["kp"]), ptr(d["eig"]),
                   B, self.F, self.NZ, unc, pt, use_offset, rot6d, g("roi"), g("coord"), g("rot"), g("qu"), g("Lc"), g("Lr"), g("pts"), g("shp"),
                   dz, dprow, dfeat, dW, db, dP, dPk)
        return out

    def check_linear(self, z):
        """Stage 1: z against feat W^T + b in float64, |err| <= (F + 8) 2^-24 (|feat| |W|^T + |b|) (standard accumulation bound)."""
        f, W, b = self.feat.astype(np.float64), self.W.astype(np.float64), self.b.astype(np.float64)
        bound = (self.F + 8) * EPS24 * (np.abs(f) @ np.abs(W).T + np.abs(b))
        err = np.abs(z - (f @ W.T + b))
        assert (err <= bound).all(), f"z: {int((err > bound).sum())} elements beyond the accumulation bound, worst {float((err / np.maximum(bound, 1e-300)).max()):.2f} x"

    def check_reductions(self, out):
        """Stage 4: the reductions of the kernel's own dz / dprow; bounds hold in any summation order."""
        B, F, NZ = self.B, self.F, self.NZ
        dz, dprow = out.np("dz", B, NZ).astype(np.float64), out.np("dprow", B, 8).astype(np.float64)
        f, W = self.feat.astype(np.float64), self.W.astype(np.float64)

        def within(name, got, ref, bound):
            err = np.abs(got - ref)
            assert (err <= bound).all(), f"{name}: {int((err > bound).sum())} elements beyond the bound, worst {float((err / np.maximum(bound, 1e-300)).max()):.2f} x"

        within("dfeat", out.np("dfeat", B, F), dz @ W, (NZ + 4) * EPS24 * (np.abs(dz) @ np.abs(W)))
        within("dW", out.np("dW", NZ, F), dz.T @ f, (B + 8) * EPS24 * (np.abs(dz).T @ np.abs(f)))
        within("db", out.np("db", NZ), dz.sum(0), (B + 8) * EPS24 * np.abs(dz).sum(0))
        if self.cfg[3]:
            ids = np.zeros(B, np.int64) if self.ids is None else self.ids
            onehot = (ids[:, None] == np.arange(8)[None, :]).astype(np.float64)  # [B, 8]
            for name, cols in (("dP", dprow[:, :4]), ("dPk", dprow[:, 4:])):
                got = out.np(name, 8, 4)
                within(name, got, onehot.T @ cols, (B + 8) * EPS24 * (onehot.T @ np.abs(cols)))
                unused = np.setdiff1d(np.arange(8), ids)
                assert self.absent in unused and not got[unused].any(), f"{name}: rows of ids that no sample has must be exactly 0"
