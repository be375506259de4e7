"""Cases, launches and bounds shared by the face-model fit tests (tests/test_facefit_ref.py on the CPU, tests/test_facefit_gpu.py on the
device): the planted cases the optimiser is run on, both float64 references on them (tests/facefit_ref.py: the project's optimiser
restated in numpy, and scipy's BFGS on the same objective), FIT_OBJ_MARGIN, and the C-ABI launches on guarded buffers.

Planted cases: landmarks of a random pose (yaw up to +-70 degrees) and shape (sigma 0.5) of the synthetic basis of oracle/synth.py with
noise 0.005, started 0.1 rad off with zero shape; B in (1, 3, 65), both weight modes.  Computed once per process and left unchanged.

Bounds.
  objective parity (kernel against restatement, both float64 on the same float32 inputs): facefit_ref.objective_bound - 256 roundings
    (the longest serial chain is the 204-term sum of a shape gradient; the rest is shorter) on the sum of the MAGNITUDES of the terms,
    first order in eps = 2^-53, the way tests/ensemble_cases.bounds takes first-order bounds on term magnitudes.
  FIT_OBJ_MARGIN = 2 x the largest amount by which the restatement's final objective exceeds scipy's over the planted cases: the gap
    between two correct optimisers that stop at the same gradient tolerance, measured, not chosen."""
from __future__ import annotations

import functools

import numpy as np
import torch

import facefit_ref as R

BATCHES = (1, 3, 65)
MODES = (False, True)  # fit_3d_projections


def seed_of(B, mode):
    return 4000 + 10 * B + int(mode)


@functools.lru_cache(maxsize=None)
def model(K=None):
    return R.synthetic_model(K)


@functools.lru_cache(maxsize=None)
def planted(B, mode):
    """(x0, target, weight) float32 + the two references' fits per sample."""
    x0, y, w = R.planted_cases(model(), B, seed_of(B, mode), mode)
    ours = [R.fit(model(), x0[b], y[b], w[b]) for b in range(B)]
    scipy_ = [R.fit_scipy(model(), x0[b], y[b], w[b]) for b in range(B)]
    for a in (x0, y, w):
        a.setflags(write=False)
    return x0, y, w, ours, scipy_


@functools.lru_cache(maxsize=None)
def fit_obj_margin():
    worst = 0.0
    for B in BATCHES:
        for mode in MODES:
            _, _, _, ours, sc = planted(B, mode)
            worst = max(worst, max(o["f"] - s["f"] for o, s in zip(ours, sc)))
    return 2.0 * worst


# ---------------------------------------------------------------------------------------------
# launches through the C-ABI on guarded buffers
# ---------------------------------------------------------------------------------------------
INT_GUARD = -0x5A5A5A5A


class Buffers:
    """head_loss_cases.Guarded for the float outputs plus sentinel-filled int32 buffers (NaN has no int32 form)."""

    def __init__(self):
        from head_loss_cases import GUARD, Guarded

        self.f, self.ints, self.guard = Guarded(), {}, GUARD

    def __call__(self, name, numel, dtype=torch.float32):
        if dtype == torch.int32:
            full = torch.full((numel + self.guard,), INT_GUARD, dtype=torch.int32, device="cuda")
            self.ints[name] = (full, numel)
            return full.data_ptr()
        return self.f(name, numel, dtype)

    def np(self, name, *shape):
        if name in self.ints:
            full, numel = self.ints[name]
            return full[:numel].cpu().numpy().reshape(*shape)
        return self.f.np(name, *shape)

    def bands_intact(self, what):
        for name, (full, numel) in list(self.f.bufs.items()):
            assert bool(full[numel:].isnan().all()), f"{what}: {name} written past its {numel} elements"
        for name, (full, numel) in self.ints.items():
            assert bool((full[numel:] == INT_GUARD).all()), f"{what}: {name} written past its {numel} elements"

    def untouched(self, what):
        self.bands_intact(what)
        for name, (full, numel) in list(self.f.bufs.items()):
            assert bool(full[:numel].isnan().all()), f"{what}: {name} was written"
        for name, (full, numel) in self.ints.items():
            assert bool((full[:numel] == INT_GUARD).all()), f"{what}: {name} was written"

    def check(self, what):
        self.f.check(what)
        self.bands_intact(what)
        for name, (full, numel) in self.ints.items():
            assert bool((full[:numel] != INT_GUARD).all()), f"{what}: {name} not written completely"


class DeviceModel:
    def __init__(self, m: R.Model):
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
        self.t = (f32(m.kp), f32(m.eig), f64(m.ck), f64(m.mu), f64(m.sinv))
        self.K = m.K

    def args(self, null=None, K=None):
        from trackertraincode._hip import ptr

        return tuple(None if i == null else ptr(t) for i, t in enumerate(self.t)) + (self.K if K is None else K,)


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()  # (a copy: the planted arrays are read-only)


def launch_objective(dm, x, y, w, n_free, raw=False, **model_kw):
    """ttk_facefit_objective -> Buffers with f [B] and g [B,57]; raw=True returns (rc, error string, Buffers) instead of raising."""
    from trackertraincode._hip import ptr

    B = len(x)
    keep = (_dev(x), _dev(y), _dev(w))
    out = Buffers()
    args = (ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), *dm.args(**model_kw), B, n_free, out("f", B, torch.float64), out("g", B * 57, torch.float64))
    return _call("ttk_facefit_objective", args, out, raw)


def launch_fit(dm, x0, y, w, iters=R.ITERS, gtol=R.GTOL, raw=False, null_x0=False, B=None, **model_kw):
    """ttk_facefit -> Buffers with x [B,57], pts [B,68,3], f [B,2], status [B], iters [B,2]."""
    from trackertraincode._hip import ptr

    n = len(x0)
    B = n if B is None else B  # (B = 0 with real buffers: the no-launch path)
    keep = (_dev(x0), _dev(y), _dev(w))
    out = Buffers()
    args = (None if null_x0 else ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), *dm.args(**model_kw), B, int(iters[0]), float(gtol[0]), int(iters[1]),
            float(gtol[1]), out("x", n * 57), out("pts", n * 204), out("f", n * 2, torch.float64), out("status", n, torch.int32),
            out("iters", n * 2, torch.int32))
    return _call("ttk_facefit", args, out, raw)


def _call(name, args, out, raw):
    from trackertraincode._hip import lib, _cur_device, _raw_stream

    L = lib()
    if not raw:
        L.call(name, *args)
        torch.cuda.synchronize()
        return out
    rc = L._fns[name](*args, _raw_stream(_cur_device()))
    torch.cuda.synchronize()
    return rc, L.cdll.ttk_last_error_string().decode(errors="replace"), out


def fit_outputs(out, B):
    return {"x": out.np("x", B, 57), "pts": out.np("pts", B, 68, 3), "f": out.np("f", B, 2), "status": out.np("status", B),
            "iters": out.np("iters", B, 2)}
