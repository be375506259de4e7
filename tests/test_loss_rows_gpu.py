"""Every single-op entry point of csrc/losses.hip (and ttk_diag_scale_* of csrc/heads.hip) against the CPU oracle in float64, row by
row, through the C-ABI: the row classes of tests/head_loss_cases.py cycled to n in SIZES (the tails of the 256-thread blocks and of
the 4-waves-per-block wave-per-sample kernels), NaN-filled outputs with a 64-element guard band, two runs that must be bitwise equal,
and the same ops once more inside ttk_loss_batch launches.

Criterion per class of rows and per output: E_hip <= K * E_ref + 4 * 2^-24 with E = max over the rows of max|x - f64| / s_row
(head_loss_cases.class_errors); E_ref is the oracle's own formula evaluated in float32 on the CPU.  Rows whose float64 value or
gradient is exactly zero must be exactly zero on the device.

Measured on an MI355X (gfx950), ROCm 7.2.0: the worst (E_hip - 4 * 2^-24) / E_ref over all classes and all n, per entry point and
output (0: inside the floor), and the class it occurred in.  K = twice the worst ratio of the group, rounded up.

  polynomial kinds                      ratio   class                 transcendental kinds                ratio   class
  rot           value                   2.24    angle_1e-4 (*)        rot_geodesic  value                 1.19    angle_0.9deg
  rot           dq                      0.48    angle_pi-1e-3         rot_geodesic  dq                    0.94    angle_1e-3
  quatreg       value                   0.97    unit (*)              nllrot        value                 0.26    scale/generic/0sigma
  quatreg       dq                      0.43    unit (*)              nllrot        dq                    1.30    pair/angle_1e-3
  rot6d, ortho6d, mat_to_quat,                                        nllrot        dL                    1.16    scale/generic/100sigma
  mse_rows, mse_cols, points,                                         nllcoord      value / dc / dL       0.87 / 0.56 / 0.30
  elem (l2, l1, smooth_l1): all         0.00                          normal        value / dmu / dsg     0.28 / 0.44 / 1.55
                                                                      laplace       value / dmu / dsg     0.19 / 0.00 / 0.73
                                                                      diag_scale, gmm dx                  0.00
  K["poly"] = 5                                                       K["trans"] = 8 (the heads reach 3.57, tests/test_heads_rows_gpu.py)

(*) cancellation, in the yardstick as much as in the kernel: 1 - (q.t)^2 at an angle of 1e-4 is 2.5e-9, below one rounding of (q.t)^2, and
(1 - |q|)^2 of a float32 unit quaternion is the square of its rounding; E_ref itself is 1.0 and 23 there.  No ratio is above 8.

The exactly-zero rows found one thing: with the left-to-right quaternion product of hm::qmul, conj(q) * t at t == q kept an imaginary
residue of about 1e-8, so a prediction equal to its target had a non-zero geodesic distance and, under a sharp predicted scale (1e-3 rad),
a rotation-NLL gradient of 1e-2 where the float64 reference has exactly 0.  lm::rotation_delta now sums antisymmetric pairs without FMA
contraction (lm::qmul_conj_paired) and is exactly zero there.
"""
import numpy as np
import pytest
import torch

import head_loss_cases as C
from head_loss_cases import K, LOSS_OPS, SIZES, Guarded, assert_within, class_errors, oracle, zero_rows

pytestmark = pytest.mark.gpu


def _dev(inputs, gv):
    d = {k: torch.from_numpy(v).cuda() for k, v in inputs.items()}
    d["gv"] = torch.from_numpy(gv).cuda()
    return d


def _calls(op, n, d, out):
    """([forward (entry point, arguments)], [backward ...]); outputs "v" and "g:<input>" are allocated in `out`."""
    from trackertraincode._hip import ptr

    e, prm = op.entry, op.prm
    P = lambda k: ptr(d[k])
    fwd, bwd = f"ttk_{e}_fwd", f"ttk_{e}_bwd"
    if e in ("loss_rot", "loss_rot_geodesic"):
        return (fwd, (P("q"), P("t"), n, out("v", n))), (bwd, (P("q"), P("t"), P("gv"), n, out("g:q", 4 * n)))
    if e == "loss_rot6d":
        return (fwd, (P("m"), P("t"), n, out("v", n))), (bwd, (P("t"), P("gv"), n, out("g:m", 9 * n)))
    if e == "loss_ortho6d":
        return (fwd, (P("z"), n, out("v", n))), (bwd, (P("z"), P("gv"), n, out("g:z", 6 * n)))
    if e == "mat_to_quat":
        return (fwd, (P("m"), n, out("v", 4 * n))), (bwd, (P("m"), P("gv"), n, out("g:m", 9 * n)))
    if e == "loss_quatreg":
        return (fwd, (P("q"), n, out("v", n))), (bwd, (P("q"), P("gv"), n, out("g:q", 4 * n)))
    if e == "loss_mse_rows":
        D = prm["D"]
        return (fwd, (P("p"), P("t"), n, D, out("v", n))), (bwd, (P("p"), P("t"), P("gv"), n, D, out("g:p", n * D)))
    if e == "loss_mse_cols":
        a = (prm["Dt"], prm["c0"], prm["Dc"])
        return (fwd, (P("p"), P("t"), n, *a, out("v", n))), (bwd, (P("p"), P("t"), P("gv"), n, *a, out("g:p", n * prm["Dt"])))
    if e == "loss_points":
        a = (prm["dim"], C.CHIN, C.EYE)
        return (fwd, (P("p"), P("t"), n, *a, out("v", n))), (bwd, (P("p"), P("t"), P("gv"), n, *a, out("g:p", n * 204)))
    if e in ("loss_nllrot", "loss_nllcoord"):
        x = "q" if e == "loss_nllrot" else "c"
        w = 4 if e == "loss_nllrot" else 3
        return ((fwd, (P(x), P("t"), P("L"), n, out("v", n))),
                (bwd, (P(x), P("t"), P("L"), P("gv"), n, out("g:" + x, w * n), out("g:L", 9 * n))))
    if e in ("loss_normal", "loss_laplace"):
        a = (prm["per"], prm["points"], prm["dim"], C.CHIN, C.EYE)
        m = n * (204 if prm["points"] else prm["per"])
        return ((fwd, (P("mu"), P("sg"), P("x"), n, *a, out("v", n))),
                (bwd, (P("mu"), P("sg"), P("x"), P("gv"), n, *a, out("g:mu", m), out("g:sg", m))))
    if e == "loss_elem":
        a = (prm["D"], prm["kind"], prm["beta"])
        return ((fwd, (P("p"), P("t"), P("colw"), n, *a, out("v", n))),
                (bwd, (P("p"), P("t"), P("colw"), P("gv"), n, *a, out("g:p", n * prm["D"]))))
    if e == "diag_scale":
        return (fwd, (P("h"), out("v", n), n)), (bwd, (P("h"), P("gv"), out("g:h", n + 1), n))
    raise KeyError(e)


def _launch(op, n, d, batch=None):
    """One forward and one backward launch on fresh buffers (or appended to `batch` for ttk_loss_batch); returns the buffers."""
    from trackertraincode._hip import lib

    out = Guarded()
    for name, args in _calls(op, n, d, out):
        if batch is None:
            lib().call(name, *args)
        else:
            batch.append((name, args))
    return out


_REFS = {}


def _reference(op, n):
    """(cls, inputs, gv, float64 (out, grads), float32 (out, grads)) - computed once per (op, n), never modified."""
    key = (op.name, n)
    if key not in _REFS:
        cls, inp = op.make(n)
        o64, g64, gv = oracle(op, inp, torch.float64)
        o32, g32, _ = oracle(op, inp, torch.float32)
        assert np.isfinite(o64).all() and all(np.isfinite(g).all() for g in g64.values()), op.name
        _REFS[key] = (cls, inp, gv, (o64, g64), (o32, g32))
    return _REFS[key]


def _compare(op, n, out, report=None):
    cls, inp, gv, (o64, g64), (o32, g32) = _reference(op, n)
    skip = op.no_grad_rows(inp) if op.no_grad_rows else None
    items = [("value", out.get("v").cpu().numpy(), o64, o32, None)]
    for k in op.wrt:
        items.append(("d" + k, out.get("g:" + k).cpu().numpy(), g64[k], g32[k], skip))
    for what, got, r64, r32, sk in items:
        tag = f"{op.name} n={n} {what}"
        if op.entry == "diag_scale" and what == "dh":
            # gh[0] is a sum over all n elements: (n + 8) 2^-24 sum|terms| holds in any summation order
            h = inp["h"].astype(np.float64)
            elu1 = lambda x: np.where(x > 0, x + 1.0, np.exp(np.minimum(x, 0.0)))
            terms = np.abs(gv.astype(np.float64) * elu1(h[1:])).sum() * np.exp(min(h[0], 0.0))
            assert abs(got[0] - r64[0]) <= (n + 8) * C.EPS24 * terms, tag
            got, r64, r32 = got[1:], r64[1:], r32[1:]
        zr = zero_rows(r64, n)
        if sk is not None:
            zr &= ~sk
        g2 = np.asarray(got, np.float64).reshape(n, -1)
        assert not g2[zr].any(), f"{tag}: rows {np.flatnonzero(zr & g2.any(-1))[:8]} must be exactly zero"
        assert_within(class_errors(got, r64, cls, sk), class_errors(r32, r64, cls, sk), K[op.group], tag, report)


@pytest.mark.parametrize("op", LOSS_OPS, ids=repr)
def test_single_op_rows(op):
    for n in SIZES:
        cls, inp, gv, _, _ = _reference(op, n)
        d = _dev(inp, gv)
        a, b = _launch(op, n, d), _launch(op, n, d)
        torch.cuda.synchronize()
        for o in (a, b):
            o.check(f"{op.name} n={n}")
        for k in a.bufs:
            assert torch.equal(a.bufs[k][0][:a.bufs[k][1]], b.bufs[k][0][:b.bufs[k][1]]), f"{op.name} n={n}: {k} differs between two runs"
        _compare(op, n, a)


def _gmm_launch(g, x, gv, n, batch=None):
    from trackertraincode._hip import lib, ptr

    out = Guarded()
    post = out("post", n * g["K"], torch.float64)
    calls = [("ttk_loss_gmm_fwd", (ptr(x), ptr(g["ck"]), ptr(g["mu"]), ptr(g["sinv"]), g["K"], g["fudge"], n, out("v", n), post)),
             ("ttk_loss_gmm_bwd", (ptr(x), ptr(g["mu"]), ptr(g["sinv"]), post, g["K"], g["fudge"], ptr(gv), n, out("g:x", 50 * n)))]
    if batch is None:
        for name, args in calls:
            lib().call(name, *args)
    return out, calls


@pytest.fixture(scope="module")
def gmm():
    g = C.ShapeGmm64()
    return {"oracle": g, "K": g.K, "fudge": g.fudge, "ck": torch.from_numpy(g.ck).cuda(), "mu": torch.from_numpy(g.mu).cuda(),
            "sinv": torch.from_numpy(g.sinv).cuda()}


def _gmm_reference(gmm, n):
    t = C.gmm_rows().cycle(n)
    x64 = torch.from_numpy(t.a["x"]).double().requires_grad_(True)
    v64, post64 = gmm["oracle"](x64)
    gv = C.cotangent((n,))
    (v64 * torch.from_numpy(gv).double()).sum().backward()
    x32 = torch.from_numpy(t.a["x"]).requires_grad_(True)  # the oracle's own float32 path: float64 inside, float32 leaves
    (gmm["oracle"].g({"shapeparam": x32}, None) * torch.from_numpy(gv)).sum().backward()
    return t, gv, v64.detach().numpy(), post64.detach().numpy(), x64.grad.numpy(), x32.grad.double().numpy()


def test_gmm_rows(gmm):
    """Values and posteriors are float64 on the device: one fp32 rounding of the value, 1e-12 on the posteriors."""
    for n in SIZES:
        t, gv, v64, post64, g64, g32 = _gmm_reference(gmm, n)
        x, gvd = torch.from_numpy(t.a["x"]).cuda(), torch.from_numpy(gv).cuda()
        (a, _), (b, _) = _gmm_launch(gmm, x, gvd, n), _gmm_launch(gmm, x, gvd, n)
        torch.cuda.synchronize()
        for o in (a, b):
            o.check(f"gmm n={n}")
        for k in a.bufs:
            assert torch.equal(a.get(k), b.get(k)), f"gmm n={n}: {k} differs between two runs"
        np.testing.assert_allclose(a.get("post").cpu().numpy().reshape(n, -1), post64, rtol=1e-12, atol=0, err_msg=f"posteriors n={n}")
        np.testing.assert_allclose(a.get("v").cpu().numpy(), v64, rtol=2.0 ** -23, atol=0, err_msg=f"value n={n}")
        assert_within(class_errors(a.get("g:x").cpu().numpy(), g64, t.cls), class_errors(g32, g64, t.cls), K["trans"], f"gmm n={n} dx")


def test_batched_launch_is_bitwise_the_single_ops(gmm):
    """One ttk_loss_batch launch per 32 ops, item counts 1, 65, 257 and 1000 mixed (the grid is sized by the largest op, the small ones
    exit early), every TTK_OP_* kind forward and backward: bitwise the single-op launches, guard bands intact."""
    from trackertraincode._hip import LOSS_BATCH_OPS, lib

    by_entry = {}
    for op in LOSS_OPS:
        by_entry.setdefault(op.entry, op)
    ns = (1, 65, 257, 1000)
    batch, singles, batched = [], [], []
    kinds = set()
    for i, (entry, op) in enumerate(sorted((e, o) for e, o in by_entry.items() if f"ttk_{e}_fwd" in LOSS_BATCH_OPS)):
        n = ns[i % len(ns)]
        cls, inp, gv, _, _ = _reference(op, n)
        d = _dev(inp, gv)
        singles.append((op, n, _launch(op, n, d), d))
        batched.append(_launch(op, n, d, batch))
    n = 257
    t, gv = C.gmm_rows().cycle(n), C.cotangent((n,))
    x, gvd = torch.from_numpy(t.a["x"]).cuda(), torch.from_numpy(gv).cuda()
    g_single, _ = _gmm_launch(gmm, x, gvd, n)
    g_batched, calls = _gmm_launch(gmm, x, gvd, n, batch)
    # the GMM backward reads the posteriors its forward writes: forward ops in a first launch, backward ops in a second
    fwd_ops = [c for c in batch if c[0].endswith("_fwd")] + [calls[0]]
    bwd_ops = [c for c in batch if c[0].endswith("_bwd")] + [calls[1]]
    for ops in (fwd_ops, bwd_ops):
        kinds |= {LOSS_BATCH_OPS[name][0] for name, _ in ops}
        assert len(ops) <= 32
        lib().loss_batch(ops)
    assert kinds == set(range(len(LOSS_BATCH_OPS))) and len(LOSS_BATCH_OPS) == 22
    assert {n for _, n, _, _ in singles} == set(ns)
    torch.cuda.synchronize()
    for (op, n, s, _), b in zip(singles, batched):
        b.check(f"batched {op.name} n={n}")
        for k in s.bufs:
            assert torch.equal(s.get(k), b.get(k)), f"batched {op.name} n={n}: {k} differs from the single-op launch"
    g_batched.check("batched gmm")
    for k in g_single.bufs:
        assert torch.equal(g_single.get(k), g_batched.get(k)), f"batched gmm: {k}"
