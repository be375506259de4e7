"""The case table of the per-row GPU tests (tests/head_loss_cases.py) checked without a GPU: (a) the float64 oracle is finite, value
and gradient, on every row the GPU tests compare; (b) the rows left out of a gradient comparison are exactly the crafted four-way ties
of from_matrix; (c) the math headers compiled for the host (tests/host_math/shim.cpp) agree with the oracle on every class at the
tolerances of tests/test_host_math.py.  A later GPU failure on a class that passes here is device code, not formula."""
import ctypes

import numpy as np
import pytest
import torch

import head_loss_cases as C
from oracle import refmodel as R
from test_host_math import P, hm  # noqa: F401  (hm: the fixture that compiles the shim)

VAL = dict(rtol=2e-5, atol=2e-6)
GRAD = dict(rtol=3e-4, atol=3e-5)


@pytest.mark.parametrize("op", C.LOSS_OPS, ids=repr)
def test_oracle_is_finite_and_only_ties_are_left_out(op):
    n = 1000  # every table fits, every class appears
    cls, inp = op.make(n)
    o64, g64, _ = C.oracle(op, inp, torch.float64)
    o32, g32, _ = C.oracle(op, inp, torch.float32)
    for a in (o64, o32, *g64.values(), *g32.values()):
        assert np.isfinite(a).all(), op.name
    if op.no_grad_rows is None:
        assert op.entry != "mat_to_quat"
    else:
        left_out = op.no_grad_rows(inp)
        np.testing.assert_array_equal(left_out, cls == "four_way_tie")
        assert 0 < left_out.sum() == (np.arange(n) % 64 >= 48).sum()
    if "m" in inp:  # all four from_matrix solutions occur among the generic rows
        picks = np.argmax(C.from_matrix_args(inp["m"][cls == "generic"]), -1)
        assert set(picks.tolist()) == {0, 1, 2, 3}


def test_gmm_rows_are_finite():
    g = C.ShapeGmm64()
    t = C.gmm_rows()
    x = torch.from_numpy(t.a["x"]).double().requires_grad_(True)
    v, post = g(x)
    v.sum().backward()
    assert torch.isfinite(v).all() and torch.isfinite(x.grad).all() and torch.isfinite(post).all()
    one_hot = post.detach()[torch.from_numpy(t.cls == "magnitude_20")].amax(-1)
    assert float(one_hot.min()) > 1 - 1e-9


@pytest.mark.parametrize("cfg", C.HEAD_CONFIGS, ids=str)
def test_head_edge_rows_are_finite(cfg):
    rng = np.random.default_rng(1)
    cls, z = C.head_edge_rows(cfg)
    B = len(cls)
    Prow, Pkrow = (rng.standard_normal((B, 4)) * 0.3).astype(np.float32), (rng.standard_normal((B, 4)) * 0.3).astype(np.float32)
    ups = {k: rng.standard_normal((B, w)).astype(np.float32) for k, (_, w) in C.head_outputs(cfg).items()}
    for dtype in (torch.float64, torch.float32):
        out, dz, dprow = C.heads_oracle(cfg, z, Prow, Pkrow, ups, dtype)
        assert all(np.isfinite(v).all() for v in out.values()) and np.isfinite(dz).all() and np.isfinite(dprow).all()
    unc, pt, rot6d, use_offset = cfg
    if rot6d and not use_offset:
        fb = np.isin(np.array([c.split("/")[0] for c in cls]), C.FALLBACK_6D_CLASSES)
        assert fb.sum() == 64 and (out["rot"][fb] == np.eye(3).reshape(-1)).all() and not (out["rot"][~fb] == np.eye(3).reshape(-1)).all(-1).any()


# ---- (c) the host-compiled headers on every class ------------------------------------------------------------------------------------
def _z(n, *w):
    return np.zeros((n,) + w, np.float32)


def _shim(hm, op, n, inp, gv):
    """(value, {input: gradient}) of the host-compiled math for the ops that tests/host_math/shim.cpp exposes per row."""
    e = op.entry
    v = _z(n)
    if e in ("loss_rot", "loss_rot_geodesic"):
        g = _z(n, 4)
        getattr(hm, "lm_rot" if e == "loss_rot" else "lm_rot_geodesic")(n, P(inp["q"]), P(inp["t"]), P(gv), P(v), P(g))
        return v, {"q": g}
    if e == "loss_quatreg":
        g = _z(n, 4)
        hm.lm_quatreg(n, P(inp["q"]), P(gv), P(v), P(g))
        return v, {"q": g}
    if e == "loss_nllrot":
        g, gL = _z(n, 4), _z(n, 3, 3)
        hm.lm_nllrot(n, P(inp["q"]), P(inp["t"]), P(inp["L"]), P(gv), P(v), P(g), P(gL))
        return v, {"q": g, "L": gL}
    if e == "loss_nllcoord":
        g, gL = _z(n, 3), _z(n, 3, 3)
        hm.lm_nllcoord(n, P(inp["c"]), P(inp["t"]), P(inp["L"]), P(gv), P(v), P(g), P(gL))
        return v, {"c": g, "L": gL}
    if e == "loss_rot6d":
        g = _z(n, 3, 3)
        hm.lm_rot6d(n, P(inp["m"]), P(inp["t"]), P(gv), P(v), P(g))
        return v, {"m": g}
    if e == "loss_ortho6d":
        g = _z(n, 6)
        hm.lm_ortho6d(n, P(inp["z"]), P(gv), P(v), P(g))
        return v, {"z": g}
    if e == "mat_to_quat":
        q, g = _z(n, 4), _z(n, 3, 3)
        hm.lm_from_matrix(n, P(inp["m"]), P(gv), P(q), P(g))
        return q, {"m": g}
    return None


ROW_OPS = [op for op in C.LOSS_OPS if op.entry in ("loss_rot", "loss_rot_geodesic", "loss_quatreg", "loss_nllrot", "loss_nllcoord", "loss_rot6d",
                                                   "loss_ortho6d", "mat_to_quat")]


@pytest.mark.parametrize("op", ROW_OPS, ids=repr)
def test_host_math_agrees_per_row(hm, op):
    n = 1000
    cls, inp = op.make(n)
    o64, g64, gv = C.oracle(op, inp, torch.float64)
    v, g = _shim(hm, op, n, inp, gv)
    for c in dict.fromkeys(cls.tolist()):
        rows = cls == c
        np.testing.assert_allclose(v[rows], o64[rows], **VAL, err_msg=f"{op.name} {c} value")
        if c == "four_way_tie" and op.no_grad_rows is not None:
            continue
        for k in op.wrt:
            np.testing.assert_allclose(g[k][rows], g64[k][rows], **GRAD, err_msg=f"{op.name} {c} d{k}")


@pytest.mark.parametrize("kind,beta", [("l2", 1.0), ("l1", 1.0), ("smooth_l1", 1.0), ("smooth_l1", 0.1)])
def test_host_math_agrees_on_element_classes(hm, kind, beta):
    t = C.elem_rows(96, 8, beta, seed=1)
    p, tt = t.a["p"].reshape(-1), t.a["t"].reshape(-1)
    pt = torch.from_numpy(p).double().requires_grad_(True)
    ref = R.elem_distance(kind, pt, torch.from_numpy(tt).double(), beta)
    ref.sum().backward()
    v, d = _z(p.size), _z(p.size)
    hm.lm_elem.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float] + [ctypes.c_void_p] * 4
    hm.lm_elem(p.size, {"l2": 0, "l1": 1, "smooth_l1": 2}[kind], beta, P(p), P(tt), P(v), P(d))
    np.testing.assert_allclose(v, ref.detach().numpy(), **VAL)
    np.testing.assert_allclose(d, pt.grad.numpy(), **GRAD)
    zero = np.repeat(t.cls == "zero", 8)
    assert not v[zero].any() and not d[zero].any()


@pytest.mark.parametrize("dist", ["gaussian", "laplace"])
def test_host_math_agrees_on_distribution_classes(hm, dist):
    t = C.dist_rows(64, (8,), seed=2)
    mu, sg, x = (t.a[k].reshape(-1) for k in ("mu", "sg", "x"))
    mt, st = torch.from_numpy(mu).double().requires_grad_(True), torch.from_numpy(sg).double().requires_grad_(True)
    ref = -R._dist_logprob(dist)(torch.from_numpy(x).double(), mt, st)
    ref.sum().backward()
    v, gmu, gsg = _z(mu.size), _z(mu.size), _z(mu.size)
    getattr(hm, "lm_normal" if dist == "gaussian" else "lm_laplace")(mu.size, P(mu), P(sg), P(x), P(v), P(gmu), P(gsg))
    np.testing.assert_allclose(v, ref.detach().numpy(), **VAL)
    np.testing.assert_allclose(gmu, mt.grad.numpy(), **GRAD)
    np.testing.assert_allclose(gsg, st.grad.numpy(), **GRAD)


def test_host_math_agrees_on_gmm_classes(hm):
    g = C.ShapeGmm64()
    t = C.gmm_rows()
    n = len(t)
    v64, post64 = g(torch.from_numpy(t.a["x"]))
    v, post = _z(n), np.zeros((n, g.K), np.float64)
    hm.lm_gmm.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    hm.lm_gmm(n, P(t.a["x"]), P(g.ck), P(g.mu), P(g.sinv), g.K, g.fudge, P(v), P(post))
    np.testing.assert_allclose(v, v64.numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(post, post64.numpy(), rtol=1e-9, atol=1e-300)


@pytest.mark.parametrize("cfg", C.HEAD_CONFIGS, ids=str)
def test_host_math_agrees_on_head_edge_rows(hm, cfg):
    from oracle.synth import synthetic_keypoint_buffers

    unc, pt, rot6d, use_offset = cfg
    rng = np.random.default_rng(2)
    cls, z = C.head_edge_rows(cfg)
    n, NZ = z.shape
    ids = rng.integers(0, 8, n).astype(np.int32)
    Pm, Pk = (rng.standard_normal((8, 4)) * 0.3).astype(np.float32), (rng.standard_normal((8, 4)) * 0.3).astype(np.float32)
    names = C.head_outputs(cfg)
    ups = {k: rng.standard_normal((n, w)).astype(np.float32) for k, (_, w) in names.items()}
    out, dz, dprow = C.heads_oracle(cfg, z, Pm[ids], Pk[ids], ups, torch.float64)
    kp, ke = synthetic_keypoint_buffers()
    wrot = 9 if rot6d else 4
    o = {"roi": _z(n, 4), "coord": _z(n, 3), "rot": _z(n, wrot), "qu": _z(n, 4), "Lc": _z(n, 9), "Lr": _z(n, 9), "pts": _z(n, 204)}
    up = lambda k, w: ups[k] if k in ups else _z(n, w)
    gz, gP, gPk = _z(n, NZ), _z(8, 4), _z(8, 4)
    if rot6d:
        hm.hm_heads6d_fwd(n, NZ, P(z), P(ids), P(Pm), P(Pk), P(kp), P(ke), unc, pt, use_offset, P(o["roi"]), P(o["coord"]), P(o["rot"]), P(o["Lc"]),
                          P(o["Lr"]), P(o["pts"]))
        hm.hm_heads6d_bwd(n, NZ, P(z), P(ids), P(Pm), P(Pk), P(kp), P(ke), unc, pt, use_offset, P(ups["roi"]), P(ups["coord"]), P(ups["rot"]),
                          P(ups["qu"]), P(up("Lc", 9)), P(up("Lr", 9)), P(up("pts", 204)), P(up("shp", 50)), P(gz), P(gP), P(gPk))
    else:
        hm.hm_heads_fwd(n, NZ, P(z), P(ids), P(Pm), P(Pk), P(kp), P(ke), unc, pt, use_offset, P(o["roi"]), P(o["coord"]), P(o["rot"]), P(o["qu"]),
                        P(o["Lc"]), P(o["Lr"]), P(o["pts"]))
        hm.hm_heads_bwd(n, NZ, P(z), P(ids), P(Pm), P(Pk), P(kp), P(ke), unc, pt, use_offset, P(ups["roi"]), P(ups["coord"]), P(ups["rot"]),
                        P(ups["qu"]), P(up("Lc", 9)), P(up("Lr", 9)), P(up("pts", 204)), P(up("shp", 50)), P(gz), P(gP), P(gPk))
    for k in names:
        if k == "shp" or (k == "qu" and rot6d):
            continue
        np.testing.assert_allclose(o[k], out[k], rtol=2e-5, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(gz, dz, rtol=2e-4, atol=3e-5 if rot6d else 2e-5)
    if use_offset:
        onehot = (ids[:, None] == np.arange(8)[None, :]).astype(np.float64)
        np.testing.assert_allclose(gP, onehot.T @ dprow[:, :4], rtol=2e-4, atol=3e-5 if rot6d else 2e-5)
        if pt:
            np.testing.assert_allclose(gPk, onehot.T @ dprow[:, 4:], rtol=2e-4, atol=3e-5 if rot6d else 2e-5)
    if rot6d:
        fb = np.isin(np.array([c.split("/")[0] for c in cls]), C.FALLBACK_6D_CLASSES)
        np.testing.assert_array_equal(gz[fb, 7:13], ups["qu"][fb])  # no gradient through the identity fallback
        if not use_offset:
            assert (o["rot"][fb] == np.eye(3, dtype=np.float32).reshape(-1)).all()
