"""The flat training step on the MI355X: ttk_loss_batch_rows / ttk_row_weights row by row, train.flat_training_step against the reference
goldens and against the per-Tag eager step on splits the goldens do not have, ONE captured graph for a split that changes every step
(GraphedTrainStep(layout="flat")), and fit / the train script end to end.  Host side: tests/test_flat_step.py.

Row criterion of the kernel test: the one of tests/test_loss_rows_gpu.py for live rows (E_hip <= K * E_ref + 4 * 2^-24 against float64,
K["poly"] = 5, K["trans"] = 8, measured and recorded there - the bodies are the same device functions), exactly 0.0 for dead rows."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import head_loss_cases as C
from head_loss_cases import K, LOSS_OPS, Guarded, assert_within, class_errors, oracle
from oracle import refmodel as R
from oracle.synth import digest_close, make_inputs, make_labels, make_state
from util import GOLDEN, REPO, build_net, load_golden, make_batches, script_args, train_script

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_TOL = 1.0e-3  # tests/test_model_gpu.py
NAN = float("nan")
CODES = (1, 7, 11)  # POSE_WITH_LANDMARKS, ONLY_POSE, POSE_WITH_LMKS_NO_SHAPE_PARAMS
SETS = [1 << 1, (1 << 7) | (1 << 11), (1 << 1) | (1 << 11), 1 << 7, (1 << 1) | (1 << 7) | (1 << 11)]
PER_ROW = {"q", "t", "m", "z", "L", "c", "p", "mu", "sg", "x"}  # inputs with one row per sample (colw and the GMM tables are shared)


# =====================================================================================================================================
# 1. the kernels, row by row
# =====================================================================================================================================
def _batch_ops():
    """Every LOSS_OPS case whose entry point is an op kind of ttk_loss_batch (the GMM is added by the test: its tables are not a LOSS_OPS case)."""
    from trackertraincode._hip import LOSS_BATCH_OPS

    return [op for op in LOSS_OPS if f"ttk_{op.entry}_fwd" in LOSS_BATCH_OPS]


_REFS = {}


def _live(tag_set, codes):
    """Row liveness as include/ttk.h defines it: the row's code is in 0..31 and its bit is set."""
    return np.array([0 <= int(c) < 32 and bool((tag_set >> int(c)) & 1) for c in codes], bool)


def _reference(op, n):
    """(cls, inputs, gv, float64 (out, grads), float32 (out, grads)) on finite inputs - once per (op, n), never modified."""
    if (op.name, n) not in _REFS:
        cls, inp = op.make(n)
        o64, g64, gv = oracle(op, inp, torch.float64)
        o32, g32, _ = oracle(op, inp, torch.float32)
        _REFS[(op.name, n)] = (cls, inp, gv, (o64, g64), (o32, g32))
    return _REFS[(op.name, n)]


def _poisoned(arrays, dead):
    """Device copies of per-row inputs with the rows in `dead` NaN: a dead row's inputs - its target above all - must never be read."""
    out = {}
    for k, v in arrays.items():
        v = v.copy()
        if k in PER_ROW or k == "gv":
            v[dead] = np.nan
        out[k] = torch.from_numpy(v).cuda()
    return out


@pytest.fixture(scope="module")
def gmm():
    g = C.ShapeGmm64()
    return {"oracle": g, "K": g.K, "fudge": g.fudge, "ck": torch.from_numpy(g.ck).cuda(), "mu": torch.from_numpy(g.mu).cuda(),
            "sinv": torch.from_numpy(g.sinv).cuda()}


def _gmm_reference(gmm, n):
    if ("gmm", n) not in _REFS:
        t = C.gmm_rows().cycle(n)
        x64 = torch.from_numpy(t.a["x"]).double().requires_grad_(True)
        v64, _ = gmm["oracle"](x64)
        gv = C.cotangent((n,))
        (v64 * torch.from_numpy(gv).double()).sum().backward()
        x32 = torch.from_numpy(t.a["x"]).requires_grad_(True)
        v32 = gmm["oracle"].g({"shapeparam": x32}, None)
        (v32 * torch.from_numpy(gv)).sum().backward()
        _REFS[("gmm", n)] = (t, gv, v64.detach().numpy(), x64.grad.numpy(), v32.detach().double().numpy(), x32.grad.double().numpy())
    return _REFS[("gmm", n)]


def _launch_all(n, codes, sets_of, gmm, rows=True, null_codes=False):
    """All op kinds forward in ONE launch and backward in a second one (the GMM backward reads what its forward wrote) on fresh
    NaN-filled guarded buffers.  rows=False: through ttk_loss_batch.  Returns [(op or "gmm", set, buffers)]."""
    from test_loss_rows_gpu import _calls
    from trackertraincode._hip import lib, ptr

    L = lib()
    tag = None if codes is None else torch.from_numpy(codes.astype(np.int32)).cuda()
    fwd, bwd, sets, outs, keep = [], [], [], [], []
    ops = _batch_ops()
    for i, op in enumerate(ops):
        cls, inp, gv, _, _ = _reference(op, n)
        s = sets_of(i)
        dead = np.zeros(n, bool) if codes is None else ~_live(s, codes)
        d = _poisoned(dict(inp, gv=gv), dead)
        out = Guarded()
        f, b = _calls(op, n, d, out)
        fwd.append(f), bwd.append(b), sets.append(s), outs.append((op, s, out)), keep.append(d)
    t, gv = _gmm_reference(gmm, n)[:2]
    s = sets_of(len(ops))
    dead = np.zeros(n, bool) if codes is None else ~_live(s, codes)
    d = _poisoned({"x": t.a["x"], "gv": gv}, dead)
    out = Guarded()
    post = out("post", n * gmm["K"], torch.float64)
    fwd.append(("ttk_loss_gmm_fwd", (ptr(d["x"]), ptr(gmm["ck"]), ptr(gmm["mu"]), ptr(gmm["sinv"]), gmm["K"], gmm["fudge"], n, out("v", n), post)))
    bwd.append(("ttk_loss_gmm_bwd", (ptr(d["x"]), ptr(gmm["mu"]), ptr(gmm["sinv"]), post, gmm["K"], gmm["fudge"], ptr(d["gv"]), n, out("g:x", 50 * n))))
    sets.append(s), outs.append(("gmm", s, out)), keep.append(d)
    assert len(fwd) <= 32 and {L.pack_loss_ops([c])[0].kind for c in fwd + bwd} == set(range(22)), "every TTK_OP_* kind"
    for chunk in (fwd, bwd):
        if not rows:
            L.loss_batch(chunk)
        elif null_codes:  # the entry point itself with tag_code == NULL
            L.call("ttk_loss_batch_rows", len(chunk), L.pack_loss_ops(chunk), (ctypes.c_uint * len(chunk))(*sets), None)
        else:
            L.loss_batch(chunk, sets, tag)
    torch.cuda.synchronize()
    return outs


def _same(a, b, what):
    for (op, _, x), (_, _, y) in zip(a, b):
        for k in x.bufs:
            assert torch.equal(x.bufs[k][0].view(torch.uint8), y.bufs[k][0].view(torch.uint8)), f"{what}: {op} {k} differs bitwise (guard band included)"


def _check_rows(n, codes, outs, gmm):
    for op, s, out in outs:
        name = op if isinstance(op, str) else op.name
        out.check(f"{name} n={n}")  # nothing NaN, guard band intact
        live = _live(s, codes)
        if name == "gmm":
            t, gv, v64, g64, v32, g32 = _gmm_reference(gmm, n)
            cls, group, skip_g = t.cls, "trans", None
            items = [("value", "v", v64, v32), ("dx", "g:x", g64, g32)]
            assert not out.get("post").cpu().numpy().reshape(n, -1)[~live].any()
        else:
            cls, inp, gv, (o64, g64), (o32, g32) = _reference(op, n)
            group, skip_g = op.group, (op.no_grad_rows(inp) if op.no_grad_rows else None)
            items = [("value", "v", o64, o32)] + [("d" + k, "g:" + k, g64[k], g32[k]) for k in op.wrt]
        for what, key, r64, r32 in items:
            got = out.get(key).cpu().numpy().astype(np.float64).reshape(n, -1)
            assert (got[~live] == 0.0).all(), f"{name} n={n} {what}: dead rows must be exactly 0.0"
            skip = ~live if (what == "value" or skip_g is None) else (~live | skip_g)
            if live.any():
                assert_within(class_errors(got, r64, cls, skip), class_errors(r32, r64, cls, skip), K[group], f"{name} n={n} {what}")


@pytest.mark.parametrize("n", [1, 7, 65])
def test_loss_batch_rows_live_and_dead_rows(n, gmm):
    rng = np.random.default_rng(900 + n)
    codes = rng.choice(CODES, n)
    sets_of = lambda i: SETS[i % len(SETS)]
    a, b = _launch_all(n, codes, sets_of, gmm), _launch_all(n, codes, sets_of, gmm)
    _same(a, b, f"n={n}: two runs")
    _check_rows(n, codes, a, gmm)
    lives = np.concatenate([_live(s, codes) for _, s, _ in a])
    assert lives.any() and not lives.all(), "the case must hold live and dead rows"


@pytest.mark.parametrize("n", [7, 65])
def test_loss_batch_rows_all_dead_all_live_and_null(n, gmm):
    codes = np.random.default_rng(901 + n).choice(CODES, n)
    every = (1 << 1) | (1 << 7) | (1 << 11)
    dead = _launch_all(n, codes, lambda i: (1 << 3) | (1 << 31), gmm)  # sets that hold none of the codes
    _check_rows(n, codes, dead, gmm)
    plain = _launch_all(n, None, lambda i: 0, gmm, rows=False)  # ttk_loss_batch on the same ops
    live = _launch_all(n, codes, lambda i: every, gmm)
    _check_rows(n, codes, live, gmm)
    _same(live, plain, f"n={n}: all rows live against ttk_loss_batch")
    null = _launch_all(n, None, lambda i: 0, gmm, null_codes=True)  # tag_code == NULL: the Tag sets are not looked at
    _same(null, plain, f"n={n}: tag_code NULL against ttk_loss_batch")
    # a code outside 0..31 is in no set
    wild = _launch_all(n, np.full(n, 32), lambda i: 0xFFFFFFFF, gmm)
    _same(wild, _launch_all(n, np.full(n, -1), lambda i: 0xFFFFFFFF, gmm), "codes 32 and -1")
    assert all(not o.get(k).cpu().numpy().any() for _, _, o in wild for k in o.bufs)


@pytest.mark.parametrize("with_dw", [False, True])
def test_row_weights_exact(with_dw):
    """One fp32 product per element: exact against numpy."""
    from trackertraincode.neuralnets import _hipops

    rng = np.random.default_rng(5)
    Kt, n = 3, 7
    wtable = rng.uniform(-2, 2, (Kt, 32)).astype(np.float32)
    codes = np.array([1, 7, 11, 7, 1, 31, 0], np.int32)
    dw = rng.uniform(0.5, 2.0, n).astype(np.float32)
    rw = _hipops.row_weights(torch.from_numpy(wtable).cuda(), torch.from_numpy(codes).cuda(), torch.from_numpy(dw).cuda() if with_dw else None, Kt)
    ref = wtable[:, codes] * (dw[None, :] if with_dw else np.float32(1.0))
    assert rw.shape == (Kt, n) and rw.dtype == torch.float32
    np.testing.assert_array_equal(rw.cpu().numpy(), ref.astype(np.float32))
    out = Guarded()  # through the C-ABI on a guarded buffer, with a code outside 0..31
    from trackertraincode._hip import lib, ptr
    bad, wt = torch.tensor([1, 40, -2, 7, 11, 7, 1], dtype=torch.int32, device=DEV), torch.from_numpy(wtable).cuda()
    lib().call("ttk_row_weights", ptr(wt), ptr(bad), None, Kt, n, out("rw", Kt * n))
    torch.cuda.synchronize()
    out.check("row_weights")
    ref = wtable[:, np.array([1, 0, 0, 7, 11, 7, 1])]
    ref[:, 1:3] = 0.0
    np.testing.assert_array_equal(out.np("rw", Kt, n), ref)


# =====================================================================================================================================
# 2. the flat step against the reference goldens
# =====================================================================================================================================
@pytest.mark.parametrize("cfg", ["full", "default", "rot6d"])
def test_flat_step_matches_reference_golden(cfg):
    """The checks and tolerances of test_model_gpu.test_train_step_matches_reference_golden on train.flat_training_step, with NaN in every
    label row a sub-batch does not have."""
    import trackertraincode.train as train

    d, meta = load_golden(f"model_{cfg}.npz")
    S = train_script()
    for epoch in (0, 20, 150):
        net = build_net(meta, DEV).train()
        crit, _ = S.setup_losses(script_args(meta["flags"]), net)
        flat = train.flatten_batches(make_batches(meta, DEV), fill=NAN)
        out = train.flat_training_step(net, flat, epoch, crit)
        names = [k.split("/")[3] for k in d.files if k.startswith(f"train/e{epoch}/loss/") and k.endswith("/values")]
        assert list(out["mt_losses"].keys()) == names and list(out["mt_rows"].keys()) == names
        for n in names:
            v, rows = out["mt_losses"][n], out["mt_rows"][n]
            assert v.shape == (meta["B"],) and rows.shape == (meta["B"],) and rows.dtype == torch.bool
            assert not bool(v.isnan().any()) and not bool(v[~rows].any()), n
            np.testing.assert_allclose(v[rows].cpu().numpy(), d[f"train/e{epoch}/loss/{n}/values"], rtol=LOSS_TOL, atol=LOSS_TOL, err_msg=n)
        assert abs(out["loss"].item() - float(d[f"train/e{epoch}/loss_sum"])) < LOSS_TOL
    out["loss"].backward()
    torch.cuda.synchronize()
    params = dict(net.named_parameters())
    bad = []
    for k in [k for k in d.files if k.startswith("train/grad/")]:
        g = params[k[len("train/grad/"):]].grad
        g = torch.zeros_like(params[k[len("train/grad/"):]]) if g is None else g
        ok, msg = digest_close(d[k], g.cpu().numpy(), rtol=2e-2, atol=1e-6, rtol_samples=1e-1)
        if not ok:
            bad.append((k, msg))
    assert not bad, bad[:5]
    sd = net.state_dict()
    for k in [k for k in d.files if k.startswith("train/after/")]:
        ok, msg = digest_close(d[k], sd[k[len("train/after/"):]].cpu().numpy(), rtol=2e-4, atol=1e-6)
        assert ok, f"{k}: {msg}"


def test_flat_step_refuses_what_it_cannot_flatten():
    import trackertraincode.train as train
    from trackertraincode.neuralnets import losses
    from trackertraincode.pipelines import Tag

    _, meta = load_golden("model_full.npz")
    net = build_net(meta, DEV).train()
    flat = train.flatten_batches(make_batches(meta, DEV))
    rot = losses.QuatPoseLoss("approx_distance")
    scaled = {Tag.POSE_WITH_LANDMARKS: train.CriterionGroup([train.Criterion("twice_rot", lambda p, b: 2.0 * rot(p, b), 1.0)]),
              Tag.ONLY_POSE: train.CriterionGroup([train.Criterion("rot", rot, 1.0)])}
    with pytest.raises(NotImplementedError, match="twice_rot"):  # post-processes a deferred value: the unbatched path of default_compute_loss
        train.flat_training_step(net, flat, 0, scaled)
    geo = {Tag.POSE_WITH_LANDMARKS: train.CriterionGroup([train.Criterion("geo", losses.QuatPoseLoss("smooth_geodesic"), 1.0)])}
    with pytest.raises(NotImplementedError, match="rot_geodesic"):  # a loss kind outside ttk_loss_batch: no row-liveness form
        train.flat_training_step(net, flat, 0, geo)


# =====================================================================================================================================
# 3. flat against the per-Tag eager step on other splits
# =====================================================================================================================================
SPLITS = (5, 2, 7, 8, 0)


def _split_batches(meta, k, device, flip=False):
    """The eight rows of make_labels / make_inputs: rows [:k] POSE_WITH_LANDMARKS, rows [k:] ONLY_POSE, with dataset weights; an empty
    sub-batch is left out."""
    from trackertraincode.datasets.batch import Batch, Metadata
    from trackertraincode.pipelines import Tag

    B = meta["B"]
    image, ids = make_inputs(B, seed=meta["input_seed"])
    if flip:
        image = image[..., ::-1]
    lab = make_labels(B, seed=meta["input_seed"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    out = []
    for tag, rows, fields in ((Tag.POSE_WITH_LANDMARKS, slice(0, k), ("pose", "coord", "roi", "pt3d_68", "shapeparam", "dataset_weight")),
                              (Tag.ONLY_POSE, slice(k, B), ("pose", "coord", "roi", "dataset_weight"))):
        n = len(range(B)[rows])
        if n:
            out.append(Batch(Metadata(129, batchsize=n, tag=tag), dict(image=t(image[rows]), coord_convention_id=t(ids[rows]), **{f: t(lab[f][rows]) for f in fields})))
    return out


@pytest.fixture(scope="module")
def oracle_grads():
    """{k: {parameter: float64 gradient}} of the oracle step (oracle.refmodel, epoch 150) for every split in SPLITS: ONE float64 forward,
    one backward per split's loss."""
    d, meta = load_golden("model_full.npz")
    shapes = {k: tuple(v) for k, v in meta["shapes"].items()}
    B = meta["B"]
    image, ids = make_inputs(B, seed=meta["input_seed"])
    lab = make_labels(B, seed=meta["input_seed"])
    fl = meta["flags"]
    ocrit, _ = R.setup_losses(with_pointhead=fl["with_pointhead"], with_nll_loss=fl["with_nll_loss"], rampup_nll_losses=fl["rampup_nll_losses"],
                              epochs=200, gmm=R.ShapeGmm(os.path.join(GOLDEN, "shapeparams_gmm.npz")))
    st = {}
    for k, v in make_state(shapes, 0).items():
        t = torch.from_numpy(np.array(v))
        t = t.double() if t.is_floating_point() else t
        st[k] = t.requires_grad_(True) if not R.is_buffer(k) else t
    out, _ = R.network_forward(st, torch.from_numpy(image).double(), torch.from_numpy(ids), meta["config"], True)
    t64 = lambda a: torch.from_numpy(a.copy()).double()
    grads = {}
    for k in SPLITS:
        bs = []
        if k:
            bs.append(dict({f: t64(lab[f][:k]) for f in ("pose", "coord", "roi", "pt3d_68", "shapeparam", "dataset_weight")}, tag="POSE_WITH_LANDMARKS", n=k))
        if B - k:
            bs.append(dict({f: t64(lab[f][k:]) for f in ("pose", "coord", "roi", "dataset_weight")}, tag="ONLY_POSE", n=B - k))
        loss, _ = R.compute_loss(out, bs, 150, ocrit)
        params = {n: p for n, p in st.items() if not R.is_buffer(n)}
        gs = torch.autograd.grad(loss, list(params.values()), retain_graph=True, allow_unused=True)
        grads[k] = {n: (None if g is None else g.detach().clone()) for n, g in zip(params, gs)}
    return grads


@pytest.mark.parametrize("k", SPLITS)
def test_flat_step_matches_per_tag_eager(k, oracle_grads, monkeypatch):
    import trackertraincode.backbones.mobilenet_v1 as MB
    import trackertraincode.train as train

    monkeypatch.setattr(MB, "_DETERMINISTIC", True)
    _, meta = load_golden("model_full.npz")
    B = meta["B"]
    S = train_script()

    def run(flat):
        net = build_net(meta, DEV).train()
        crit, _ = S.setup_losses(script_args(meta["flags"]), net)
        seen = {}
        net.register_forward_hook(lambda m, a, o: seen.update(o))
        batches = _split_batches(meta, k, DEV)
        if flat:
            out = train.flat_training_step(net, train.flatten_batches(batches, fill=NAN), 150, crit)
            loss, abssum = out["loss"], None
        else:
            preds = net(torch.concat([b["image"] for b in batches]), torch.concat([b["coord_convention_id"] for b in batches]))
            loss, lossvals = train.default_compute_loss(preds, batches, 150, crit)
            abssum = sum(float((v.val.double() * train._as_weight_tensor(v.weight).double()).abs().sum()) for vs in lossvals for v in vs) / B
        loss.backward()
        torch.cuda.synchronize()
        val = lambda v: (v.value if hasattr(v, "value") else v).detach()
        return {n: val(v) for n, v in seen.items()}, loss.item(), abssum, {n: p.grad for n, p in net.named_parameters()}

    p_f, loss_f, _, g_f = run(True)
    p_e, loss_e, abssum, g_e = run(False)
    assert list(p_f) == list(p_e)
    for n in p_e:
        assert torch.equal(p_f[n], p_e[n]), f"forward output {n}"
    # each product w * dw * val differs by at most two fp32 roundings, the sums run in double, one rounding of the result: 3 * 2^-24 of the
    # absolute sum; 1e-6 leaves a factor of 5
    print(f"FLAT k={k} loss flat {loss_f:.9g} eager {loss_e:.9g} |diff| {abs(loss_f - loss_e):.3g} bound {1e-6 * abssum:.3g}")
    assert abs(loss_f - loss_e) <= 1.0e-6 * abssum
    worst = (0.0, "")
    for n, ge in g_e.items():
        g64 = oracle_grads[k][n]
        gf = g_f[n]
        if g64 is None or ge is None:
            assert (ge is None or not bool(ge.any())) and (gf is None or not bool(gf.any())), n
            continue
        d_fe = float((gf.double() - ge.double()).norm())
        d_e64 = float((ge.double().cpu() - g64.reshape(ge.shape)).norm())
        ratio = d_fe / d_e64 if d_e64 > 0 else (0.0 if d_fe == 0 else float("inf"))
        worst = max(worst, (ratio, n))
        assert d_fe <= d_e64, f"{n}: |flat - eager| {d_fe:.3e} > |eager - float64| {d_e64:.3e}"
    print(f"FLAT k={k} worst |flat - eager| / |eager - float64| over the parameters: {worst[0]:.3e} ({worst[1]})")


# =====================================================================================================================================
# 4. one graph for a varying split
# =====================================================================================================================================
SEQ_SPLITS = [5, 2, 8, 5, 0, 7]  # (5,3), (2,6), (8,0), (5,3), (0,8), (7,1)
SEQ_EPOCHS = [0, 0, 0, 150, 150, 150]


def _make_run(meta):
    S = train_script()
    net = build_net(meta, DEV).train()
    crit, _ = S.setup_losses(script_args(meta["flags"]), net)
    opt, sch = S.create_optimizer(net, script_args(meta["flags"], epochs=20))
    return net, crit, opt, sch


def _eager_run(meta):
    import trackertraincode.train as train

    net, crit, opt, sch = _make_run(meta)
    losses = []
    for i, (k, ep) in enumerate(zip(SEQ_SPLITS, SEQ_EPOCHS)):
        if i == 3:
            sch.step()
        opt.zero_grad(set_to_none=True)
        out = train.training_step(net, _split_batches(meta, k, DEV, flip=i % 2 == 1), ep, crit)
        out["loss"].backward()
        opt.step()
        losses.append(out["loss"].item())
    return net, opt, losses


def test_one_graph_serves_a_varying_split(monkeypatch):
    """Six steps whose Tag split changes every step, whose ramp weights change after the third and whose learning rate changes with them:
    ONE capture, no fallback, no warning - and the trajectory of the eager per-Tag run (tolerances of
    test_model_gpu.test_graphed_train_step_matches_eager).  Rows that were landmark rows in one step and pose-only rows in the next keep
    stale landmarks in the static buffers: agreement with eager shows they are not read."""
    import trackertraincode.backbones.mobilenet_v1 as MB
    import trackertraincode.train as train

    monkeypatch.setattr(MB, "_DETERMINISTIC", True)
    _, meta = load_golden("model_full.npz")
    net_e, opt_e, losses_e = _eager_run(meta)

    net_g, crit_g, opt_g, sch_g = _make_run(meta)
    g = train.GraphedTrainStep(net_g, crit_g, opt_g, layout="flat")
    losses_g = []
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        for i, (k, ep) in enumerate(zip(SEQ_SPLITS, SEQ_EPOCHS)):
            if i == 3:
                sch_g.step()
            out = g.run(_split_batches(meta, k, DEV, flip=i % 2 == 1), ep)
            losses_g.append(out["loss"].item())
            B = meta["B"]
            assert out["mt_rows"]["shp_l2"].tolist() == [True] * k + [False] * (B - k) and out["mt_rows"]["rot"].tolist() == [True] * B
            assert not bool(out["mt_losses"]["points3d"][k:].any()) and bool(out["mt_losses"]["rot"].isfinite().all())
    torch.cuda.synchronize()
    print("FLAT graph losses", losses_g, "eager", losses_e)
    assert g.captures == 1 and g.eager_only is False
    assert opt_g._t == opt_e._t == len(SEQ_SPLITS) == 6
    np.testing.assert_allclose(losses_g[:2], losses_e[:2], rtol=1e-4)
    np.testing.assert_allclose(losses_g[2:4], losses_e[2:4], rtol=2e-3)
    np.testing.assert_allclose(losses_g[4:], losses_e[4:], rtol=6e-2)
    lr = max(gr["lr"] for gr in opt_e.param_groups)
    for (name, a), (_, b) in zip(net_g.state_dict().items(), net_e.state_dict().items()):
        if a.is_floating_point():
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=2.5 * lr * len(SEQ_SPLITS), err_msg=name)
        else:
            assert int(a) == int(b), name


def test_default_layout_still_falls_back_on_a_varying_split(monkeypatch):
    """The unchanged default: on the same sequence the per-Tag layout misses three times, warns and stays eager."""
    import trackertraincode.backbones.mobilenet_v1 as MB
    import trackertraincode.train as train

    monkeypatch.setattr(MB, "_DETERMINISTIC", True)
    _, meta = load_golden("model_full.npz")
    net, crit, opt, sch = _make_run(meta)
    g = train.GraphedTrainStep(net, crit, opt)
    assert g.layout == "per_tag"
    losses = []
    with pytest.warns(RuntimeWarning, match="sub-batch layout changed"):
        for i, (k, ep) in enumerate(zip(SEQ_SPLITS, SEQ_EPOCHS)):
            if i == 3:
                sch.step()
            out = g.run(_split_batches(meta, k, DEV, flip=i % 2 == 1), ep)
            losses.append(out["loss"].item())
            assert "mt_rows" not in out
    assert g.eager_only is True and opt._t == 6 and all(np.isfinite(losses))


# =====================================================================================================================================
# 5. end to end
# =====================================================================================================================================
def test_fit_flat_over_a_loader_that_varies_the_split(monkeypatch):
    import trackertraincode.train as train
    from trackertraincode.neuralnets.models import NetworkWithPointHead
    from trackertraincode.pipelines import SyntheticPoseLoader, Tag

    S = train_script()
    torch.manual_seed(0)
    net = NetworkWithPointHead(enable_point_head=True, enable_uncertainty=False, config="mobilenetv1", backbone_args={"use_blurpool": False})
    gen = torch.Generator().manual_seed(7)
    net.landmarks.deformablekeypoints.set_basis(torch.randn(68, 3, generator=gen) * 0.5, torch.randn(50, 68, 3, generator=gen) * 0.05)
    net = net.to(DEV)
    flags = dict(with_pointhead=True, with_nll_loss=False, rampup_nll_losses=False)
    crit, _ = S.setup_losses(script_args(flags), net)
    opt, sch = S.create_optimizer(net, script_args(flags, epochs=2))
    loader = SyntheticPoseLoader(16, [(Tag.POSE_WITH_LANDMARKS, 11), (Tag.POSE_WITH_LMKS_NO_SHAPE_PARAMS, 1), (Tag.ONLY_POSE, 2)], device=DEV,
                                 seed=5, steps_per_epoch=3, vary_split=True)
    steppers, losses = [], []

    class Recorded(train.GraphedTrainStep):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            steppers.append(self)

    monkeypatch.setattr(train, "GraphedTrainStep", Recorded)
    train.fit(net, loader, crit, opt, sch, epochs=2, graphed="flat", on_step=lambda ep, out: losses.append(out["loss"].item()))
    torch.cuda.synchronize()
    assert len(losses) == 6 and all(np.isfinite(losses)), losses
    assert len(steppers) == 1 and steppers[0].layout == "flat" and steppers[0].captures == 1 and not steppers[0].eager_only
    assert opt._t == 6 and all(torch.isfinite(q).all() for q in net.parameters())
    with pytest.raises(ValueError, match="graphed"):
        train.fit(net, loader, crit, opt, epochs=1, graphed="rows")


WRAP = r"""
import sys, os, runpy
sys.argv = [sys.argv[1]] + sys.argv[2:]
import trackertraincode.pipelines as P
_orig = P.make_pose_estimation_loaders
def short(*a, **k):
    tr, te, n = _orig(*a, **k)
    tr._steps = 4
    return tr, te, n
P.make_pose_estimation_loaders = short
runpy.run_path(sys.argv[0], run_name="__main__")
"""


@pytest.mark.parametrize("extra", [["--with-nll-loss", "--rampup-nll-losses"], ["--precision", "bf16-compute"]], ids=["nll_ramp", "bf16_compute"])
def test_train_script_graph_layout_flat(extra, tmp_path):
    """scripts/train_poseestimator.py --graph-steps --graph-layout flat as a program (epochs cut to four steps)."""
    from trackertraincode.neuralnets.models import load_model

    script = os.path.join(REPO, "neuralnet-tracker-traincode_amd", "scripts", "train_poseestimator.py")
    wrap = tmp_path / "wrap.py"
    wrap.write_text(WRAP)
    env = dict(os.environ, PYTHONPATH=os.path.join(REPO, "neuralnet-tracker-traincode_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    flags = ["--ds", "synthetic", "--batchsize", "16", "--epochs", "2", "--graph-steps", "--graph-layout", "flat", *extra]
    out = subprocess.run([sys.executable, str(wrap), script, *flags, "--outdir", str(tmp_path / "out")], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "running eagerly from here on" not in out.stderr
    net = load_model(str(tmp_path / "out" / "NetworkWithPointHead_mobilenetv1" / "last.ckpt"))
    assert all(torch.isfinite(v).all() for v in net.state_dict().values() if v.is_floating_point())
    assert net.get_config()["enable_uncertainty"] == ("--with-nll-loss" in flags)
