"""Fused clip + Adam (train.ClipAdam -> csrc/adam.hip) against torch.optim.Adam + clip_grad_norm_ - the pair the reference
gets from Lightning (scripts/train_poseestimator.py:147-167, :442-445): checkpoint resume, per-parameter step counts
(a parameter without a gradient is not stepped), data-parallel gradient scale, stable device tables.  The second half holds
train.ClipAdam to the float64 reference of tests/adam_ref.py, element by element and within its derived bounds: un-clipped steps,
max_norm=None, weight decay on a multi-chunk tensor, a transposed gradient, misaligned views of one buffer, and a learning rate
changed between eager steps and between replays of one captured step; each also against double-beta semantics with the derived term."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1024, 1024), (50, 1024), (7,), (3, 3, 5), (4097,), (1,)]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(DEV)) for s in SHAPES]


def _grads(step, skip=()):
    g = torch.Generator().manual_seed(100 + step)
    return [None if i in skip else (torch.randn(s, generator=g) * (10.0 if step % 2 else 0.01)).to(DEV) for i, s in enumerate(SHAPES)]


def _groups(ps):
    return [{"params": ps[:3], "lr": 1e-3}, {"params": ps[3:5], "lr": 1e-4}, {"params": ps[5:], "lr": 1e-5, "weight_decay": 0.01}]


def _reference_run(steps, skips):
    ps = _params()
    opt = torch.optim.Adam(_groups(ps), lr=1e-3)
    for s in range(steps):
        for p, g in zip(ps, _grads(s, skips.get(s, ()))):
            p.grad = g
        torch.nn.utils.clip_grad_norm_(ps, 1.0)
        opt.step()
    return ps, opt


def test_matches_torch_adam_with_skipped_parameters_and_resume():
    from trackertraincode.train import ClipAdam

    skips = {1: (2, 4), 2: (2,)}  # parameters 2 and 4 have no gradient in some steps: torch does not advance their step count
    ref_ps, ref_opt = _reference_run(5, skips)

    ps = _params()
    opt = ClipAdam(_groups(ps), lr=1e-3, max_norm=1.0)
    for s in range(3):
        for p, g in zip(ps, _grads(s, skips.get(s, ()))):
            p.grad = g
        opt.step()
    # ---- checkpoint, resume into a fresh optimiser over copies of the parameters
    sd = copy.deepcopy(opt.state_dict())
    assert float(sd["state"][2]["step"]) == 1.0 and float(sd["state"][0]["step"]) == 3.0  # per-parameter counts
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = ClipAdam(_groups(ps2), lr=1e-3, max_norm=1.0)
    opt2.load_state_dict(sd)
    assert opt2._t == 3
    for s in range(3, 5):
        for p, g in zip(ps2, _grads(s, skips.get(s, ()))):
            p.grad = g
        opt2.step()
    torch.cuda.synchronize()
    for a, b in zip(ps2, ref_ps):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=1e-5, atol=2e-7)
    for a, b in zip(ps2, ref_ps):
        sa, sb = opt2.state[a], ref_opt.state[b]
        assert float(sa["step"]) == float(sb["step"])
        np.testing.assert_allclose(sa["exp_avg"].cpu().numpy(), sb["exp_avg"].cpu().numpy(), rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(sa["exp_avg_sq"].cpu().numpy(), sb["exp_avg_sq"].cpu().numpy(), rtol=5e-5, atol=1e-12)  # g^2 after the clip coefficient: twice its fp32 rounding
    # a load AFTER steps were taken must drop every cached device address (the old moments are orphaned otherwise)
    opt2.load_state_dict(sd)
    assert opt2._tables is None and opt2._t == 3


def test_grad_scale_equals_prescaled_gradients():
    """grad_scale = 1/world with summed gradients in memory == plain step on the averaged gradients."""
    from trackertraincode.train import ClipAdam

    world = 8
    a, b = _params(), _params()
    oa, ob = ClipAdam(_groups(a), max_norm=1.0), ClipAdam(_groups(b), max_norm=1.0)
    ob.grad_scale = 1.0 / world
    for s in range(3):
        for p, q, g in zip(a, b, _grads(s)):
            p.grad, q.grad = g, g * world
        oa.step()
        ob.step()
        np.testing.assert_allclose(ob.last_grad_norm.item(), oa.last_grad_norm.item(), rtol=1e-6)
    for p, q in zip(a, b):
        np.testing.assert_allclose(q.detach().cpu().numpy(), p.detach().cpu().numpy(), rtol=1e-5, atol=1e-7)


def test_pointer_table_follows_new_gradient_addresses():
    """Gradients that live at new addresses every step (fresh tensors, the old ones kept alive) must be the ones read."""
    from trackertraincode.train import ClipAdam

    ref_ps, _ = _reference_run(4, {})
    ps = _params()
    opt = ClipAdam(_groups(ps), max_norm=1.0)
    keep = []
    for s in range(4):
        gs = _grads(s)
        keep.append(gs)  # nothing is freed: the allocator cannot hand the same addresses out again
        for p, g in zip(ps, gs):
            p.grad = g
        opt.step()  # no synchronisation between steps: the host runs ahead of the GPU
    torch.cuda.synchronize()
    for a, b in zip(ps, ref_ps):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=1e-5, atol=2e-7)


# ---------------------------------------------------------------------------------------------------------------------------------
# train.ClipAdam against float64, element by element (tests/adam_ref.py: the reference and the derivation of every bound)
# ---------------------------------------------------------------------------------------------------------------------------------
BIG = 2 * 4096 + 3  # three chunks of ClipAdam.CHUNK, the last of 3 elements
REF_SHAPES = [(33, 7), (BIG,), (5,), (1,)]
SETTINGS = {"unclipped": {}, "max_norm_none": dict(max_norm=None, gscale=40.0), "wd_multichunk": dict(gscale=40.0),
            "transposed_grad": dict(transposed=True), "misaligned_views": dict(misaligned=True, gscale=40.0)}


def _ref_params(misaligned=False):
    """Parameters of REF_SHAPES; `misaligned`: contiguous views of ONE buffer that start 4, 8, 12 and 4 bytes past a 16-byte boundary."""
    g = torch.Generator().manual_seed(7)
    if not misaligned:
        return [torch.nn.Parameter(torch.randn(s, generator=g).to(DEV)) for s in REF_SHAPES]
    sizes = [int(np.prod(s)) for s in REF_SHAPES]
    starts, cur = [], 0
    for k, n in enumerate(sizes):
        starts.append((cur + 3) // 4 * 4 + (1, 2, 3, 1)[k])
        cur = starts[-1] + n
    buf = torch.randn(cur, generator=g).to(DEV)
    ps = [torch.nn.Parameter(buf[o:o + n].view(s)) for o, n, s in zip(starts, sizes, REF_SHAPES)]
    assert [p.data_ptr() % 16 for p in ps] == [4, 8, 12, 4] and all(p.is_contiguous() for p in ps)
    return ps


def _ref_groups(ps):
    # the weight-decay group (lr 1e-5, the rate whose whole step the allclose tolerance above swallows) holds the multi-chunk tensor
    return [{"params": [ps[0], ps[2]], "lr": 1e-3}, {"params": [ps[1], ps[3]], "lr": 1e-5, "weight_decay": 0.05}]


def _ref_grads(ps, step, gscale=1.0, transposed=False):
    """Seeded gradients of norm ~0.1 * gscale (below max_norm = 1 at gscale 1); `transposed`: the matrix's gradient is a transposed view."""
    g = torch.Generator().manual_seed(300 + step)
    out = []
    for p in ps:
        if transposed and p.dim() == 2:
            t = (torch.randn(p.shape[1], p.shape[0], generator=g) * (1e-3 * gscale)).to(DEV).t()
            assert not t.is_contiguous()
        else:
            t = (torch.randn(p.shape, generator=g) * (1e-3 * gscale)).to(DEV)
        out.append(t)
    return out


def _state_before(opt, ps, grads):
    """What the next step is given, as float32 numpy: p, g, m, v per tensor in the order of the groups, steps, group indices, hyper."""
    import adam_ref as R

    torch.cuda.synchronize()
    order = [(p, gi) for gi, grp in enumerate(opt.param_groups) for p in grp["params"]]
    gof = {id(p): g for p, g in zip(ps, grads)}
    f = lambda t: t.detach().contiguous().cpu().numpy().reshape(-1).copy()
    st = [opt.state[p] for p, _ in order]
    zeros = lambda p: np.zeros(p.numel(), np.float32)
    b1, b2 = opt.param_groups[0]["betas"]
    h = R.hyper([grp["lr"] for grp in opt.param_groups], [grp["weight_decay"] for grp in opt.param_groups], b1, b2, opt.param_groups[0]["eps"],
                float(opt.max_norm or 0.0), opt.grad_scale)
    return dict(params=[p for p, _ in order], p=[f(p) for p, _ in order], g=[None if gof[id(p)] is None else f(gof[id(p)]) for p, _ in order],
                m=[f(s["exp_avg"]) if "exp_avg" in s else zeros(p) for s, (p, _) in zip(st, order)],
                v=[f(s["exp_avg_sq"]) if "exp_avg_sq" in s else zeros(p) for s, (p, _) in zip(st, order)],
                steps=np.array([float(s["step"]) if "step" in s else 0.0 for s in st], np.float32), group=[gi for _, gi in order], h=h)


def _judge(opt, b, what):
    """The state after the step that was given `b` against adam_ref: the derived bound against the float32-beta reference, and the same
    bound plus the derived double-beta term against double-beta semantics (what torch.optim.Adam computes by default)."""
    import adam_ref as R
    from trackertraincode.train import ClipAdam

    torch.cuda.synchronize()
    print()
    f = lambda t: t.detach().cpu().numpy().reshape(-1)
    p = [f(q) for q in b["params"]]
    m, v = [f(opt.state[q]["exp_avg"]) for q in b["params"]], [f(opt.state[q]["exp_avg_sq"]) for q in b["params"]]
    steps = np.array([float(opt.state[q]["step"]) for q in b["params"]], np.float32)
    r = R.reference(b["p"], b["g"], b["m"], b["v"], b["steps"], b["group"], b["h"], ClipAdam.CHUNK)
    ratios = R.ratios(r, p, m, v, steps, opt.last_grad_norm.item())
    print("RATIO ClipAdam", what, {k: f"{x:.3f}" for k, x in ratios.items()})
    assert all(x <= 1.0 for x in ratios.values()), (what, ratios)
    rd = R.reference(b["p"], b["g"], b["m"], b["v"], b["steps"], b["group"], b["h"], ClipAdam.CHUNK, betas64=tuple(opt.param_groups[0]["betas"]))
    # the gap between the two semantics (float64 against float64) next to the term derived for it, which must bound it element by element
    gap = max(float(np.abs(a - c).max()) for a, c in zip(r.p, rd.p))
    derived = max(float(x.max()) for x in rd.dbeta)
    assert all((np.abs(a - c) <= 1.001 * x + 1e-15 * np.abs(a)).all() for a, c, x in zip(r.p, rd.p, rd.dbeta))
    rp = R.ratios(rd, p, m, v, steps, extra_p=rd.dbeta)["p"]
    print("RATIO ClipAdam double-beta", what, f"p {rp:.3f}  measured gap {gap:.3e}  derived double-beta term {derived:.3e}")
    assert rp <= 1.0, (what, rp)
    return r


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_clip_adam_step_against_float64(setting):
    from trackertraincode.train import ClipAdam

    s = dict(SETTINGS[setting])
    ps = _ref_params(s.pop("misaligned", False))
    opt = ClipAdam(_ref_groups(ps), max_norm=s.pop("max_norm", 1.0))
    for step in range(2):  # from zero moments, then from live ones
        grads = _ref_grads(ps, step, **s)
        b = _state_before(opt, ps, grads)
        for p, g in zip(ps, grads):
            p.grad = g
        opt.step()
        r = _judge(opt, b, f"{setting}[{step}]")
        clipped = r.coef < 1.0
        assert clipped == (setting in ("wd_multichunk", "misaligned_views")), (setting, r.norm, r.coef)
        assert [float(x) for x in r.steps] == [step + 1.0] * 4


def _lr_sequence(replayed):
    """One eager step, then three more with the first group's learning rate divided by 10 before the second of them and the second
    group's multiplied by 50 before the third - eagerly (host arrays), or as replays of ONE captured step (device block)."""
    from trackertraincode.train import ClipAdam

    ps = _ref_params()
    opt = ClipAdam(_ref_groups(ps), max_norm=1.0)
    static = _ref_grads(ps, 0, gscale=40.0)
    for p, g in zip(ps, static):
        p.grad = g
    b = _state_before(opt, ps, static)
    opt.step()
    _judge(opt, b, f"lr[{'graph' if replayed else 'eager'}][0]")
    graph = None
    if replayed:
        torch.cuda.synchronize()
        opt.sync_hyper_to_device()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opt.step()  # (a single linear step; capturing runs nothing)
    for k in (1, 2, 3):
        if k == 2:
            opt.param_groups[0]["lr"] = 1e-4
        if k == 3:
            opt.param_groups[1]["lr"] = 5e-4
        for s, g in zip(static, _ref_grads(ps, k, gscale=40.0 if k % 2 else 1.0)):
            s.copy_(g)
        b = _state_before(opt, ps, static)
        assert [float(x) for x in b["h"].lr[:2]] == [float(np.float32(1e-3 if k < 2 else 1e-4)), float(np.float32(1e-5 if k < 3 else 5e-4))]
        if replayed:
            opt.before_graph_replay()
            graph.replay()
            opt.after_graph_replay()
        else:
            opt.step()
        _judge(opt, b, f"lr[{'graph' if replayed else 'eager'}][{k}]")  # the new rate holds from the first step after the change
    torch.cuda.synchronize()
    return [p.detach().clone() for p in ps]


def test_learning_rate_changed_between_eager_steps_and_between_replays():
    eager = _lr_sequence(False)
    graph = _lr_sequence(True)
    for a, b in zip(eager, graph):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
