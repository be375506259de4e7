"""The non-finite guard of the fused clip + Adam (train.ClipAdam(skip_nonfinite=True) -> ttk_clip_adam_guarded, csrc/adam.hip) on the kernel alone.

A bad step - the total gradient norm is not finite - leaves parameters, both moments and the per-parameter step counts bitwise as they were and
counts itself in the device health block; a good step is bitwise the unguarded step.  Every comparison here is bitwise: the guard adds no
arithmetic to a good step, so there is no rounding to allow for.

Tensors: numel 1, 5, 4096 (= one chunk), 9 (never has a gradient), 4097 (a one-element last chunk) and 3 * 4096 + 7, cut from one buffer so
that some start on a 16-byte boundary (vector body) and some do not (scalar path); two groups with their own lr / weight_decay."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = 4096
NUMEL = [1, 5, CHUNK, 9, CHUNK + 1, 3 * CHUNK + 7]
OFFSET = [0, 1, 8, 8 + CHUNK, 8 + CHUNK + 9, 8212]  # in floats: tensors 0, 2, 3, 5 start 16-byte aligned, 1 and 4 do not
NO_GRAD = 3
MIDDLE, FIRST = 4, 0
LAST = NUMEL[MIDDLE] - 1  # the only element of tensor 4's last chunk


def _params():
    g = torch.Generator().manual_seed(0)
    buf = torch.randn(OFFSET[-1] + NUMEL[-1], generator=g).to(DEV)
    ps = [torch.nn.Parameter(buf[o:o + n]) for o, n in zip(OFFSET, NUMEL)]
    assert [p.data_ptr() % 16 == 0 for p in ps] == [True, False, True, True, False, True]
    return ps


def _grads(step, poison=None):
    """Seeded gradients of one step (none for tensor NO_GRAD); `poison` = (tensor, element, value)."""
    g = torch.Generator().manual_seed(100 + step)
    out = [None if i == NO_GRAD else torch.randn(n, generator=g) * (3.0 if step % 2 else 0.02) for i, n in enumerate(NUMEL)]
    if poison is not None:
        out[poison[0]][poison[1]] = poison[2]
    return [None if t is None else t.to(DEV) for t in out]


def _optimizer(ps, guarded, grad_scale=1.0):
    from trackertraincode.train import ClipAdam

    assert ClipAdam.CHUNK == CHUNK
    groups = [{"params": ps[:3], "lr": 1e-2}, {"params": ps[3:], "lr": 3e-3, "weight_decay": 0.05}]
    opt = ClipAdam(groups, lr=1e-2, max_norm=1.0, skip_nonfinite=guarded)
    opt.grad_scale = grad_scale
    return opt


def _step(opt, ps, grads):
    for p, g in zip(ps, grads):
        p.grad = g
    opt.step()


def _snapshot(opt, ps):
    torch.cuda.synchronize()
    out = []
    for p in ps:
        st = opt.state[p]
        out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), float(st["step"])))
    return out


def _assert_same(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        for what, u, v in zip(("param", "exp_avg", "exp_avg_sq"), x[:3], y[:3]):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), (i, what)  # bit patterns: a NaN would not compare equal to itself
        assert x[3] == y[3], (i, "step", x[3], y[3])


POISONS = {"nan_last_element_of_last_chunk_of_a_middle_tensor": (MIDDLE, LAST, float("nan")),
           "inf_in_the_first_tensor": (FIRST, 0, float("inf")),
           "finite_1e20_whose_square_overflows": (MIDDLE, LAST, 1.0e20)}


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("poison", list(POISONS))
def test_bad_step_changes_nothing_and_is_counted(poison, grad_scale):
    ti, el, val = POISONS[poison]
    ps = _params()
    opt = _optimizer(ps, True, grad_scale)
    assert opt.health() == {"skipped": 0, "consecutive": 0, "culprit_index": -1}
    _step(opt, ps, _grads(0))  # a good step first: the moments and step counts are not zero
    before = _snapshot(opt, ps)
    assert [s[3] for s in before] == [1.0, 1.0, 1.0, 0.0, 1.0, 1.0] and math.isfinite(opt.last_grad_norm.item())
    assert opt.health() == {"skipped": 0, "consecutive": 0, "culprit_index": -1}
    _step(opt, ps, _grads(1, (ti, el, val)))
    _assert_same(_snapshot(opt, ps), before)
    assert opt.health() == {"skipped": 1, "consecutive": 1, "culprit_index": ti}
    assert not math.isfinite(opt.last_grad_norm.item())
    # the same poisoned step through the unguarded entry point ruins the state: the poison is one
    ps_u = _params()
    opt_u = _optimizer(ps_u, False, grad_scale)
    _step(opt_u, ps_u, _grads(0))
    _assert_same(_snapshot(opt_u, ps_u), before)
    _step(opt_u, ps_u, _grads(1, (ti, el, val)))
    after_u = _snapshot(opt_u, ps_u)
    if math.isfinite(val):  # an infinite norm clips a finite gradient to zero: the step still decays the moments and counts itself
        assert [s[3] for s in after_u] == [2.0, 2.0, 2.0, 0.0, 2.0, 2.0] and not torch.equal(after_u[0][1], before[0][1])
    else:
        assert not bool(torch.isfinite(after_u[ti][0]).all())
    with pytest.raises(RuntimeError, match="skip_nonfinite"):
        opt_u.health()


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_good_steps_are_bitwise_the_unguarded_ones(grad_scale):
    ps_g, ps_u = _params(), _params()
    og, ou = _optimizer(ps_g, True, grad_scale), _optimizer(ps_u, False, grad_scale)
    _step(og, ps_g, _grads(0))
    _step(ou, ps_u, _grads(0))
    _step(og, ps_g, _grads(1, POISONS["inf_in_the_first_tensor"]))  # skipped: the unguarded twin does not see this step at all
    assert og.health() == {"skipped": 1, "consecutive": 1, "culprit_index": FIRST}
    for s in (2, 3):
        _step(og, ps_g, _grads(s))
        _step(ou, ps_u, _grads(s))
        _assert_same(_snapshot(og, ps_g), _snapshot(ou, ps_u))
        assert og.last_grad_norm.item() == ou.last_grad_norm.item()
    assert og.health() == {"skipped": 1, "consecutive": 0, "culprit_index": FIRST}
    assert [s[3] for s in _snapshot(og, ps_g)] == [3.0, 3.0, 3.0, 0.0, 3.0, 3.0]


def _bad_good_bad(replayed):
    """One eager good step, then bad / good / bad - eagerly, or as three replays of ONE captured step over static gradient tensors."""
    ps = _params()
    opt = _optimizer(ps, True)
    static = _grads(0)
    _step(opt, ps, static)
    sequence = [_grads(1, POISONS["nan_last_element_of_last_chunk_of_a_middle_tensor"]), _grads(2), _grads(3, POISONS["inf_in_the_first_tensor"])]
    if not replayed:
        for grads in sequence:
            _step(opt, ps, grads)
        return _snapshot(opt, ps), opt.health(), opt.last_grad_norm.item()
    torch.cuda.synchronize()
    opt.sync_hyper_to_device()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()  # (the parameters' .grad are the static tensors; capturing runs nothing)
    for grads in sequence:
        for s, g in zip(static, grads):
            if s is not None:
                s.copy_(g)
        opt.before_graph_replay()
        graph.replay()
        opt.after_graph_replay()
    return _snapshot(opt, ps), opt.health(), opt.last_grad_norm.item()


def test_captured_step_replayed_bad_good_bad_equals_the_eager_sequence():
    eager, health_e, norm_e = _bad_good_bad(False)
    graph, health_g, norm_g = _bad_good_bad(True)
    _assert_same(graph, eager)
    assert health_g == health_e == {"skipped": 2, "consecutive": 1, "culprit_index": FIRST}
    assert math.isinf(norm_e) and math.isinf(norm_g)
    # and both are the two good steps alone
    ps = _params()
    opt = _optimizer(ps, False)
    _step(opt, ps, _grads(0))
    _step(opt, ps, _grads(2))
    _assert_same(eager, _snapshot(opt, ps))


def test_state_dict_after_a_skipped_step_resumes_like_a_run_without_it():
    ps_g, ps_u = _params(), _params()
    og, ou = _optimizer(ps_g, True), _optimizer(ps_u, False)
    _step(og, ps_g, _grads(0))
    _step(og, ps_g, _grads(1, POISONS["finite_1e20_whose_square_overflows"]))
    _step(og, ps_g, _grads(2))
    _step(ou, ps_u, _grads(0))
    _step(ou, ps_u, _grads(2))
    sd = copy.deepcopy(og.state_dict())
    assert [float(sd["state"][i]["step"]) for i in range(len(NUMEL))] == [float(ou.state[p]["step"]) for p in ps_u] == [2.0, 2.0, 2.0, 0.0, 2.0, 2.0]
    health = og.health()
    ps_r = [torch.nn.Parameter(p.detach().clone()) for p in ps_g]
    orr = _optimizer(ps_r, True)
    orr.load_state_dict(sd)
    orr.load_health(health)
    assert orr.health() == health == {"skipped": 1, "consecutive": 0, "culprit_index": MIDDLE}
    _step(orr, ps_r, _grads(3))
    _step(ou, ps_u, _grads(3))
    _assert_same(_snapshot(orr, ps_r), _snapshot(ou, ps_u))
    assert orr.health() == health
    og.load_state_dict(sd)  # a load drops the device tables; the counters survive it
    assert og._tables is None and og.health() == health
