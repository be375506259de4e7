"""The float64 reference of the fused clip + Adam tests (tests/adam_ref.py) on its own, without a GPU: a float32 emulation of the
kernel's arithmetic meets every bound in every case of the table, the same emulation with ONE planted error is rejected in a named case,
and the reference is torch.optim.Adam behind clip_grad_norm_ in float64 - so that a failure of tests/test_adam_rows_gpu.py indicts the
kernel and a pass means something."""
import functools
import math

import numpy as np
import pytest
import torch

import adam_ref as R

F = np.float32


def _fma(a, b, c):
    """float32 fma: the product of two float32 values is exact in float64; the sum is rounded to 53 bits and then to 24 (a double
    rounding that differs from the fused one only on a tie of the second)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _chunk_sqsum(g):
    """Sum of squares of one chunk in float32, in another order than the kernel's: 256 lanes take the elements lane, lane + 256, ...
    one by one (the kernel takes them in fours), then a pairwise tree over the lanes (the kernel: 6 shuffle levels and 4 serial adds).
    No square passes through more than ceil(n/256) + 8 additions, which is within the L + 10 of the bound at every chunk size."""
    lanes = np.zeros(256, F)
    pad = np.zeros((len(g) + 255) // 256 * 256, F)
    pad[:len(g)] = g
    for row in pad.reshape(-1, 256):
        lanes = _fma(row, row, lanes)
    while len(lanes) > 1:
        lanes = lanes[0::2] + lanes[1::2]
    return lanes[0]


MUTATIONS = {  # planted error -> the case of adam_ref.TABLE that must reject it
    "wd_dropped": "product_mix",
    "wd_decoupled": "product_mix",
    "wd_before_clip": "product_mix",
    "clip_always": "chunk64_unclipped_third",
    "no_1e-6": "clip_just_above_1e-3",
    "norm_without_grad_scale": "chunk16384_passes",
    "update_without_grad_scale": "chunk64_unclipped_third",
    "shared_step_count": "product_mix",
    "step_without_gradient": "no_gradient",
    "eps_inside_sqrt": "tiny_gradients",
    "eps_before_bias_correction": "eps_1e-3",
    "bc2_not_rooted": "eps_1e-3",
    "tail_last_element_skipped": "chunks_257",
    "chunk_twice": "chunks_600",
    "hyper_dev_ignored": "hyper_dev",
}


def emulate(c, bufs, steps, mut=None):
    """One call of the kernel pair on the CPU, operation by operation in float32 (csrc/adam.hip: grad_sqnorm_k, clip_adam_k), chunk by
    chunk.  bufs: role -> float32 buffer (copied); steps: float32.  `mut`: one planted error.  -> bufs, steps, norm, partial."""
    bufs = {k: np.array(a) for k, a in bufs.items()}
    steps = np.array(steps, F)
    h = c.h
    lr, wd = (np.full(R.MAX_GROUPS, np.nan, F),) * 2 if (c.hyper_dev and mut == "hyper_dev_ignored") else (h.lr, h.wd)
    nch = len(c.chunk_tensor)
    partial = np.zeros(nch, F)
    view = lambda role, ti, off, n: bufs[role][c.pos[role][ti] + off:c.pos[role][ti] + off + n]
    for k in range(nch):
        ti, off = c.chunk_tensor[k], c.chunk_offset[k]
        n = min(c.chunk, c.numel[ti] - off)
        if off == 0 and (c.has_grad[ti] or mut == "step_without_gradient"):
            steps[ti] += F(1)
        if c.has_grad[ti]:
            partial[k] = _chunk_sqsum(view("g", ti, off, n))
    gs = h.grad_scale
    total = (F(1) if mut == "norm_without_grad_scale" else gs) * F(math.sqrt(float(np.sum(partial.astype(np.float64)))))
    coef = F(1) if mut == "update_without_grad_scale" else gs
    if h.max_norm > 0:
        q = h.max_norm / (total if mut == "no_1e-6" else total + F(1e-6))
        coef = coef * (q if mut == "clip_always" else min(q, F(1)))
    for k in list(range(nch)) + ([nch - 1] if mut == "chunk_twice" else []):
        ti, off = c.chunk_tensor[k], c.chunk_offset[k]
        if not c.has_grad[ti]:
            continue
        n = min(c.chunk, c.numel[ti] - off)
        if mut == "tail_last_element_skipped" and n < c.chunk:
            n -= 1
        p, g, m, v = (view(role, ti, off, n) for role in R.ROLES)
        w = wd[c.group[ti]]
        t = float(steps[0] if mut == "shared_step_count" else steps[ti])
        bc1, bc2 = F(1.0 - float(h.beta1) ** t), F(1.0 - float(h.beta2) ** t)
        step_size = lr[c.group[ti]] / bc1
        inv = F(1) / (bc2 if mut == "bc2_not_rooted" else np.sqrt(bc2))
        if mut == "wd_before_clip":
            gr = _fma(w, p, g) * coef
        else:
            gr = g * coef
            if w != 0 and mut not in ("wd_dropped", "wd_decoupled"):
                gr = _fma(w, p, gr)
        m[:] = _fma(h.beta1, m, (F(1) - h.beta1) * gr)
        v[:] = _fma(h.beta2, v, (F(1) - h.beta2) * gr * gr)
        if mut == "eps_inside_sqrt":
            denom = np.sqrt(v + h.eps) * inv
        elif mut == "eps_before_bias_correction":
            denom = (np.sqrt(v) + h.eps) * inv
        else:
            denom = np.sqrt(v) * inv + h.eps
        q = p * (F(1) - lr[c.group[ti]] * w) if mut == "wd_decoupled" else p
        p[:] = q - step_size * (m / denom)
    return bufs, steps, total, partial


@functools.lru_cache(maxsize=None)
def _case(name):
    return R.make_case(name)


def _run(name, mut=None):
    """Every call of a case through the emulation, teacher-forced: -> the worst ratio per output over the calls."""
    c = _case(name)
    bufs, steps = dict(c.buf), c.steps0
    worst = {}
    for k in range(c.calls):
        bufs = dict(bufs, g=c.grads[k])
        r = R.case_reference(c, bufs, steps)
        out, steps, norm, _ = emulate(c, bufs, steps, mut)
        assert R.bands_untouched(c, out)
        for key, val in R.case_ratios(c, r, out, steps, norm).items():
            worst[key] = val if (val != val or val > worst.get(key, 0.0)) else worst.get(key, 0.0)
        bufs = out
    return worst


@pytest.mark.parametrize("name", R.CASES)
def test_float32_emulation_meets_every_bound(name):
    w = _run(name)
    print("RATIO emulation", name, {k: f"{v:.3f}" for k, v in w.items()})
    assert all(v <= 1.0 for v in w.values()), w


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_planted_error_is_rejected(mut):
    w = _run(MUTATIONS[mut], mut)
    print("RATIO", mut, MUTATIONS[mut], {k: f"{v:.3g}" for k, v in w.items()})
    assert not all(v <= 1.0 for v in w.values()), (mut, w)


def test_exact_rules_are_armed():
    """The bitwise rules have elements to judge: planted zeros with bound 0, and the one-product bound where coef == grad_scale == 1."""
    c = _case("zeros")
    r = R.case_reference(c, c.buf, c.steps0)
    assert (r.tp[0] == 0).all() and (r.tm[0] == 0).all() and (r.tv[0] == 0).all()  # all-zero gradient on zero moments
    assert (r.tp[2] == 0).sum() == 1 and (r.tp[1] > 0).sum() == c.numel[1] - 1    # planted element / pure decay of live moments
    c = _case("one_chunk")
    r = R.case_reference(c, c.buf, c.steps0)
    live = r.tm[0] > 0
    assert live.sum() == c.numel[0] - 1 and np.allclose(r.tm[0][live], R.U * np.abs(r.m[0][live]) + R.FLT_MIN, rtol=0, atol=0)


def test_case_table_covers_the_dimensions():
    cs = [_case(n) for n in R.CASES]
    assert {c.chunk for c in cs} == {64, 66, 4096, 16384}
    assert {len(c.chunk_tensor) for c in cs} >= {1, 256, 257} and any(590 <= len(c.chunk_tensor) <= 610 for c in cs)
    offs = {tuple(c.pos[role][i] % 4 for role in R.ROLES) for c in cs for i in range(len(c.numel))}
    assert offs >= {(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (0, 2, 0, 0), (0, 0, 0, 1), (1, 0, 0, 0), (0, 0, 3, 0)}
    assert {float(c.h.grad_scale) for c in cs} == {1.0, 0.125, float(F(1 / 3))}
    assert {float(s) for c in cs for s in c.steps0} == {0.0, 1.0, 9.0, 999.0, 100000.0}
    assert any(c.hyper_dev for c in cs) and any(c.group == [0, 127, 64] for c in cs) and any(c.calls == 3 for c in cs)
    assert {float(c.h.eps) for c in cs} == {float(F(1e-8)), float(F(1e-3))} and any(float(c.h.beta1) == 0.5 for c in cs)


@pytest.mark.parametrize("name", R.CASES)
def test_double_beta_term_bounds_the_gap_between_the_two_semantics(name):
    """float64 against float64: the reference with the betas as Python doubles (0.9, 0.999 - torch.optim.Adam's default path) differs
    from the reference with the float32 betas by at most the derived term, element by element (first order: 0.1 % of room)."""
    c = _case(name)
    nominal = tuple(float(f"{float(b):.6g}") for b in (c.h.beta1, c.h.beta2))
    assert nominal in ((0.9, 0.999), (0.5, 0.9))
    r, rd = R.case_reference(c, c.buf, c.steps0), R.case_reference(c, c.buf, c.steps0, betas64=nominal)
    for a, b, x in zip(r.p, rd.p, rd.dbeta):
        assert (np.abs(a - b) <= 1.001 * x + 1e-15 * np.abs(a)).all()
    if nominal[1] == 0.999:  # the figure of the module docstring: 6.4e-6 of the update at t = 1 through the bias correction of beta2
        k2 = 0.5 * abs(float(c.h.beta2) - 0.999) / (1 - float(c.h.beta2))
        assert 6.3e-6 < k2 < 6.6e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference is torch's Adam behind clip_grad_norm_, in float64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["product_mix", "chunk66_off_boundary", "no_gradient"])
def test_reference_is_float64_torch_adam_behind_clip_grad_norm(name):
    """grad_scale: torch sees the scaled gradients; per-parameter steps: planted in torch's state.  betas, lr, wd, eps, max_norm: the
    float32 values widened to Python doubles, as in the reference."""
    c = _case(name)
    h = c.h
    r = R.case_reference(c, c.buf, c.steps0)
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    ps = [torch.nn.Parameter(t64(a)) for a in R.tensors_of(c, c.buf, "p")]
    groups = {}
    for i, p in enumerate(ps):
        groups.setdefault(c.group[i], []).append(p)
    opt = torch.optim.Adam([{"params": q, "lr": float(h.lr[gi]), "weight_decay": float(h.wd[gi])} for gi, q in groups.items()],
                           betas=(float(h.beta1), float(h.beta2)), eps=float(h.eps), foreach=False)
    ms, vs, gsv = R.tensors_of(c, c.buf, "m"), R.tensors_of(c, c.buf, "v"), R.tensors_of(c, c.buf, "g", True)
    for i, p in enumerate(ps):
        opt.state[p] = {"step": torch.tensor(float(c.steps0[i])), "exp_avg": t64(ms[i]), "exp_avg_sq": t64(vs[i])}
        p.grad = None if gsv[i] is None else t64(gsv[i]) * float(h.grad_scale)
    if h.max_norm > 0:
        norm = torch.nn.utils.clip_grad_norm_(ps, float(h.max_norm))
        assert abs(float(norm) - r.norm) <= 1e-12 * r.norm
    opt.step()
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * float(np.abs(b).max()))
    for i, p in enumerate(ps):
        close(p.detach().numpy(), r.p[i])
        close(opt.state[p]["exp_avg"].numpy(), r.m[i])
        close(opt.state[p]["exp_avg_sq"].numpy(), r.v[i])
        assert float(opt.state[p]["step"]) == float(r.steps[i])
