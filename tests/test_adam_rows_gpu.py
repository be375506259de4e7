"""ttk_clip_adam / ttk_clip_adam_guarded (csrc/adam.hip) against float64, element by element, through the C ABI with device tables
built here (tests/adam_ref.py: the reference, the derivation of every bound, the case table; tests/test_adam_ref.py: the reference on its
own).  Per case: parameters, both moments, steps[] (exact) and out_norm are judged, the sentinel bands around every tensor and around
`partial` must be bitwise untouched, everything must be finite, a second run from the same state must repeat bit for bit (with out_norm
null), and the guarded entry must give the same bits, reset health[CONSECUTIVE] and leave SKIPPED and CULPRIT alone.  Each case prints
"RATIO <entry> <case> <output> <worst error/bound>"; the assertion is the derived bound, ratio <= 1.

Worst ratios on the MI355X (the full listing: profiles/adam_float64.txt), measurements - the assertion is the derived bound:
    p 0.995 (chunks_600)    exp_avg 0.944 (eps_1e-3)    exp_avg_sq 0.583 (chunk16384_passes)    norm 0.083 (chunks_257)
p and, under the one-product rule, exp_avg sit close to 1 because their bounds are one rounding, u|x|, which round-to-nearest attains
just above a power of two.  The norm's bound is slack by a factor of 12: it lets each of the L + 10 additions of a sum of squares err
at its worst and to one side, where they average out; it enters the other bounds beside larger terms, and the planted errors of
tests/test_adam_ref.py that touch the norm are rejected all the same.  Nothing here plants a non-finite value."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
HEALTH0 = [5, 3, 7, 0]  # SKIPPED, CONSECUTIVE, CULPRIT, spare: what the guarded entry finds


@functools.lru_cache(maxsize=None)
def _case(name):
    return R.make_case(name)


class _Call:
    """The device side of one case: the four buffers, the tables, `partial` between sentinel bands, and the argument list."""

    def __init__(self, c):
        i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
        self.c = c
        self.bufs = {role: torch.from_numpy(c.buf[role]).to(DEV) for role in R.ROLES}
        self.steps = torch.from_numpy(c.steps0).to(DEV)
        base = {role: self.bufs[role].data_ptr() for role in R.ROLES}
        assert all(b % 16 == 0 for b in base.values())  # the offsets of the table are offsets from a 16-byte boundary
        for role in R.ROLES:  # every tensor lies inside its buffer, a band away from both ends
            for pos, n in zip(c.pos[role], c.numel):
                assert R.BAND <= pos and pos + n + R.BAND <= self.bufs[role].numel()
        ptrs = [[0 if (role == "g" and not c.has_grad[i]) else base[role] + 4 * c.pos[role][i] for role in R.ROLES] for i in range(len(c.numel))]
        self.ptrs = torch.tensor(ptrs, dtype=torch.int64, device=DEV)
        self.numel, self.group = i32(c.numel), i32(c.group)
        assert all(0 <= o < c.numel[t] for t, o in zip(c.chunk_tensor, c.chunk_offset))
        self.chunk_tensor, self.chunk_offset = i32(c.chunk_tensor), i32(c.chunk_offset)
        self.nchunks = len(c.chunk_tensor)
        self.partial = torch.full((2 * R.BAND + self.nchunks,), float(R.SENTINEL), device=DEV)
        self.partial[R.BAND:R.BAND + self.nchunks] = float("nan")
        self.norm = torch.full((1 + 2 * R.BAND,), float(R.SENTINEL), device=DEV)
        self.health = torch.tensor(HEALTH0, dtype=torch.int32, device=DEV)
        G = R.MAX_GROUPS
        host = (lambda a: np.full(G, np.nan, np.float32)) if c.hyper_dev else (lambda a: a)
        self.lr4, self.wd4 = (ctypes.c_float * G)(*host(c.h.lr)), (ctypes.c_float * G)(*host(c.h.wd))
        self.hyper = torch.from_numpy(np.concatenate([c.h.lr, c.h.wd])).to(DEV) if c.hyper_dev else None

    def args(self, with_norm=True, **over):
        h, p = self.c.h, (lambda t: None if t is None else t.data_ptr())
        a = dict(ptrs=p(self.ptrs), numel=p(self.numel), group=p(self.group), chunk_tensor=p(self.chunk_tensor), chunk_offset=p(self.chunk_offset),
                 nchunks=self.nchunks, chunk=self.c.chunk, lr4=self.lr4, wd4=self.wd4, b1=float(h.beta1), b2=float(h.beta2), eps=float(h.eps),
                 max_norm=float(h.max_norm), grad_scale=float(h.grad_scale), steps=p(self.steps), partial=self.partial.data_ptr() + 4 * R.BAND,
                 norm=self.norm.data_ptr() + 4 * R.BAND if with_norm else None, hyper=p(self.hyper))
        a.update(over)
        return list(a.values())

    def state(self):
        torch.cuda.synchronize()
        return {role: self.bufs[role].cpu().numpy() for role in R.ROLES}, self.steps.cpu().numpy()


def _run(c, guarded=False, with_norm=True):
    """Every call of the case from its initial state.  -> [(bufs before, steps before, bufs after, steps after, norm, partial)] per call, health."""
    import trackertraincode._hip as hip

    d = _Call(c)
    out = []
    for k in range(c.calls):
        d.bufs["g"].copy_(torch.from_numpy(c.grads[k]))
        before = d.state()
        if guarded:
            hip.lib().call("ttk_clip_adam_guarded", *d.args(with_norm), d.health.data_ptr())
        else:
            hip.lib().call("ttk_clip_adam", *d.args(with_norm))
        after = d.state()
        out.append((*before, *after, d.norm.cpu().numpy(), d.partial.cpu().numpy()))
    return out, d.health.cpu().tolist()


def _bits(a):
    return np.asarray(a).view(np.uint32)


@pytest.mark.parametrize("name", R.CASES)
def test_clip_adam_against_float64(name):
    c = _case(name)
    first, _ = _run(c)
    sent = _bits(R.SENTINEL)
    print()
    for k, (b0, s0, b1, s1, norm, partial) in enumerate(first):
        r = R.case_reference(c, b0, s0)  # from the kernel's own float32 state: the bound does not compound over the calls
        assert R.bands_untouched(c, b1) and np.array_equal(_bits(b1["g"]), _bits(b0["g"]))
        assert all(np.isfinite(b1[role]).all() for role in R.ROLES)
        nch = len(c.chunk_tensor)
        assert (_bits(partial[:R.BAND]) == sent).all() and (_bits(partial[R.BAND + nch:]) == sent).all()
        assert np.isfinite(partial[R.BAND:R.BAND + nch]).all()  # exactly nchunks floats of it are written
        assert (_bits(norm[:R.BAND]) == sent).all() and (_bits(norm[R.BAND + 1:]) == sent).all()
        ratios = R.case_ratios(c, r, b1, s1, norm[R.BAND])
        for key, val in ratios.items():
            print("RATIO ttk_clip_adam", name if c.calls == 1 else f"{name}[{k}]", key, f"{val:.3f}")
        assert all(v <= 1.0 for v in ratios.values()), (name, k, ratios)
    # a second run from the same state, out_norm null: the same bits, and nothing lands where the norm would
    second, _ = _run(c, with_norm=False)
    # the guarded entry on the same (good) steps
    guarded, health = _run(c, guarded=True)
    for (_, _, b1, s1, norm, partial), (_, _, b2, s2, norm2, partial2), (_, _, b3, s3, norm3, partial3) in zip(first, second, guarded):
        for role in R.ROLES:
            assert np.array_equal(_bits(b1[role]), _bits(b2[role])) and np.array_equal(_bits(b1[role]), _bits(b3[role])), role
        assert np.array_equal(s1, s2) and np.array_equal(s1, s3)
        assert np.array_equal(_bits(partial), _bits(partial2)) and np.array_equal(_bits(partial), _bits(partial3))
        assert (_bits(norm2) == sent).all() and np.array_equal(_bits(norm), _bits(norm3))
    assert health == [HEALTH0[0], 0, HEALTH0[2], HEALTH0[3]]


REFUSALS = {"null_table": dict(ptrs=None), "no_chunks": dict(nchunks=0), "chunk_size_0": dict(chunk=0), "grad_scale_0": dict(grad_scale=0.0),
            "grad_scale_negative": dict(grad_scale=-1.0)}


@pytest.mark.parametrize("what", list(REFUSALS) + ["guarded_without_health"])
def test_refusals_change_nothing(what):
    import trackertraincode._hip as hip

    c = _case("no_gradient")
    d = _Call(c)
    b0, s0 = d.state()
    with pytest.raises(RuntimeError):
        if what == "guarded_without_health":
            hip.lib().call("ttk_clip_adam_guarded", *d.args(), None)
        else:
            hip.lib().call("ttk_clip_adam", *d.args(**REFUSALS[what]))
    b1, s1 = d.state()
    assert all(np.array_equal(_bits(b0[role]), _bits(b1[role])) for role in R.ROLES) and np.array_equal(s0, s1)
    assert (_bits(d.norm.cpu().numpy()) == _bits(R.SENTINEL)).all()
    assert d.health.cpu().tolist() == HEALTH0
