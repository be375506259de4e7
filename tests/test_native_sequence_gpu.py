"""The native launch sequence (MobileNet.set_sequence("native"): ttk_mobilenet_forward / ttk_mobilenet_backward, csrc/mobilenet_seq.hip) held to
the Python sequence it restates (backbones/mobilenet_v1.py, _mobilenet_bc.py) on the MI355X.  Host side: tests/test_native_sequence.py.

The yardstick is the Python sequence itself, on the same weights, buffers and input:
  * the launch list the plan describes equals the entry-point names the Python sequence passes through `lib.call`;
  * forward (features, running statistics, num_batches_tracked) bitwise;
  * gradients bitwise under TTK_DETERMINISTIC=1 (a worker process) and, in the default mode, bitwise for every tensor that three Python passes
    repeat bitwise, and within twice the Python passes' own largest pairwise distance elsewhere (float atomics; the factor 2: a maximum over
    three pairs underestimates the spread);
  * the whole training step, graph capture, the data-parallel hook, and the refusals.
Shapes: B = 3 at 129 x 129 and B = 2 at 65 x 65 (final map 3 x 3); widths 1.0 (every layer tuned), 0.5 (mixed) and 0.75 (every layer on the
any-channel-count family); BlurPool on and off."""
import copy
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

# (precision, widen_factor, blur, mode, B, H)
CASES = [("fp32", 1.0, False, "train", 3, 129), ("fp32", 0.5, False, "train", 3, 129), ("fp32", 0.75, False, "train", 3, 129),
         ("fp32", 1.0, True, "train", 2, 65), ("fp32", 0.75, True, "train", 2, 65), ("fp32", 1.0, False, "frozen", 2, 65),
         ("fp32", 0.5, True, "frozen", 2, 65), ("fp32", 1.0, False, "eval", 3, 129), ("fp32", 0.75, True, "eval", 2, 65),
         ("bf16-compute", 1.0, False, "train", 3, 129), ("bf16-compute", 1.0, True, "train", 2, 65), ("bf16-compute", 1.0, False, "frozen", 2, 65),
         ("bf16-compute", 1.0, False, "eval", 2, 65)]
_id = lambda c: f"{c[0]}-w{c[1]}-{'blur' if c[2] else 'plain'}-{c[3]}-B{c[4]}x{c[5]}"


def _mods():
    import trackertraincode._hip as H
    import trackertraincode.backbones.mobilenet_v1 as MB

    return MB, H


def make_backbone(wf=1.0, blur=False, precision="fp32", seed=0):
    """A backbone with non-trivial BatchNorm parameters and running statistics (the running means are the statistics pivots: part of the input)."""
    MB, _ = _mods()
    torch.manual_seed(seed)
    net = MB.MobileNet(num_classes=0, widen_factor=wf, use_blurpool=blur)
    for bn in net._bns():
        bn.weight.data.uniform_(0.5, 1.5)
        bn.bias.data.normal_(0, 0.1)
        bn.running_mean.normal_(0, 0.1)
        bn.running_var.uniform_(0.5, 1.5)
    return net.to(DEV).set_precision(precision).train()


def set_mode(net, mode):
    """train: batch statistics; frozen: every BatchNorm in eval mode with frozen affine parameters, convolutions trainable; eval."""
    net.train(mode == "train")
    for bn in net._bns():
        for q in bn.parameters():
            q.requires_grad_(mode == "train")
    return net


def one_pass(net, x, G, mode="train"):
    """One forward (+ backward of sum(feat * G)) -> {"feat", buffers, gradients}, cloned."""
    net.zero_grad(set_to_none=True)
    if mode == "eval":
        with torch.no_grad():
            feat = net.forward_features(x)
    else:
        feat = net.forward_features(x)
        (feat * G).sum().backward()
    torch.cuda.synchronize()
    out = {"feat": feat.detach().clone()}
    for k, v in net.state_dict().items():
        if "running_" in k or "num_batches" in k:
            out["buf:" + k] = v.clone()
    for k, q in net.named_parameters():
        if q.grad is not None:
            out["grad:" + k] = q.grad.clone()
    return out


def _inputs(net, B, H, seed=7):
    x = torch.randn(B, 1, H, H, generator=torch.Generator().manual_seed(seed)).to(DEV)
    G = torch.randn(B, net.num_features, generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
    return x, G


def _plan(net, B, H, mode, precision):
    MB, Hh = _mods()
    blur = net._blur_weights()
    return Hh.lib().mobilenet_plan(B, H, H, net.conv1.out_channels, tuple((cin, cout, s) for _, cin, cout, s in net._blocks),
                                   tuple(b is not None for b in blur) if blur is not None else (False,) * len(net._blocks), mode, precision,
                                   MB._DETERMINISTIC)


class _Recorded:
    """Names passing through lib.call while the block runs (as tests/test_bf16_compute_gpu.py wraps it)."""

    def __enter__(self):
        _, H = _mods()
        self.lib, self.names = H.lib(), []
        self.orig = self.lib.call
        self.lib.call = lambda name, *a: (self.names.append(name), self.orig(name, *a))[1]
        return self.names

    def __exit__(self, *exc):
        del self.lib.call  # back to the class's method
        return False


# ---- 1. order -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_described_launch_list_equals_the_python_sequence(case):
    precision, wf, blur, mode, B, H = case
    _, Hh = _mods()
    net = set_mode(make_backbone(wf, blur, precision), mode)
    x, G = _inputs(net, B, H)
    plan = _plan(net, B, H, mode, precision)
    L = Hh.lib()
    with _Recorded() as names:
        if mode == "eval":
            with torch.no_grad():
                net.forward_features(x)
            split = len(names)
        else:
            feat = net.forward_features(x)
            split = len(names)
            (feat * G).sum().backward()
        torch.cuda.synchronize()
    fwd, bwd = L.mobilenet_describe(plan, False), (L.mobilenet_describe(plan, True) if mode != "eval" else [])
    assert fwd == names[:split], [(i, a, b) for i, (a, b) in enumerate(zip(fwd, names[:split])) if a != b][:3]
    assert bwd == names[split:], [(i, a, b) for i, (a, b) in enumerate(zip(bwd, names[split:])) if a != b][:3]
    assert plan.launches[0] == len(fwd) and plan.launches[1] == len(bwd)
    if mode == "eval":
        assert L.cdll.ttk_mobilenet_describe(plan, 1, None, 0, None) != 0  # a forward-only plan has no backward list
    # a buffer that is too small is refused and reports what the list takes
    need = ctypes.c_size_t(0)
    small = ctypes.create_string_buffer(16)
    assert L.cdll.ttk_mobilenet_describe(plan, 0, small, 16, ctypes.byref(need)) == -1 and need.value == len("\n".join(fwd)) + 1


# ---- 2. forward, 4. gradients in the default mode -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_bitwise_and_gradients_within_the_python_spread(case):
    precision, wf, blur, mode, B, H = case
    MB, _ = _mods()
    net = set_mode(make_backbone(wf, blur, precision), mode)
    x, G = _inputs(net, B, H)
    start = copy.deepcopy(net.state_dict())

    def run(seq):
        net.load_state_dict(start)  # the same running statistics every pass: they are the statistics pivots, i.e. part of the input
        return one_pass(net.set_sequence(seq), x, G, mode)

    r = [run("python") for _ in range(3)]
    with _Recorded() as names:
        n = run("native")
    assert names == [], names[:4]  # the native pass issues nothing through the per-launch path
    assert net.set_sequence("python").effective_sequence() == "python"
    assert set(n) == set(r[0]) and torch.isfinite(n["feat"]).all()
    ngrads = 0
    for k in r[0]:
        if not k.startswith("grad:"):
            assert torch.equal(n[k], r[0][k]) and torch.equal(r[1][k], r[0][k]), k  # features, running_mean / running_var, num_batches_tracked
            continue
        ngrads += 1
        spread = max(float((r[i][k].double() - r[j][k].double()).norm()) for i, j in ((0, 1), (0, 2), (1, 2)))
        dist = float((n[k].double() - r[0][k].double()).norm())
        print(f"{k}: |n - r1| = {dist:.3e}, max |ri - rj| = {spread:.3e}, |r1| = {float(r[0][k].double().norm()):.3e}")
        if torch.equal(r[0][k], r[1][k]) and torch.equal(r[0][k], r[2][k]):
            assert torch.equal(n[k], r[0][k]), (k, dist)
        else:
            # float atomics: the tuned fp32 kernels, and the tuned stem's weight gradient, which the bf16-compute path shares with them; the
            # any-channel-count family and the bf16-compute path's own kernels have none
            assert (precision == "fp32" and wf != 0.75) or k == "grad:conv1.weight", k
            assert dist <= 2 * spread, (k, dist, spread)
    if mode == "train":
        assert ngrads == 3 + 6 * 13 and float(n["buf:bn1.num_batches_tracked"]) == float(start["bn1.num_batches_tracked"]) + 1
    elif mode == "frozen":
        assert ngrads == 1 + 2 * 13  # the convolutions only; BatchNorm is a fixed affine map
    else:
        assert ngrads == 0


# ---- 3. gradients and 5. the step, deterministic mode ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def det_worker():
    env = dict(os.environ, TTK_DETERMINISTIC="1")
    out = subprocess.run([sys.executable, os.path.join(REPO, "tests", "_native_sequence_worker.py"), REPO], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


def test_deterministic_gradients_are_bitwise_equal(det_worker):
    assert set(det_worker["grads"]) == {"fp32_w100", "fp32_w050", "fp32_blur", "bc_w100", "bc_blur"}
    assert all(bad == [] for bad in det_worker["grads"].values()), det_worker["grads"]


def test_deterministic_parameters_are_bitwise_equal_after_three_clipadam_steps(det_worker):
    py, nat = det_worker["step"]["python"], det_worker["step"]["native"]
    assert py["optimizer"] == "ClipAdam"
    assert py["losses"] == nat["losses"] and len(py["losses"]) == 3, (py["losses"], nat["losses"])
    assert py["state"] == nat["state"]


def _step_setup(seq, precision=None):
    from util import build_net, load_golden, make_batches, script_args, train_script

    S = train_script()
    _, meta = load_golden("model_default.npz")
    meta = dict(meta, B=8, split=5)
    net = build_net(meta, DEV).train()
    net.convnet.set_sequence(seq)
    if precision:
        net.convnet.set_precision(precision)
    crit, _ = S.setup_losses(script_args(meta["flags"]), net)
    opt, _ = S.create_optimizer(net, script_args(meta["flags"], epochs=20))
    return net, crit, opt, make_batches(meta, DEV)


def test_training_step_loss_is_bitwise_equal():
    import trackertraincode.train as train

    losses = {}
    for seq in ("python", "native"):
        net, crit, opt, batches = _step_setup(seq)
        out = train.training_step(net, batches, 150, crit)
        out["loss"].backward()
        opt.step()
        torch.cuda.synchronize()
        losses[seq] = out["loss"].detach().clone()
        assert all(torch.isfinite(q).all() for q in net.parameters())
    assert torch.equal(losses["python"], losses["native"]), losses


# ---- 6. capture -----------------------------------------------------------------------------------------------------------------------
def test_graphed_step_replays_the_native_sequence_bitwise(det_worker):
    """The library allocates nothing and never synchronises, its zero fills are memset nodes: the native step captures.  GraphedTrainStep runs
    its first step eagerly and captures then, so steps 2, 3 and 4 are replays: under TTK_DETERMINISTIC=1 (every reduction of the step in a fixed
    order) their losses are bitwise those of four eager native steps from the same start.  A zero fill or a callback that ran at capture time
    only would leave a stale BatchNorm bound or gradient arena behind and show here."""
    eager, graphed = det_worker["graph"]["eager"], det_worker["graph"]["graphed"]
    assert graphed["captures"] == 1 and not graphed["eager_only"] and graphed["has_graph"]
    assert len(eager["losses"]) == 4 and len(set(eager["losses"])) == 4
    assert graphed["losses"] == eager["losses"], (graphed["losses"], eager["losses"])
    assert eager["losses"][:3] == det_worker["step"]["native"]["losses"]


# ---- 7. hook --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,wf,blur", [("fp32", 0.75, False), ("bf16-compute", 1.0, True), ("fp32", 1.0, False)], ids=["anyc", "bc-blur", "tuned-det"])
def test_grad_ready_hook_fires_after_the_blocks_last_launch(monkeypatch, precision, wf, blur):
    """Both sequences announce the same parameter ranges in the same order.  A hook that halves each announced range in place (on the stream the
    launches went to) must leave exactly half of every gradient: a callback that fired before the block's last launch was enqueued would be
    overwritten or added to afterwards.  Halving is exact, so the comparison is bitwise: the backbone runs its fixed-order reductions (the
    any-channel-count family and the bf16-compute path have no others; the tuned fp32 kernels through the host's deterministic flag)."""
    MB, _ = _mods()
    monkeypatch.setattr(MB, "_DETERMINISTIC", True)
    B, H = 2, 65
    net = make_backbone(wf, blur, precision)
    x, G = _inputs(net, B, H)
    start = copy.deepcopy(net.state_dict())
    params = net._flat_params()

    def run(seq, hook):
        net.load_state_dict(start)
        monkeypatch.setattr(MB, "grad_ready_hook", hook)
        return one_pass(net.set_sequence(seq), x, G)

    plain = run("native", None)
    seen = {}

    def make_hook(key):
        seen[key] = []

        def hook(arena, entries):
            assert arena.dtype == torch.float32 and arena.dim() == 1
            seen[key].append([(next(i for i, q in enumerate(params) if q.data_ptr() == p_.data_ptr()), lo, hi) for p_, lo, hi in entries])
            for p_, lo, hi in entries:
                assert hi - lo == (p_.numel() + 63) // 64 * 64
            arena[entries[0][1]:entries[-1][2]].mul_(0.5)
        return hook

    halved = {seq: run(seq, make_hook(seq)) for seq in ("python", "native")}
    assert seen["native"] == seen["python"]
    firsts = [e[0][0] for e in seen["native"]]
    assert firsts == [3 + 6 * k for k in range(12, -1, -1)] + [0] and [len(e) for e in seen["native"]] == [6] * 13 + [3]
    for k, v in plain.items():
        if not k.startswith("grad:"):
            continue
        assert torch.equal(halved["native"][k], 0.5 * v), k
        assert torch.equal(halved["python"][k], 0.5 * v), k

    def boom(arena, entries):
        raise KeyError("from the hook")
    with pytest.raises(KeyError, match="from the hook"):  # an exception in the hook surfaces after the C call returned
        run("native", boom)


# ---- 8. refusal -----------------------------------------------------------------------------------------------------------------------
def test_refused_forward_launches_nothing():
    MB, Hh = _mods()
    L = Hh.lib()
    B, H = 2, 65
    net = make_backbone(0.5)
    x, _ = _inputs(net, B, H)
    plan = _plan(net, B, H, "train", "fp32")
    params, buffers = net._flat_params(), net._flat_buffers()
    before = [b.clone() for b in buffers]
    nan = float("nan")
    ws = torch.full((plan.ws_bytes[0] // 4,), nan, device=DEV).view(torch.uint8)
    feat = torch.full((B, net.num_features), nan, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    PA = lambda ts: (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])

    def call(plan=plan, params=params, nparams=None, buffers=buffers, ws_bytes=ws.numel(), xx=x, ff=feat):
        return L.cdll.ttk_mobilenet_forward(plan, None if xx is None else xx.data_ptr(), PA(params), len(params) if nparams is None else nparams,
                                            PA(buffers), len(buffers), None, 0.1, 1e-5, ws.data_ptr(), ws_bytes, None if ff is None else ff.data_ptr(), stream)

    def refused(rc, word):
        msg = L.cdll.ttk_last_error_string().decode()
        assert rc != 0 and word in msg, (rc, msg)
        torch.cuda.synchronize()
        assert torch.isnan(ws.view(torch.float32)).all() and torch.isnan(feat).all()
        assert all(torch.equal(a, b) for a, b in zip(before, buffers))

    refused(call(params=params[:40] + [None] + params[41:]), "params[40]")       # a null parameter pointer
    refused(call(ws_bytes=ws.numel() - 256), "workspace_bytes")                   # a workspace that is too small
    other = type(plan).from_buffer_copy(plan)                                                   # a block table changed after init
    other.cout[3] = 256
    refused(call(plan=other), "block table")
    refused(call(plan=_plan(make_backbone(1.0), B, H, "train", "fp32"), nparams=len(params)), "workspace")  # another width's plan: larger workspace
    refused(call(params=params[:-6], nparams=len(params) - 6), "nparams")         # a block short
    refused(call(buffers=buffers[:1] + [None] + buffers[2:]), "buffers[1]")
    refused(call(xx=None), "x and feat")
    blurred = _plan(make_backbone(0.5, blur=True), B, H, "train", "fp32")
    assert blurred.ws_bytes[0] >= plan.ws_bytes[0]
    big = torch.full((blurred.ws_bytes[0] // 4,), nan, device=DEV).view(torch.uint8)
    rc = L.cdll.ttk_mobilenet_forward(blurred, x.data_ptr(), PA(params), len(params), PA(buffers), len(buffers), None, 0.1, 1e-5, big.data_ptr(), big.numel(),
                                      feat.data_ptr(), stream)
    refused(rc, "blur_kernels")
    assert torch.isnan(big.view(torch.float32)).all()
    assert call() == 0  # ... and the same call with good arguments runs
    torch.cuda.synchronize()
    assert torch.isfinite(feat).all()


# ---- plan invariants (the size arithmetic asks the pointwise kernels for tilings that depend on the device: here, not in the CPU file) ----
def _python_allocations(fn):
    """Runs fn() and returns the (shape, dtype, bytes) of every torch.empty / torch.zeros it made."""
    made = []
    orig_e, orig_z = torch.empty, torch.zeros

    def rec(orig):
        def f(*a, **kw):
            t = orig(*a, **kw)
            made.append((tuple(t.shape), t.dtype, t.numel() * t.element_size()))
            return t
        return f
    torch.empty, torch.zeros = rec(orig_e), rec(orig_z)
    try:
        out = fn()
    finally:
        torch.empty, torch.zeros = orig_e, orig_z
    return out, made


@pytest.mark.parametrize("precision,wf,blur,mode,det", [("fp32", 1.0, False, "train", False), ("fp32", 0.5, True, "train", False), ("fp32", 0.75, False, "train", False),
                                                        ("fp32", 1.0, True, "train", True), ("fp32", 0.5, False, "frozen", False), ("fp32", 0.75, True, "train", True),
                                                        ("bf16-compute", 1.0, False, "train", False), ("bf16-compute", 1.0, True, "train", True)],
                         ids=lambda v: str(v))
def test_plan_sub_buffers_are_aligned_disjoint_and_sized_like_the_python_tensors(monkeypatch, precision, wf, blur, mode, det):
    MB, Hh = _mods()
    from trackertraincode.backbones import _mobilenet_bc as BC

    monkeypatch.setattr(MB, "_DETERMINISTIC", det)
    B, H = 3, 129
    net = set_mode(make_backbone(wf, blur, precision), mode)
    x, G = _inputs(net, B, H)
    plan = _plan(net, B, H, mode, precision)
    al = lambda v: (v + 255) // 256 * 256
    for w in (0, 1):
        n = plan.nbuf[w]
        spans = sorted((plan.buf_off[w][i], plan.buf_bytes[w][i]) for i in range(n))
        assert all(o % 256 == 0 and s > 0 for o, s in spans)
        assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= plan.ws_bytes[w]
        assert plan.ws_bytes[w] == sum(al(s) for _, s in spans)
    size = lambda w, i: 0 if i < 0 else plan.buf_bytes[w][i]
    params, buffers = [q.detach() for q in net._flat_params()], net._flat_buffers()
    bufs = [b.clone() for b in buffers]
    frozen = mode == "frozen"
    if precision == "fp32":
        (feat, c), _ = _python_allocations(lambda: MB._forward_impl(x, params, bufs, 0.1, 1e-5, training=not frozen, frozen=frozen, blur=net._blur_weights(), blocks=net._blocks))
    else:
        (feat, c), _ = _python_allocations(lambda: BC.forward_impl(MB, x, params, bufs, 0.1, 1e-5, training=not frozen, frozen=frozen, blur=net._blur_weights()))
    nb = lambda t: 0 if t is None else t.numel() * t.element_size()
    # the forward workspace: everything _Ctx keeps alive
    assert size(0, plan.i_part) == nb(c.part)
    assert size(0, plan.i_bn) == 4 * 8 * (net.conv1.out_channels + sum(cin + cout for _, cin, cout, _ in net._blocks))
    assert size(0, plan.i_prep) == sum(nb(t) for t in c.prep) and [plan.prep_bytes[k] for k in range(13)] == [nb(t) for t in c.prep]
    assert size(0, plan.i_y0) == nb(c.stages[0].y)
    for k in range(13):
        assert size(0, plan.i_ydw[k]) == nb(c.stages[2 * k + 1].y) and size(0, plan.i_ypw[k]) == nb(c.stages[2 * k + 2].y), k
        assert size(0, plan.i_ain[k]) == nb(c.a_in[k]), k
        assert size(0, plan.i_t[k]) == (nb(c.blur[k][0].y) if c.blur[k] is not None else 0) and size(0, plan.i_idbn[k]) == (nb(c.blur[k][0].bn) if c.blur[k] is not None else 0)
    assert plan.nbuf[0] == 4 - (plan.i_prep < 0) + sum((plan.i_ain[k] >= 0) + 2 * (plan.i_t[k] >= 0) + 2 for k in range(13))
    # the backward workspace: the gradient activations (two alternating buffers, one behind the pointwise layer, one behind a blur) and the scratch
    gfeat = torch.randn_like(feat)
    back = (lambda: MB._backward_impl(c, gfeat, params)) if precision == "fp32" else (lambda: BC.backward_impl(MB, c, gfeat, params))
    _, made = _python_allocations(back)
    arena = [m for m in made if len(m[0]) == 1 and m[1] == torch.float32][0]
    assert arena[2] == 4 * plan.arena_floats
    acts = [m[2] for m in made if len(m[0]) == 4]
    scratch = sorted(m[2] for m in made if len(m[0]) == 1 and m is not arena and m[2] > 0)
    assert scratch == sorted(s for s in (size(1, plan.i_wg), size(1, plan.i_pw), size(1, plan.i_dwrows), size(1, plan.i_any)) if s)
    it = iter(acts)
    gsz, gdw, gt = [0, 0], 0, 0
    gsz[12 & 1] = next(it)
    for k in range(12, -1, -1):
        gdw = max(gdw, next(it))
        gsz[(k + 1) & 1] = max(gsz[(k + 1) & 1], next(it))
        if c.blur[k] is not None:  # (allocated inside the blur branch, after the block input's gradient)
            gt = max(gt, next(it))
    assert next(it, None) is None
    assert [size(1, plan.i_g[0]), size(1, plan.i_g[1]), size(1, plan.i_gdw), size(1, plan.i_gt)] == [gsz[0], gsz[1], gdw, gt]
    assert Hh.lib().cdll.ttk_mobilenet_forward_workspace_bytes(plan) == plan.ws_bytes[0] and Hh.lib().cdll.ttk_mobilenet_backward_workspace_bytes(plan) == plan.ws_bytes[1]
