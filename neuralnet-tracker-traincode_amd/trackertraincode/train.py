"""Loss plumbing, optimiser, schedules and the training loop (reference: trackertraincode/train.py and
the Lightning pieces of scripts/train_poseestimator.py).

Same public names as the reference for what the hot path uses: LossVal, Criterion, CriterionGroup,
concatenated_lossvals_by_name, default_compute_loss, ExponentialUpThenSteps, LinearUpThenSteps,
SwaCallback.  pytorch-lightning is replaced by `fit()` below, which reproduces the step order the
reference gets from `pl.Trainer(gradient_clip_val=1.0, gradient_clip_algorithm="norm")`:
zero_grad -> forward -> loss -> backward -> global-norm clip -> Adam, LR scheduler stepped per epoch,
SWA update per epoch after `start_epoch`.  The clip+Adam pair is one fused HIP entry point
(`ClipAdam`, csrc/adam.hip).

Difference on purpose: `default_compute_loss` does NOT copy the per-sample loss vectors to the host
and does NOT synchronise the stream every step (reference :433-438); the returned LossVals hold
detached DEVICE tensors (call .cpu() when you want them).
"""
from __future__ import annotations

import ctypes
import functools
import itertools
import math
import os
from collections import defaultdict
from typing import Any, Callable, List, NamedTuple, Union

import torch
import torch.nn as nn
from torch import Tensor
from torch.optim.lr_scheduler import LambdaLR

from . import _hip
from .datasets.batch import Batch, Metadata
from .neuralnets.io import save_model


class LossVal(NamedTuple):
    val: Tensor
    weight: Any
    name: str


class SampleWeight:
    """Per-sample weight of one loss term, `scalar * dataset_weight` (or the scalar broadcast over the sub-batch) -
    what the reference stores as a tensor in `LossVal.weight` after default_compute_loss (:404-412).  The tensor is
    only built when something reads it (`.tensor()`, or arithmetic with a tensor): the training step itself feeds
    (scalar, per_sample) to one fused weighted-sum kernel instead of launching a fill or multiply per term."""

    __slots__ = ("scalar", "per_sample", "_like", "_t")

    def __init__(self, scalar: float, per_sample: Tensor | None, like: Tensor):
        self.scalar, self.per_sample, self._like, self._t = float(scalar), per_sample, like, None

    def tensor(self) -> Tensor:
        if self._t is None:
            like = self._like
            self._t = like.new_full(like.shape, self.scalar) if self.per_sample is None else self.scalar * self.per_sample
        return self._t

    def __mul__(self, other):
        return self.tensor() * other

    __rmul__ = __mul__

    @property
    def shape(self):
        return self._like.shape


def _as_weight_tensor(w):
    return w.tensor() if isinstance(w, SampleWeight) else w


def _concat_groups(groups: dict):
    """{name: [1-D tensors]} -> {name: concatenation}; on the GPU all groups land in one buffer with one launch."""
    flat = [t for ts in groups.values() for t in ts]
    if not flat or not all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 1 and not t.requires_grad for t in flat):
        return {k: torch.concat(ts) for k, ts in groups.items()}
    flat = [t.contiguous() for t in flat]
    buf = torch.empty(sum(t.numel() for t in flat), dtype=torch.float32, device=flat[0].device)
    _hip.lib().multi_copy(flat, list(torch.split(buf, [t.numel() for t in flat])))
    return dict(zip(groups.keys(), torch.split(buf, [sum(t.numel() for t in ts) for ts in groups.values()])))


def concatenated_lossvals_by_name(vals):
    """{name: (values, weights)} concatenated over sub-batches, first-seen order (reference :47-62)."""
    values, weights = defaultdict(list), defaultdict(list)
    for v in vals:
        values[v.name].append(v.val)
        weights[v.name].append(_as_weight_tensor(v.weight))
    values = _concat_groups(values)
    return {k: (values[k], torch.concat(weights[k])) for k in values}


def concatenated_values_by_name(vals):
    """{name: values} only - what the training step logs (no weight tensors are built)."""
    values = defaultdict(list)
    for v in vals:
        values[v.name].append(v.val)
    return _concat_groups(values)


def _split_predictions(preds: dict, sizes):
    """Per sub-batch {key: rows of preds[key]}.  float32 GPU tensors (and the rotation containers around them) are
    split by ONE autograd node whose backward assembles all gradients with a single launch."""
    from .neuralnets import _hipops

    def tensor_of(v):
        t = v if isinstance(v, Tensor) else getattr(v, "value", None)
        ok = isinstance(t, Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() >= 1
        return t if ok else None

    fused = {k: tensor_of(v) for k, v in preds.items()}
    fused = {k: t for k, t in fused.items() if t is not None}
    pieces = _hipops.SplitRowsFn.apply(tuple(sizes), *fused.values()) if fused else ()
    out, offset = [], 0
    for i, n in enumerate(sizes):
        sub = {}
        for k, v in preds.items():
            if k in fused:
                piece = pieces[list(fused).index(k) * len(sizes) + i]
                sub[k] = piece if isinstance(v, Tensor) else type(v)(piece)
            else:
                sub[k] = v[offset:offset + n, ...]
        out.append(sub)
        offset += n
    return out


def _weight_at(w, step):
    return w if isinstance(w, float) else w(step)


class Criterion(NamedTuple):
    name: str
    f: Callable[[Any, Any], Tensor]
    w: Union[float, Callable[[int], float]]

    def evaluate(self, pred, batch, step) -> List[LossVal]:
        return [LossVal(self.f(pred, batch), _weight_at(self.w, step), self.name)]


class CriterionGroup(NamedTuple):
    criterions: List[Union["CriterionGroup", Criterion]]
    name: str = ""
    w: Union[float, Callable[[int], float]] = 1.0

    def evaluate(self, pred, batch, step) -> List[LossVal]:
        w = _weight_at(self.w, step)
        out = []
        for c in self.criterions:
            out += [LossVal(v.val, v.weight * w, self.name + v.name) for v in c.evaluate(pred, batch, step)]
        return out


def default_compute_loss(preds: dict, batch: List[Batch], current_epoch: int, loss):
    """(loss_sum, per-sub-batch lists of LossVal) - reference :372-439.

    Sub-batches are addressed by integer offsets into the concatenated predictions; weights become
    per-sample tensors (scaled by `dataset_weight` when the sub-batch has one); the sum is divided by
    the TOTAL batch size so that a loss a sub-batch does not have counts as zero."""
    from .neuralnets import _hipops

    sizes = [subset.meta.prefixshape[0] for subset in batch]
    split = _split_predictions(preds, sizes)

    def evaluate_all():
        out: list[list[LossVal]] = []
        for subset, subpreds in zip(batch, split):
            crit = loss[subset.meta.tag] if isinstance(loss, dict) else loss
            terms = crit.evaluate(subpreds, subset, current_epoch)
            dw = None
            if "dataset_weight" in subset:
                dw = subset["dataset_weight"]
                assert dw.size(0) == subset.meta.batchsize
            out.append([v._replace(weight=SampleWeight(v.weight, dw, v.val)) for v in terms])
        return out

    # the criterions' HIP kernels are independent of one another: their launches are collected and issued as ONE
    # (neuralnets/_hipops.py: loss_batch / apply / BatchedLossFn), forward here and backward in BatchedLossFn.backward
    with _hipops.loss_batch() as lb:
        all_lossvals = evaluate_all()
    returned = {id(v.val) for terms in all_lossvals for v in terms}
    if any(id(r[3]) not in returned for r in lb.records):
        # A criterion did arithmetic on a deferred per-sample value (scaled it, sliced it, added two losses: the reference's
        # Criterion accepts any callable) - that read memory the batch had not filled yet, and the term would get no gradient.
        # Nothing was launched so far: throw the deferred pass away and evaluate every term with one launch per loss op.
        _warn_once("a Criterion post-processes the value of a batched loss kernel; this step's losses run unbatched "
                   "(wrap the arithmetic into the loss function's autograd to silence this)")
        lb.ops.clear()
        lb.records.clear()
        lb.keep.clear()
        with _hipops.unbatched():
            all_lossvals = evaluate_all()
    batchsize = sum(subset.meta.batchsize for subset in batch)
    flat = list(itertools.chain.from_iterable(all_lossvals))
    if flat and all(v.val.is_cuda and v.val.dtype == torch.float32 for v in flat):
        loss_sum = _batched_loss_sum(lb, flat, 1.0 / batchsize)
    else:  # host-side logic on CPU tensors (tests); the reference's formula
        lb.flush()
        by_name = concatenated_lossvals_by_name(flat)
        loss_sum = torch.concat([v * w for v, w in by_name.values()]).sum() / batchsize
    all_lossvals = [[v._replace(val=v.val.detach()) for v in terms] for terms in all_lossvals]
    return loss_sum, all_lossvals


_WARNED: set = set()


def _warn_once(msg):
    if msg not in _WARNED:
        _WARNED.add(msg)
        import warnings
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


def _batched_loss_sum(lb, flat, scale):
    """The weighted sum over all terms; the terms whose kernels were deferred into `lb` go through BatchedLossFn together."""
    from .neuralnets import _hipops
    by_val = {id(r[3]): r for r in lb.records}
    deferred = [v for v in flat if id(v.val) in by_val]
    ordinary = [v for v in flat if id(v.val) not in by_val]
    if not deferred:
        lb.flush()
        return _hipops.WeightedSumFn.apply([v.weight.scalar for v in flat], [v.weight.per_sample for v in flat], scale, *[v.val for v in flat])
    records = [by_val[id(v.val)] for v in deferred]
    assert len(records) == len(lb.records), "a deferred loss term was dropped"  # (default_compute_loss re-evaluates unbatched before this can happen)
    inputs, index, slots = [], {}, []
    for _fn, _ctx, args, _v in records:  # the distinct differentiable inputs of the deferred terms
        sl = []
        for pos, a in enumerate(args):
            if isinstance(a, Tensor) and a.requires_grad:
                if id(a) not in index:
                    index[id(a)] = len(inputs)
                    inputs.append(a)
                sl.append((pos, index[id(a)]))
        slots.append(sl)
    order = deferred + ordinary
    return _hipops.BatchedLossFn.apply(lb, records, slots, [v.weight.scalar for v in order], [v.weight.per_sample for v in order], scale,
                                       len(inputs), *inputs, *[v.val for v in ordinary])


# ---------------------------------------------------------------------------------------------
# learning-rate schedules (reference :577-629)
# ---------------------------------------------------------------------------------------------
def _step_factor(i, gamma, steps):
    return gamma ** [j for j, s in enumerate([0] + list(steps)) if i > s][-1]


def LinearUpThenSteps(optimizer, num_up, gamma, steps):
    return LambdaLR(optimizer, lambda i: (i + 1) / num_up if i < num_up else _step_factor(i, gamma, steps))


def ExponentialUpThenSteps(optimizer, num_up, gamma, steps):
    """0.01 -> 1 exponentially over `num_up` epochs, then gamma^k after the k-th step epoch."""
    eps = 1.0e-2

    def factor(i):
        if i < num_up:
            return eps * math.exp(-math.log(eps) * (i + 1) / num_up)
        return _step_factor(i, gamma, steps)

    return LambdaLR(optimizer, factor)


# ---------------------------------------------------------------------------------------------
# fused clip + Adam
# ---------------------------------------------------------------------------------------------
class ClipAdam(torch.optim.Optimizer):
    """torch.optim.Adam semantics (betas, eps, L2 weight_decay, per-group lr, per-parameter step counts) preceded by
    clip_grad_norm_(all params, max_norm) - one C-ABI call, two kernel launches, no host sync.
    State layout matches torch.optim.Adam (`step`, `exp_avg`, `exp_avg_sq`); the step counts live on the device (the
    kernel advances them), so a step can be captured in a hipGraph and `state_dict()` / `load_state_dict()` resume
    exactly.  `grad_scale` (default 1): the stored gradients are read as grad_scale * g - 1/world when a
    data-parallel all-reduce left sums in place (trackertraincode.parallel).

    `skip_nonfinite=True`: the step runs `ttk_clip_adam_guarded`.  A step whose total gradient norm is not finite (a NaN or Inf anywhere
    in the gradients, or a finite gradient whose squared norm overflows float32) changes neither parameters nor moments nor step counts;
    the kernel decides this on the device, so the step still has no host synchronisation and still captures in a hipGraph.  `health()`
    reads the device counters (one device read: call it per epoch, never per step).  The guard protects the weights and the optimiser
    state only: BatchNorm running statistics that a non-finite forward has already written stay written, and the backbone kernels treat
    non-finite inputs as before.  A good step is bitwise the unguarded step."""

    MAX_GROUPS = 128  # TTK_ADAM_MAX_GROUPS (prepare_finetune() of the default backbone returns 66, one per backbone sub-module)
    CHUNK = 4096  # elements per workgroup: ~800 workgroups for the 3.2 M parameters (16384 left most of the 256 CUs idle)

    def __init__(self, params, lr=1.0e-3, betas=(0.9, 0.999), eps=1.0e-8, weight_decay=0.0, max_norm: float | None = 1.0,
                 skip_nonfinite: bool = False):
        # capturable: torch then keeps a loaded `step` as a float32 tensor on the parameter's device
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=True))
        self.param_groups = [g for g in self.param_groups]
        if len(self.param_groups) > self.MAX_GROUPS:
            raise ValueError(f"ClipAdam supports at most {self.MAX_GROUPS} parameter groups")
        if len({(g["betas"], g["eps"]) for g in self.param_groups}) != 1:
            raise ValueError("all groups must share betas and eps")
        self.max_norm = max_norm
        self.grad_scale = 1.0
        self.skip_nonfinite = bool(skip_nonfinite)
        self._health_host = [0, 0, -1]  # (skipped, consecutive, culprit) the device block starts from when the tables are (re)built
        self._tables = None
        self._uploaded = None      # gradient addresses the device table currently holds
        self._upload_event = None  # recorded behind the last upload of the pinned table
        self._t = 0                # optimiser steps taken (host-side count; the per-parameter counts are state[p]["step"])
        self.last_grad_norm: Tensor | None = None

    def _invalidate(self):
        T = getattr(self, "_tables", None)
        if T is not None and T.get("health") is not None:  # the counters outlive the device tables (one device read: rare)
            self._health_host = T["health"][:3].tolist()
        self._tables, self._uploaded, self._upload_event = None, None, None

    def health(self) -> dict:
        """{"skipped", "consecutive", "culprit_index"} of a `skip_nonfinite` optimiser: bad steps so far, bad steps since the last good one,
        and the index (in the order of the parameter groups' parameters) of the first tensor with a non-finite gradient in the most recent
        bad step, -1 before any.  One device read, which waits for the steps enqueued so far."""
        if not self.skip_nonfinite:
            raise RuntimeError("ClipAdam.health(): the optimiser was built without skip_nonfinite=True")
        T = self._tables
        h = T["health"][:3].tolist() if T is not None else list(self._health_host)
        return {"skipped": int(h[0]), "consecutive": int(h[1]), "culprit_index": int(h[2])}

    def load_health(self, health: dict):
        """Restore the counters `health()` returned (resume)."""
        self._health_host = [int(health["skipped"]), int(health["consecutive"]), int(health["culprit_index"])]
        if self._tables is not None and self._tables.get("health") is not None:
            self._tables["health"][:3] = torch.tensor(self._health_host, dtype=torch.int32)

    def parameter_at(self, index: int):
        """The parameter behind a `culprit_index`."""
        return [p for g in self.param_groups for p in g["params"]][index]

    def load_state_dict(self, state_dict):
        """Resume: the loaded moments / step counts replace the live ones, so every cached device address is stale."""
        super().load_state_dict(state_dict)
        self._invalidate()
        steps = [float(st["step"]) for st in self.state.values() if "step" in st]
        self._t = int(max(steps)) if steps else 0

    def __setstate__(self, state):
        super().__setstate__(state)
        self._invalidate()

    def _build_tables(self):
        plist, groups = [], []
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                    raise RuntimeError("ClipAdam needs contiguous float32 CUDA parameters")
                plist.append(p)
                groups.append(gi)
        dev = plist[0].device
        # per-parameter step counts in ONE device array; state[p]["step"] are views of it (what torch.optim.Adam keeps per
        # parameter, and what state_dict() saves)
        steps = torch.zeros(len(plist), dtype=torch.float32, device=dev)
        for ti, p in enumerate(plist):
            st = self.state[p]
            if "step" in st:
                steps[ti] = float(st["step"])  # only after load_state_dict: rare
            st["step"] = steps[ti]
            for key in ("exp_avg", "exp_avg_sq"):
                if key not in st:
                    st[key] = torch.zeros_like(p)
                elif not (st[key].is_cuda and st[key].dtype == torch.float32 and st[key].is_contiguous()):
                    st[key] = st[key].to(device=dev, dtype=torch.float32).contiguous()
        ct, co = [], []
        for ti, p in enumerate(plist):
            for off in range(0, p.numel(), self.CHUNK):
                ct.append(ti)
                co.append(off)
        i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
        self._tables = dict(
            params=plist, numel=i32([p.numel() for p in plist]), group=i32(groups), chunk_tensor=i32(ct), chunk_offset=i32(co),
            nchunks=len(ct), ptrs_host=torch.zeros((len(plist), 4), dtype=torch.int64).pin_memory(),
            ptrs=torch.zeros((len(plist), 4), dtype=torch.int64, device=dev), steps=steps,
            partial=torch.empty(len(ct), dtype=torch.float32, device=dev), norm=torch.zeros(1, dtype=torch.float32, device=dev),
            hyper=torch.zeros(2 * self.MAX_GROUPS, dtype=torch.float32, device=dev),  # TTK_ADAM_HYPER_* block (include/ttk.h)
            # TTK_ADAM_HEALTH_* block of the guarded entry point
            health=torch.tensor(list(self._health_host) + [0] * (_hip.ADAM_HEALTH_WORDS - 3), dtype=torch.int32, device=dev) if self.skip_nonfinite else None,
        )
        h = self._tables["ptrs_host"]
        for ti, p in enumerate(plist):
            st = self.state[p]
            h[ti, 0], h[ti, 2], h[ti, 3] = p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
        self._uploaded = None

    def _upload_grad_pointers(self, T, capturing):
        """The device table of (param, grad, exp_avg, exp_avg_sq) addresses.  Only the gradient column ever changes, and
        only when the allocator hands out new addresses; the pinned staging table is rewritten only after the previous
        asynchronous upload has read it (a host that runs several steps ahead of the GPU would otherwise overwrite the
        addresses of a step that has not been copied yet)."""
        gptrs = []
        for p in T["params"]:
            g = p.grad
            if g is not None and not g.is_contiguous():
                g = p.grad = g.contiguous()
            gptrs.append(0 if g is None else g.data_ptr())
        gptrs = tuple(gptrs)
        if gptrs == self._uploaded:
            return
        if self._upload_event is not None and not capturing:
            self._upload_event.synchronize()
        T["ptrs_host"][:, 1] = torch.tensor(gptrs, dtype=torch.int64)
        T["ptrs"].copy_(T["ptrs_host"], non_blocking=True)
        if not capturing:
            self._upload_event = torch.cuda.Event()
            self._upload_event.record()
        self._uploaded = gptrs

    @torch.no_grad()
    def step(self, closure=None):
        assert closure is None
        if self._tables is None:
            self._build_tables()
        T = self._tables
        capturing = torch.cuda.is_current_stream_capturing()
        self._upload_grad_pointers(T, capturing)
        b1, b2 = self.param_groups[0]["betas"]
        G = self.MAX_GROUPS
        lr4 = (ctypes.c_float * G)(*([g["lr"] for g in self.param_groups] + [0.0] * G)[:G])
        wd4 = (ctypes.c_float * G)(*([g["weight_decay"] for g in self.param_groups] + [0.0] * G)[:G])
        p_ = _hip.ptr
        # inside a hipGraph capture nothing of the step may be baked into launch arguments: learning rates and weight
        # decays are read from the device block `hyper` (the step counts always live on the device)
        hyper = p_(T["hyper"]) if capturing else None
        args = (p_(T["ptrs"]), p_(T["numel"]), p_(T["group"]), p_(T["chunk_tensor"]), p_(T["chunk_offset"]),
                T["nchunks"], self.CHUNK, lr4, wd4, b1, b2, self.param_groups[0]["eps"], float(self.max_norm or 0.0),
                float(self.grad_scale), p_(T["steps"]), p_(T["partial"]), p_(T["norm"]), hyper)
        if self.skip_nonfinite:
            _hip.lib().call("ttk_clip_adam_guarded", *args, p_(T["health"]))
        else:
            _hip.lib().call("ttk_clip_adam", *args)
        if not capturing:
            self._t += 1
        self.last_grad_norm = T["norm"]
        return None

    def _hyper_values(self):
        G = self.MAX_GROUPS
        return ([g["lr"] for g in self.param_groups] + [0.0] * G)[:G] + ([g["weight_decay"] for g in self.param_groups] + [0.0] * G)[:G]

    # ---- hipGraph support -----------------------------------------------------------------------
    def sync_hyper_to_device(self):
        """Write the groups' lr / weight_decay into the device block a captured step reads.  Called before a capture and
        whenever the scheduler changed a learning rate (once per epoch)."""
        if self._tables is None:
            self._build_tables()
        vals = self._hyper_values()
        self._tables["hyper"].copy_(torch.tensor(vals, dtype=torch.float32))  # synchronous, pageable: rare
        self._hyper_sig = tuple(vals)

    def before_graph_replay(self):
        """Push a changed learning rate / weight decay (scheduler step) to the device block before the replay."""
        vals = tuple(self._hyper_values())
        if vals != getattr(self, "_hyper_sig", None):
            torch.cuda.current_stream().synchronize()  # earlier replays still read the old values
            self.sync_hyper_to_device()

    def after_graph_replay(self):
        """Host-side bookkeeping of one replayed step (the device counters were advanced by the graph)."""
        self._t += 1


# ---------------------------------------------------------------------------------------------
# stochastic weight averaging (reference SwaCallback :447-467)
# ---------------------------------------------------------------------------------------------
class SwaCallback:
    """Equal-weight running average of parameters AND buffers (AveragedModel(use_buffers=True)),
    updated once per epoch for epochs > start_epoch, kept on the CPU, saved as swa.ckpt."""

    def __init__(self, start_epoch):
        self._start_epoch = start_epoch
        self._swa_model = None
        self.n_averaged = 0

    @property
    def swa_model(self):
        return self._swa_model

    def on_train_start(self, model: nn.Module):
        import copy

        self._swa_model = copy.deepcopy(model).to("cpu")

    @torch.no_grad()
    def on_train_epoch_end(self, epoch: int, model: nn.Module):
        if epoch <= self._start_epoch:
            return
        avg, new = self._swa_model.state_dict(), model.state_dict()
        for k, a in avg.items():
            b = new[k].detach().to("cpu")
            if self.n_averaged == 0:
                a.copy_(b)
            elif a.is_floating_point():
                a.add_((b - a) / (self.n_averaged + 1))
            else:
                a.copy_(a + torch.div(b - a, self.n_averaged + 1, rounding_mode="trunc"))
        self.n_averaged += 1

    def on_train_end(self, root_dir: str):
        assert self._swa_model is not None
        save_model(self._swa_model, os.path.join(root_dir, "swa.ckpt"))

    def state_dict(self) -> dict:
        sd = None if self._swa_model is None else {k: v.detach().clone() for k, v in self._swa_model.state_dict().items()}
        return {"n_averaged": int(self.n_averaged), "swa_model": sd}

    def load_state_dict(self, state: dict):
        """After `on_train_start` (which makes the averaged model as a copy of the live one): the average so far replaces that copy."""
        if state["swa_model"] is not None:
            if self._swa_model is None:
                raise RuntimeError("SwaCallback.load_state_dict: call on_train_start(model) first - it creates the averaged model")
            self._swa_model.load_state_dict(state["swa_model"])
        self.n_averaged = int(state["n_averaged"])


# ---------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------
def _concat_rows(tensors):
    """torch.concat(tensors, dim=0) - as a VIEW when the tensors already lie back to back in one allocation (the static inputs of
    GraphedTrainStep are laid out that way: at B = 512 the copy of the images alone is 34 MB read + 34 MB written per step)."""
    t0 = tensors[0]
    if len(tensors) == 1:
        return t0
    adjacent = all(t.is_contiguous() and not t.requires_grad and t.dtype == t0.dtype and t.shape[1:] == t0.shape[1:] for t in tensors)
    if adjacent:
        base = t0.untyped_storage().data_ptr()
        end = t0.data_ptr()
        for t in tensors:
            adjacent = adjacent and t.untyped_storage().data_ptr() == base and t.data_ptr() == end
            end = t.data_ptr() + t.numel() * t.element_size()
    if not adjacent:
        return torch.concat(tensors, dim=0)
    rows = sum(int(t.shape[0]) for t in tensors)
    return torch.as_strided(t0, (rows,) + tuple(t0.shape[1:]), t0.stride())


def training_step(model: nn.Module, batches: List[Batch], epoch: int, criterions):
    """LitModel.training_step (scripts/train_poseestimator.py:310-330) without the logging."""
    if batches[0]["image"].is_cuda:
        _hip.lib().clear_stale_error("the start of a training step")  # once per step (the launches themselves no longer do it)
    inputs = _concat_rows([b["image"] for b in batches])
    ids = _concat_rows([b["coord_convention_id"] for b in batches])
    preds = model(inputs, ids)
    loss_sum, all_lossvals = default_compute_loss(preds, batches, epoch, criterions)
    by_name = concatenated_values_by_name(itertools.chain.from_iterable(all_lossvals))
    return {"loss": loss_sum, "mt_losses": by_name}


# ---------------------------------------------------------------------------------------------
# the step over ALL rows with per-row Tag codes ("flat" layout): launch arguments independent of the per-Tag split
# ---------------------------------------------------------------------------------------------
def _tag_code(tag) -> int:
    code = int(getattr(tag, "value", tag))
    if not 0 <= code < 32:
        raise ValueError(f"Tag code {code} of {tag}: the row-liveness kernels take codes 0..31")
    return code


def flatten_batches(batches: List[Batch], fill: float = 0.0) -> Batch:
    """The sub-batches of one step as ONE batch of B rows in sub-batch order.  Every tensor field becomes [B, ...]; rows whose
    sub-batch lacks the field hold `fill` (0 in integer fields).  Added: `tag_code` (int32 [B], the value of each row's Tag) and
    `dataset_weight` (float32 [B], 1 where a sub-batch had none).  Raises ValueError when the trailing shape or the dtype of a field
    differs between sub-batches.  Works on CPU tensors too."""
    if not batches:
        raise ValueError("flatten_batches: no sub-batches")
    sizes = [int(b.meta.prefixshape[0]) for b in batches]
    B = sum(sizes)
    spec: dict = {}
    for b in batches:
        for k, v in b.items():
            if not torch.is_tensor(v):
                continue
            cur = (tuple(v.shape[1:]), v.dtype)
            if spec.setdefault(k, cur) != cur:
                raise ValueError(f"flatten_batches: field {k!r} is {cur[0]} {cur[1]} in {b} but {spec[k][0]} {spec[k][1]} in an earlier sub-batch")
    device = next(v for v in batches[0].values() if torch.is_tensor(v)).device
    out = {}
    for k, (trail, dtype) in spec.items():
        if k == "dataset_weight":
            continue
        if all(k in b for b in batches):
            out[k] = torch.concat([b[k] for b in batches], dim=0)
            continue
        full = torch.full((B,) + trail, fill if dtype.is_floating_point else 0, dtype=dtype, device=device)
        off = 0
        for b, n in zip(batches, sizes):
            if k in b:
                full[off:off + n] = b[k]
            off += n
        out[k] = full
    out["tag_code"] = torch.concat([torch.full((n,), _tag_code(b.meta.tag), dtype=torch.int32) for b, n in zip(batches, sizes)]).to(device)
    out["dataset_weight"] = torch.concat([b["dataset_weight"].to(torch.float32).reshape(n) if "dataset_weight" in b
                                          else torch.ones(n, dtype=torch.float32, device=device) for b, n in zip(batches, sizes)])
    return Batch(Metadata(batches[0].meta._imagesize, batchsize=B, tag=None), out)


class LossTerm(NamedTuple):
    """One row of the flat term table: a criterion callable, its name (group prefixes included) and, per Tag whose criterion table
    holds it, the weights along its path (innermost first; floats or functions of the epoch)."""
    name: str
    f: Callable[[Any, Any], Tensor]
    paths: dict

    @property
    def tags(self):
        return tuple(self.paths)

    @property
    def tag_set(self) -> int:
        m = 0
        for t in self.paths:
            m |= 1 << _tag_code(t)
        return m

    def weight(self, tag, epoch) -> float:
        """The product Criterion.evaluate / CriterionGroup.evaluate form for a sub-batch of `tag` at `epoch` (same order of the factors)."""
        ws = [_weight_at(w, epoch) for w in self.paths[tag]]
        out = ws[0]
        for w in ws[1:]:
            out = out * w
        return out


def loss_terms(criterions: dict) -> List[LossTerm]:
    """The flat term table of a {Tag: CriterionGroup} dict: one term per distinct (name, criterion callable).  Two Criterions that
    share a name but not the callable (Points3dLoss in 3D and in 2.5D) are two terms.  Order: first seen, walking the Tags' tables
    from the one with the most terms down (ties in dict order) - the names then come out in the order concatenated_lossvals_by_name
    gives for a step whose first sub-batch has the richest Tag, which is how the reference's loaders and goldens order them (a table
    alone cannot know the order of a step's sub-batches)."""
    if not isinstance(criterions, dict):
        raise TypeError("loss_terms: a {Tag: CriterionGroup} dict is expected")
    terms: dict = {}

    def walk(c, tag, prefix, outer):
        if isinstance(c, CriterionGroup):
            for x in c.criterions:
                walk(x, tag, prefix + c.name, (c.w,) + outer)
            return
        if not isinstance(c, Criterion):
            raise NotImplementedError(f"loss_terms: {type(c).__name__} is neither a Criterion nor a CriterionGroup")
        # (CriterionGroup.evaluate prepends its name to the names below it; the weights multiply from the criterion outwards)
        key = (prefix + c.name, id(c.f))
        term = terms.setdefault(key, LossTerm(key[0], c.f, {}))
        if tag in term.paths:
            raise NotImplementedError(f"loss term {key[0]!r} occurs twice in the criterion table of {tag}: one row cannot hold two values of a term")
        term.paths[tag] = (c.w,) + outer

    def leaves(c):
        return sum(leaves(x) for x in c.criterions) if isinstance(c, CriterionGroup) else 1

    for tag, c in sorted(criterions.items(), key=lambda kv: -leaves(kv[1])):  # (sorted() is stable)
        walk(c, tag, "", ())
    return list(terms.values())


class FlatLoss:
    """Device-side tables of the flat step for one criterion dict: the terms, their Tag sets and the [K, 32] table of weights per term
    and Tag code, which is the only thing that changes with the epoch (`set_epoch` rewrites it with a copy - outside a captured graph,
    like ClipAdam.sync_hyper_to_device)."""

    def __init__(self, criterions, device):
        self.terms = loss_terms(criterions)
        if not self.terms:
            raise ValueError("the criterion table has no terms")
        self.names = list(dict.fromkeys(t.name for t in self.terms))
        by_name = {n: [t for t in self.terms if t.name == n] for n in self.names}
        for n, ts in by_name.items():
            sets = [t.tag_set for t in ts]
            if sum(bin(m).count("1") for m in sets) != bin(functools.reduce(lambda a, b: a | b, sets)).count("1"):
                raise NotImplementedError(f"loss terms named {n!r} overlap in their Tags: one [B] vector cannot hold both")
        name_sets = [functools.reduce(lambda a, b: a | b, [t.tag_set for t in by_name[n]]) for n in self.names]
        # live[name][code]: whether a row of that Tag code carries the name's loss - one index_select with the row codes gives "mt_rows"
        self.live = torch.tensor([[bool((m >> c) & 1) for c in range(32)] for m in name_sets], dtype=torch.bool, device=device)
        self.wtable = torch.zeros((len(self.terms), 32), dtype=torch.float32, device=device)
        self._epoch_sig = None

    def table_at(self, epoch):
        rows = []
        for t in self.terms:
            row = [0.0] * 32
            for tag in t.paths:
                row[_tag_code(tag)] = float(t.weight(tag, epoch))
            rows.append(row)
        return rows

    def set_epoch(self, epoch, replaying=False) -> bool:
        """Write the epoch's weights into the device table if they changed.  `replaying`: earlier replays of a captured step may still
        read the old values - wait for them first (once per epoch at most)."""
        rows = self.table_at(epoch)
        sig = tuple(map(tuple, rows))
        if sig == self._epoch_sig:
            return False
        if replaying:
            torch.cuda.current_stream().synchronize()
        self.wtable.copy_(torch.tensor(rows, dtype=torch.float32))  # synchronous, pageable: rare
        self._epoch_sig = sig
        return True


class _MissingLabel(KeyError):
    pass


class _Labels:
    """The flat batch as the criterions see it: a field no sub-batch of the step carries raises _MissingLabel."""

    def __init__(self, batch: Batch):
        self._batch, self.meta = batch, batch.meta

    def __getitem__(self, k):
        try:
            return self._batch[k]
        except KeyError:
            raise _MissingLabel(k) from None

    def __contains__(self, k):
        return k in self._batch

    def __getattr__(self, name):
        return getattr(self._batch, name)


def flat_training_step(model: nn.Module, flat_batch: Batch, epoch: int, criterions, _tables: "FlatLoss | None" = None):
    """training_step over the B rows of `flatten_batches(...)`: the reference's sum (train.py:372-439) written as
    (1/B) sum_terms sum_{i<B} [Tag_i has the term] * w_term,Tag_i(epoch) * dataset_weight_i * val_term,i.  Every term's kernel visits all
    B rows and is told which are live (ttk_loss_batch_rows: membership of the row's Tag code in the term's Tag set, not the weight);
    the weights come from a device table indexed by the Tag code (ttk_row_weights).  No launch argument depends on the per-Tag split.
    Returns {"loss", "mt_losses": {name: [B] values, 0 in dead rows}, "mt_rows": {name: [B] bool, the live rows}}:
    mt_losses[name][mt_rows[name]] is what training_step's mt_losses[name] holds for the same sub-batches.
    A term whose label field is in none of the step's sub-batches (no field of that name in `flat_batch`) has no live row: its values
    are zeros and its kernel is not launched."""
    from .neuralnets import _hipops

    image = flat_batch["image"]
    if not image.is_cuda:
        raise RuntimeError("flat_training_step runs in HIP kernels on the MI355X: CUDA tensors required (no CPU fallback)")
    _hip.lib().clear_stale_error("the start of a training step")
    tables = _tables if _tables is not None else FlatLoss(criterions, image.device)
    if _tables is None:
        tables.set_epoch(epoch)
    tag_code = flat_batch["tag_code"]
    B = int(tag_code.shape[0])
    preds = model(image, flat_batch["coord_convention_id"])
    rw = _hipops.row_weights(tables.wtable, tag_code, flat_batch["dataset_weight"] if "dataset_weight" in flat_batch else None, len(tables.terms))
    vals = []
    labels = _Labels(flat_batch)
    with _hipops.loss_batch() as lb:
        lb.tag_code = tag_code
        for k, term in enumerate(tables.terms):
            lb.tag_set = term.tag_set
            seen = len(lb.records)
            try:
                v = term.f(preds, labels)
            except _MissingLabel:
                if len(lb.records) != seen:
                    raise NotImplementedError(f"criterion {term.name!r} cannot be flattened: it launched a loss kernel before reading a label "
                                              "that this step does not have") from None
                continue  # no row of this step can be live for it
            if not (len(lb.records) == seen + 1 and lb.records[-1][3] is v and tuple(v.shape) == (B,)):
                # the value is not the untouched output of ONE batched loss kernel (the criterion post-processes it, combines several, or
                # computes it elsewhere): default_compute_loss runs such terms unbatched, over their sub-batch's rows only - there is no
                # such thing here, and computing over dead rows would read labels that do not exist
                raise NotImplementedError(f"criterion {term.name!r} cannot be flattened: its value is not the direct per-sample output of one "
                                          "batched loss kernel (use the per-Tag layout)")
            vals.append(LossVal(v, SampleWeight(1.0, rw[k], v), term.name))
    loss_sum = _batched_loss_sum(lb, vals, 1.0 / B)
    if not vals:
        raise ValueError("flat_training_step: the batch carries the labels of none of the loss terms")
    by_name = defaultdict(list)
    for v in vals:
        by_name[v.name].append(v.val)
    mt_losses = {}
    for n in tables.names:
        vs = by_name.get(n)
        if not vs:
            mt_losses[n] = torch.zeros(B, dtype=torch.float32, device=tag_code.device)
        else:
            mt_losses[n] = vs[0] if len(vs) == 1 else functools.reduce(torch.add, vs)  # (disjoint Tag sets: dead rows are exactly 0)
    live = tables.live.index_select(1, tag_code)  # [names, B]; the codes are those of _tag_code, 0..31
    return {"loss": loss_sum, "mt_losses": mt_losses, "mt_rows": dict(zip(tables.names, live.unbind(0)))}


def _criterion_weights(c, step):
    """Flat tuple of every weight in a criterion tree at `step` (they are constants inside a captured graph)."""
    if isinstance(c, dict):
        return tuple((str(k), _criterion_weights(v, step)) for k, v in c.items())
    if isinstance(c, CriterionGroup):
        return (_weight_at(c.w, step),) + tuple(_criterion_weights(x, step) for x in c.criterions)
    return (_weight_at(c.w, step),)


class GraphedTrainStep:
    """zero_grad + training_step + backward + ClipAdam.step captured ONCE as a hipGraph and replayed every step.

    A pose-estimator step is ~200 kernel launches, half of them small head / loss / bookkeeping kernels; enqueueing
    them from Python costs ~4.7 ms of host time per step next to ~8.8 ms of GPU work (B = 512) - on a slower host, or
    at smaller batches, that host time is the bound and a captured graph, which enqueues the same work with one call,
    removes it.  (The reference has no counterpart: Lightning drives eager PyTorch; `train_poseestimator.py:442-454`.)

    The graph stays valid while the sub-batch layout (tags, sizes, fields), the epoch-dependent loss weights and the
    learning-rate-independent launch arguments stay the same: `run()` compares a signature and re-captures when it
    changes (e.g. during the NLL ramp epochs).  Learning rates, weight decays and Adam's step count live in device
    memory (ClipAdam.sync_hyper_to_device), so scheduler steps need no re-capture.  New batches are copied into the
    graph's static input tensors.  Single-GPU: the data-parallel all-reduce is issued eagerly (train.fit).

    layout="flat": the captured step is `flat_training_step` over static [B, ...] buffers, whose launch arguments depend neither on
    the per-Tag split nor on the criterion weights - per step the sub-batches' fields and one Tag code per row are copied in (one
    ttk_multi_copy launch, no host synchronisation), on an epoch change the [terms, 32] weight table.  The signature is (B, the label
    fields seen so far, model.training): ONE capture serves a run whose first step shows every field, a loader that mixes Tags and
    draws their sizes anew every step included; otherwise a Tag that brings a new field re-captures once.  `run()` then also returns
    "mt_rows" (flat_training_step)."""

    def __init__(self, model: nn.Module, criterions, optimizer: "ClipAdam", layout: str = "per_tag"):
        if not isinstance(optimizer, ClipAdam):
            raise TypeError("GraphedTrainStep needs the fused ClipAdam optimiser (its step is capturable)")
        if layout not in ("per_tag", "flat"):
            raise ValueError(f"GraphedTrainStep: layout {layout!r} (per_tag | flat)")
        self.layout = layout
        self.model, self.criterions, self.optimizer = model, criterions, optimizer
        self.graph = None
        self._sig = None
        self._static: list[Batch] = []  # the graph's static inputs: per-Tag one Batch per sub-batch, flat ONE Batch of [B, ...] buffers
        self._out = None
        self.captures = 0
        self._miss_streak = 0      # consecutive steps whose signature differed from the captured one
        self.eager_only = False    # set once re-capturing is seen to happen step after step
        # flat layout only; none of it refers to a static input
        self._tables = None        # FlatLoss
        self._fields: dict = {}    # field -> (trailing shape, dtype), every field seen so far
        self._fill: dict = {}      # [B] sources of what no sub-batch carries: Tag code -> int32 vector filled with it, "ones" -> float32 ones

    # ---- what the two layouts differ in: signature, step function, static inputs, which source goes to which of them -----------------------
    def _signature(self, batches, epoch):
        if self.layout == "per_tag":
            layout = tuple((str(b.meta.tag), b.meta.batchsize, tuple((k, tuple(v.shape), str(v.dtype)) for k, v in b.items()))
                           for b in batches)
            return layout, _criterion_weights(self.criterions, epoch), self.model.training
        # flat: (B, the fields seen so far, model.training) - a Tag that brings a field no earlier step had re-captures
        B = sum(int(b.meta.prefixshape[0]) for b in batches)
        if self._tables is None:
            self._tables = FlatLoss(self.criterions, batches[0]["image"].device)
        for b in batches:
            for k, v in b.items():
                if torch.is_tensor(v) and k != "tag_code":
                    cur = (tuple(v.shape[1:]), v.dtype)
                    if self._fields.setdefault(k, cur) != cur:
                        raise ValueError(f"GraphedTrainStep(flat): field {k!r} is {cur[0]} {cur[1]} in {b}, {self._fields[k][0]} {self._fields[k][1]} before")
        return B, tuple(self._fields), self.model.training

    def _make_static(self, batches):
        if self.layout == "per_tag":
            # the fields every sub-batch has (image, coord_convention_id, ...) are views of ONE tensor per field, in sub-batch
            # order, so that training_step's concatenation over the sub-batches is a view (_concat_rows) instead of a copy per step
            shared = set.intersection(*[set(k for k, v in b.items() if torch.is_tensor(v)) for b in batches]) if len(batches) > 1 else set()
            joined = {k: torch.concat([b[k] for b in batches], dim=0).split([int(b[k].shape[0]) for b in batches], dim=0) for k in shared
                      if all(b[k].dim() >= 1 and b[k].shape[1:] == batches[0][k].shape[1:] and b[k].dtype == batches[0][k].dtype for b in batches)}
            self._static = [Batch(b.meta, ((k, joined[k][i] if k in joined else v.clone()) for k, v in b.items())) for i, b in enumerate(batches)]
            return
        # flat: buffers for every field seen so far, filled with this step's batches
        B = sum(int(b.meta.prefixshape[0]) for b in batches)
        dev = batches[0]["image"].device
        flat = {k: torch.zeros((B,) + trail, dtype=dtype, device=dev) for k, (trail, dtype) in self._fields.items() if k != "dataset_weight"}
        flat["tag_code"] = torch.zeros(B, dtype=torch.int32, device=dev)
        flat["dataset_weight"] = torch.ones(B, dtype=torch.float32, device=dev)
        self._fill = {"ones": torch.ones(B, dtype=torch.float32, device=dev)}
        self._static = [Batch(Metadata(batches[0].meta._imagesize, batchsize=B, tag=None), flat)]
        self._copy_in(batches)

    def _pairs(self, batches):
        """(static tensor, source) for every tensor of `batches`; flat: the sub-batches' rows of the buffers, with one Tag code per row and
        the dataset weights as float32 (1 where a sub-batch has none)."""
        if self.layout == "per_tag":
            yield from ((dst[k], v) for dst, src in zip(self._static, batches) for k, v in src.items())
            return
        flat, off = self._static[0], 0
        for b in batches:
            n = int(b.meta.prefixshape[0])
            code = _tag_code(b.meta.tag)
            if code not in self._fill:  # (first sight of a Tag: one allocation and fill, outside any capture)
                self._fill[code] = torch.full(flat["tag_code"].shape, code, dtype=torch.int32, device=flat["tag_code"].device)
            items = [("tag_code", self._fill[code][:n])] + [(k, v) for k, v in b.items() if torch.is_tensor(v) and k != "tag_code"]
            if "dataset_weight" not in b:
                items.append(("dataset_weight", self._fill["ones"][:n]))
            for k, v in items:
                d = flat[k][off:off + n]
                yield d, (v.to(d.dtype) if k == "dataset_weight" else v)
            off += n

    def _step(self, inputs, epoch):
        """Forward, losses, backward and optimiser step over `inputs`: launched, or recorded while a capture is open."""
        if self.layout == "per_tag":
            out = training_step(self.model, inputs, epoch, self.criterions)
        else:
            out = flat_training_step(self.model, inputs[0], epoch, self.criterions, self._tables)
        out["loss"].backward()
        self.optimizer.step()
        return out

    # ---- the protocol, once for both ------------------------------------------------------------------------------------------------
    def _eager(self, batches, epoch):
        self.optimizer.zero_grad(set_to_none=True)
        if self.layout == "flat":
            self._tables.set_epoch(epoch, replaying=self.graph is not None)
            batches = [flatten_batches(batches)]
        return self._step(batches, epoch)

    def _capture(self, epoch):
        self.optimizer.sync_hyper_to_device()
        self.graph = torch.cuda.CUDAGraph()
        self.optimizer.zero_grad(set_to_none=True)  # gradients are allocated from the graph's pool at fixed addresses
        with _hip.CAPTURE_LOCK:  # (a loader's prefetch thread must not allocate or copy while the capture is open: _hip.CAPTURE_LOCK)
            with torch.cuda.graph(self.graph):
                out = self._step(self._static, epoch)
        self._out = out
        self.captures += 1

    def _copy_in(self, batches):
        """New batches -> the static inputs.  Whatever can travel as 32-bit words does, whatever its dtype (int64 ids, float32 labels),
        all in ONE ttk_multi_copy launch, which reads pointers and element counts only; the rest falls back to copy_.  A source that
        already is its static tensor (the loader wrote into it) and empty tensors need nothing."""
        words = lambda t: t if t.dtype == torch.float32 else t.view(torch.float32)
        fsrc, fdst = [], []
        for d, v in self._pairs(batches):
            if v is d or (v.numel() == d.numel() and (v.numel() == 0 or v.data_ptr() == d.data_ptr())):
                continue
            if (v.is_cuda and v.dtype == d.dtype and v.element_size() % 4 == 0 and v.is_contiguous() and d.is_contiguous()
                    and v.numel() == d.numel() and v.dim() >= 1 and v.data_ptr() % 4 == 0):
                fsrc.append(words(v))
                fdst.append(words(d))
            else:
                d.copy_(v.reshape(d.shape), non_blocking=True)
        if fdst:
            _hip.lib().multi_copy(fsrc, fdst)

    def run(self, batches: List[Batch], epoch: int):
        """One training step.  Returns {"loss", "mt_losses"} (flat: and "mt_rows"); when replayed these are the graph's static output
        tensors (overwritten by the next call)."""
        if self.eager_only:
            return self._eager(batches, epoch)
        sig = self._signature(batches, epoch)
        if sig != self._sig:
            # Per-Tag: a loader that mixes datasets of several Tags draws the per-Tag sub-batch sizes anew every step (ResidentLoader): the
            # signature then changes almost every step and each step would run eagerly AND re-capture (synchronise, capture, a new private
            # pool) - far slower than eager.  Three misses in a row: stay eager for the rest of the run (round-3 advisor finding).
            self._miss_streak += 1
            if self.layout == "per_tag" and self._miss_streak >= 3 and self.captures >= 2:
                import warnings
                warnings.warn("GraphedTrainStep: the sub-batch layout changed on three consecutive steps (per-Tag batch sizes vary from step to "
                              "step?) - a captured graph would be re-captured every step; running eagerly from here on", RuntimeWarning, stacklevel=2)
                self.eager_only, self.graph, self._static, self._out = True, None, [], None
                return self._eager(batches, epoch)
            # first step with this signature: run it eagerly (lazy initialisation, table building, stream creation happen
            # here and the step counts), then capture for the following steps
            out = self._eager(batches, epoch)
            # hand back detached copies and drop the eager autograd graph BEFORE capturing: with it still alive,
            # hipStreamEndCapture / graph instantiation was seen to segfault on ROCm 7.2 (tools/debug/graph_capture4.py)
            fresh = lambda t: t.detach().clone()
            out = {k: fresh(v) if torch.is_tensor(v) else {n: fresh(x) for n, x in v.items()} for k, v in out.items()}
            torch.cuda.synchronize()
            self._make_static(batches)
            self._capture(epoch)
            self._sig = sig
            return out
        self._copy_in(batches)
        self._miss_streak = 0
        if self.layout == "flat":
            self._tables.set_epoch(epoch, replaying=True)  # (the weight table is device memory the graph reads, like the learning rates)
        self.optimizer.before_graph_replay()
        self.graph.replay()
        self.optimizer.after_graph_replay()
        return self._out


@torch.no_grad()
def validate(model: nn.Module, val_loader, val_criterions) -> float:
    """One validation epoch with LitModel.validation_step's arithmetic (scripts/train_poseestimator.py:332-338) and Lightning's
    epoch reduction of `self.log("val_loss", ..., on_epoch=True, batch_size=n)`: per batch the SUM over samples and terms of
    value * weight (not a mean), per epoch the batch-size-weighted mean of those sums.  The model runs in eval mode without
    coord_convention_id; the criterions receive the BATCH INDEX as their step (the reference's quirk: weights that ramp with the
    epoch ramp with the batch index here)."""
    was_training = model.training
    model.eval()
    _hip.lib().clear_stale_error("validate")  # (once per validation epoch: a pending error of an unrelated earlier call must not be blamed on these launches)
    total, count = None, 0
    try:
        for batch_idx, batch in enumerate(val_loader):
            if isinstance(batch, (list, tuple)):
                raise TypeError("validate: the validation loader yields ONE Batch per iteration (reference pipelines.py:543-552), got a list - "
                                "train loaders yield lists")
            pred = model(batch["image"])
            crit = val_criterions[batch.meta.tag] if isinstance(val_criterions, dict) else val_criterions
            values = crit.evaluate(pred, batch, batch_idx)
            val_loss = torch.cat([(lv.val * lv.weight).reshape(-1) for lv in values]).sum()
            n = int(batch.meta.batchsize)
            total = val_loss * n if total is None else total + val_loss * n
            count += n
    finally:
        model.train(was_training)
    if count == 0:
        raise ValueError("empty validation loader")
    return float(total.item()) / count


class CheckpointCallback:
    """ModelCheckpoint(save_top_k=1, save_last=True, monitor="val_loss", filename="best") of the reference's training script
    (:423-431) followed by its final re-save in the plain format (:460-465): after every validation epoch `last.ckpt` is written,
    and `best.ckpt` whenever the monitored value reaches a new minimum - both with `save_model` (state dict + constructor
    arguments, loadable by `models.load_model`)."""

    def __init__(self, dirpath: str):
        self.dirpath = dirpath
        self.best_value = math.inf
        self.best_epoch = -1
        self.history: list[float] = []

    @property
    def best_model_path(self):
        return os.path.join(self.dirpath, "best.ckpt")

    @property
    def last_model_path(self):
        return os.path.join(self.dirpath, "last.ckpt")

    def _save(self, model, path):
        import copy

        os.makedirs(self.dirpath, exist_ok=True)
        save_model(copy.deepcopy(model).to("cpu"), path)

    def state_dict(self) -> dict:
        return {"best_value": float(self.best_value), "best_epoch": int(self.best_epoch), "history": [float(v) for v in self.history]}

    def load_state_dict(self, state: dict):
        self.best_value, self.best_epoch, self.history = float(state["best_value"]), int(state["best_epoch"]), [float(v) for v in state["history"]]

    def on_validation_end(self, epoch: int, model: nn.Module, val_loss: float):
        self.history.append(val_loss)
        self._save(model, self.last_model_path)
        if val_loss < self.best_value:
            self.best_value, self.best_epoch = val_loss, epoch
            self._save(model, self.best_model_path)


class NonFiniteGradientError(RuntimeError):
    """`fit()`: a `skip_nonfinite` optimiser has skipped `max_consecutive_skips` steps in a row."""


# ---------------------------------------------------------------------------------------------
# run state: everything a run stopped after an epoch needs to go on as if it had not been stopped
# ---------------------------------------------------------------------------------------------
RUN_STATE_VERSION = 1


class RunState:
    """What `fit(run_state=...)` saves and resumes from.

    `path`: the file (one `torch.save`; data-parallel replicas add `<path>.rank<r>`, below).  `every`: save after every that many
    epochs (0: only when `stop_after_epoch` is reached).  `stop_after_epoch=N`: leave the loop once N epochs are complete, after saving.
    `resume`: what `load_run_state(path)` returned, or None for a fresh start.  `meta`: plain data stored beside the state (the training
    script records its arguments there).  `objects`: {name: object with state_dict() / load_state_dict()} captured on top of what fit()
    captures itself - model, optimiser (+ health counters), scheduler, every callback and loader that has state_dict(), torch's global CPU
    generator and the device's default CUDA generator.
    `rank` / `world`: BatchNorm running statistics and the data streams are per replica.  Rank 0 writes `path` (weights, optimiser,
    scheduler, callbacks); every rank, rank 0 included, writes `<path>.rank<r>` with its loaders, generators and module buffers.  A state
    written by another `world` is refused."""

    def __init__(self, path: str, every: int = 1, stop_after_epoch: int | None = None, resume: dict | None = None, meta: dict | None = None,
                 objects: dict | None = None, rank: int = 0, world: int = 1):
        self.path, self.every, self.stop_after_epoch, self.resume = str(path), int(every), stop_after_epoch, resume
        self.meta, self.objects, self.rank, self.world = dict(meta or {}), dict(objects or {}), int(rank), int(world)

    def rank_path(self, rank: int | None = None) -> str:
        return f"{self.path}.rank{self.rank if rank is None else rank}"

    def due(self, next_epoch: int) -> bool:
        return (self.every > 0 and next_epoch % self.every == 0) or self.stops(next_epoch)

    def stops(self, next_epoch: int) -> bool:
        return self.stop_after_epoch is not None and next_epoch >= int(self.stop_after_epoch)


def _atomic_torch_save(obj, path: str):
    """torch.save to a temporary name in the same directory, then os.replace: a write that fails leaves the previous file intact."""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    tmp = os.path.join(d, f".{os.path.basename(path)}.tmp{os.getpid()}")
    try:
        with open(tmp, "wb") as f:
            torch.save(obj, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def _cpu(obj):
    if torch.is_tensor(obj):
        return obj.detach().to("cpu").clone()
    if isinstance(obj, dict):
        return {k: _cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_cpu(v) for v in obj)
    return obj


def _stateful(objs: dict) -> dict:
    return {k: o for k, o in objs.items() if o is not None and hasattr(o, "state_dict") and hasattr(o, "load_state_dict")}


def _rng_state(device) -> dict:
    out = {"cpu": torch.get_rng_state()}
    if device is not None and device.type == "cuda":
        out["cuda"] = torch.cuda.get_rng_state(device)
    return out


def _set_rng_state(state: dict, device):
    torch.set_rng_state(state["cpu"])
    if "cuda" in state:
        if device is None or device.type != "cuda":
            raise ValueError("the run state holds a CUDA generator state, the model is not on a GPU")
        torch.cuda.set_rng_state(state["cuda"], device)


def _model_device(model):
    p = next(iter(model.parameters()), None)
    return None if p is None else p.device


def save_run_state(path, model, optimizer=None, scheduler=None, next_epoch=0, callbacks=(), train_loader=None, val_loader=None, objects=None,
                   meta=None, rank=0, world=1):
    """Write the run state at an epoch boundary (RunState; `fit(run_state=...)` calls this).  One `torch.save` file per call, written
    under a temporary name and moved into place.  Tensors are stored on the CPU.  With `world > 1` rank 0 writes `path` and every rank
    writes `<path>.rank<r>`."""
    device = _model_device(model)
    per_rank = {"version": RUN_STATE_VERSION, "next_epoch": int(next_epoch), "world": int(world), "rank": int(rank), "rng": _rng_state(device),
                "loaders": {k: _cpu(o.state_dict()) for k, o in _stateful({"train": train_loader, "val": val_loader}).items()},
                "objects": {k: _cpu(o.state_dict()) for k, o in _stateful(dict(objects or {})).items()}}
    shared = None
    if rank == 0:
        shared = {"version": RUN_STATE_VERSION, "next_epoch": int(next_epoch), "world": int(world), "meta": dict(meta or {}),
                  "model": _cpu(model.state_dict()),
                  "optimizer": None if optimizer is None else _cpu(optimizer.state_dict()),
                  "optimizer_health": optimizer.health() if getattr(optimizer, "skip_nonfinite", False) else None,
                  "scheduler": None if scheduler is None else _cpu(scheduler.state_dict()),
                  "callbacks": [(type(cb).__name__, _cpu(cb.state_dict())) for cb in callbacks if hasattr(cb, "state_dict")]}
    if world == 1:
        _atomic_torch_save(dict(shared, **{k: per_rank[k] for k in ("rng", "loaders", "objects")}), path)
        return
    per_rank["buffers"] = _cpu(dict(model.named_buffers()))
    _atomic_torch_save(per_rank, f"{path}.rank{rank}")  # the replica's part first: a shared part never points at a replica part that is older
    if shared is not None:
        _atomic_torch_save(shared, path)


def load_run_state(path, rank=0, world=1) -> dict:
    """The state `save_run_state` wrote, for `RunState(resume=...)`.  With `world > 1`: the shared part, then this rank's own file."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    if state.get("version") != RUN_STATE_VERSION:
        raise ValueError(f"{path}: run state version {state.get('version')}, this package reads {RUN_STATE_VERSION}")
    if int(state["world"]) != int(world):
        raise ValueError(f"{path} was written by a run of {state['world']} replica(s), this run has {world}: resuming with a different "
                         "WORLD_SIZE is refused (the data streams and BatchNorm statistics are per replica)")
    if world > 1:
        own = torch.load(f"{path}.rank{rank}", map_location="cpu", weights_only=True)
        if int(own["world"]) != int(world) or int(own["rank"]) != int(rank) or int(own["next_epoch"]) != int(state["next_epoch"]):
            raise ValueError(f"{path}.rank{rank} (epoch {own['next_epoch']}, rank {own['rank']} of {own['world']}) does not belong to {path} "
                             f"(epoch {state['next_epoch']}, {world} replicas)")
        state.update({k: own[k] for k in ("rng", "loaders", "objects", "buffers")})
    return state


def _restore_run_state(state, model, optimizer, scheduler, callbacks, train_loader, val_loader, objects, rank=0):
    """Put `state` into the live objects.  Called by fit() after the callbacks' on_train_start and before the first step (so before any
    graph capture: the optimiser's load drops every cached device address)."""
    model.load_state_dict(state["model"])
    if "buffers" in state:  # this replica's own BatchNorm statistics over rank 0's
        live = dict(model.named_buffers())
        if set(live) != set(state["buffers"]):
            raise ValueError("the run state's module buffers are not this model's")
        with torch.no_grad():
            for k, v in state["buffers"].items():
                live[k].copy_(v)
    if state["optimizer"] is not None:
        if optimizer is None:
            raise ValueError("the run state holds an optimiser state, fit() was given none")
        optimizer.load_state_dict(state["optimizer"])
    if state.get("optimizer_health") is not None:
        if not getattr(optimizer, "skip_nonfinite", False):
            raise ValueError("the run state was written with skip_nonfinite, this optimiser was built without")
        optimizer.load_health(state["optimizer_health"])
    if state["scheduler"] is not None:
        if scheduler is None:
            raise ValueError("the run state holds a scheduler state, fit() was given none")
        scheduler.load_state_dict(state["scheduler"])
    live_cbs = [cb for cb in callbacks if hasattr(cb, "state_dict")]
    if rank != 0 and not live_cbs:
        pass  # (the callbacks in the shared part are rank 0's: checkpoints and the SWA average are written there only)
    elif [type(cb).__name__ for cb in live_cbs] != [n for n, _ in state["callbacks"]]:
        raise ValueError(f"the run state holds callbacks {[n for n, _ in state['callbacks']]}, fit() was given {[type(cb).__name__ for cb in live_cbs]}")
    for cb, (_, sd) in zip(live_cbs, state["callbacks"]):  # (zip: nothing to do on a rank without callbacks)
        cb.load_state_dict(sd)
    for what, live in (("loaders", _stateful({"train": train_loader, "val": val_loader})), ("objects", _stateful(dict(objects or {})))):
        if set(live) != set(state[what]):
            raise ValueError(f"the run state holds {what} {sorted(state[what])}, fit() was given {sorted(live)}")
        for k, o in live.items():
            o.load_state_dict(state[what][k])
    _set_rng_state(state["rng"], _model_device(model))


def fit(model: nn.Module, train_loader, criterions, optimizer, scheduler=None, epochs=1, callbacks=(), on_step=None,
        grad_sync=None, val_loader=None, val_criterions=None, reducer=None, graphed=False, start_epoch=0, run_state: "RunState | None" = None,
        max_consecutive_skips=10):
    """Epoch loop with Lightning's ordering: per step zero_grad -> forward -> loss -> backward -> (gradient exchange) -> clip + Adam;
    per epoch the scheduler step, then - when `val_loader` is given - a validation epoch (`validate`) whose value goes to the
    callbacks' `on_validation_end(epoch, model, val_loss)` (CheckpointCallback: best.ckpt / last.ckpt), then `on_train_epoch_end`.
    Data-parallel replicas pass their `parallel.GradAllReduce` as `reducer`: `begin_step()` before the step, `finish()` between
    backward and the optimiser (it waits for the in-place all-reduces that ran during backward), and - should backward raise -
    `abort()` so that no collective is left in flight on gradient memory that is about to be freed.  `grad_sync(model)` is the
    older hook form of the same (runs between backward and the optimiser step).
    Gradients are dropped (set_to_none) before every step: the arena views autograd installs are the exchange buffers.
    `graphed=True` (single replica, ClipAdam): every step is a replay of ONE captured hipGraph (`GraphedTrainStep`; re-captured when the
    sub-batch layout or the epoch's loss weights change); `on_step` then receives the graph's static output tensors.
    `graphed="flat"`: the same with GraphedTrainStep's flat layout - one graph also when the per-Tag sizes change from step to step and
    through the epochs of a weight ramp; `on_step` receives [B] loss vectors and their live-row masks ("mt_rows").
    `start_epoch`: the loop runs `range(start_epoch, epochs)`.  `run_state` (RunState): after an epoch's callbacks (`on_train_epoch_end`
    included) the run state is saved when due; with `run_state.resume` the saved state is restored after the callbacks' `on_train_start`
    and before the first step, and the loop starts at the saved epoch.  Under TTK_DETERMINISTIC=1 the resumed run is bitwise the
    uninterrupted one.  Epoch boundaries only: no signal handling, no mid-epoch resume.
    `max_consecutive_skips` (ClipAdam(skip_nonfinite=True) only): once per epoch, after its last step, the optimiser's health counters are
    read; new skips are reported with a RuntimeWarning, and NonFiniteGradientError names the culprit parameter once that many steps in a
    row were skipped.  (10 is a policy, not a measurement.)"""
    stepper = None
    if graphed:
        if isinstance(graphed, str) and graphed != "flat":
            raise ValueError(f"fit: graphed={graphed!r} (False | True | 'flat')")
        if reducer is not None or grad_sync is not None:
            raise ValueError("graphed steps are single-replica (collectives inside a captured graph are untested on this stack)")
        stepper = GraphedTrainStep(model, criterions, optimizer, layout="flat" if graphed == "flat" else "per_tag")
    for cb in callbacks:
        if hasattr(cb, "on_train_start"):
            cb.on_train_start(model)
    if run_state is not None and run_state.resume is not None:
        _restore_run_state(run_state.resume, model, optimizer, scheduler, callbacks, train_loader, val_loader, run_state.objects, run_state.rank)
        saved_epoch = int(run_state.resume["next_epoch"])
        if start_epoch not in (0, saved_epoch):
            raise ValueError(f"fit: start_epoch={start_epoch}, the run state continues at epoch {saved_epoch}")
        start_epoch = saved_epoch
    model.train()
    params = list(model.parameters()) if reducer is not None else None
    guarded = bool(getattr(optimizer, "skip_nonfinite", False))
    skipped_before = optimizer.health()["skipped"] if guarded else 0
    for epoch in range(start_epoch, epochs):
        for batches in train_loader:
            if stepper is not None:
                out = stepper.run(batches, epoch)
                if on_step is not None:
                    on_step(epoch, out)
                continue
            optimizer.zero_grad(set_to_none=True)
            if reducer is not None:
                reducer.begin_step()
            out = training_step(model, batches, epoch, criterions)
            try:
                out["loss"].backward()
            except BaseException:
                if reducer is not None:
                    reducer.abort()
                raise
            if reducer is not None:
                reducer.finish(params)
            if grad_sync is not None:
                grad_sync(model)
            optimizer.step()
            if on_step is not None:
                on_step(epoch, out)
        if guarded:
            skipped_before = _check_health(model, optimizer, epoch, skipped_before, max_consecutive_skips)
        if scheduler is not None:
            scheduler.step()
        if val_loader is not None:
            val_loss = validate(model, val_loader, val_criterions if val_criterions is not None else criterions)
            for cb in callbacks:
                if hasattr(cb, "on_validation_end"):
                    cb.on_validation_end(epoch, model, val_loss)
        for cb in callbacks:
            if hasattr(cb, "on_train_epoch_end"):
                cb.on_train_epoch_end(epoch, model)
        if run_state is not None and run_state.due(epoch + 1):
            save_run_state(run_state.path, model, optimizer, scheduler, epoch + 1, callbacks, train_loader, val_loader, run_state.objects,
                           run_state.meta, run_state.rank, run_state.world)
            if run_state.stops(epoch + 1):
                break
    return model


def _check_health(model, optimizer, epoch, skipped_before, max_consecutive_skips):
    """The once-per-epoch read of a guarded optimiser's device counters (fit)."""
    h = optimizer.health()
    if h["skipped"] == skipped_before:
        return skipped_before
    culprit = "?"
    if h["culprit_index"] >= 0:
        p = optimizer.parameter_at(h["culprit_index"])
        culprit = next((n for n, q in model.named_parameters() if q is p), f"parameter {h['culprit_index']} of the optimiser")
    if max_consecutive_skips is not None and h["consecutive"] >= max_consecutive_skips:
        raise NonFiniteGradientError(f"epoch {epoch}: the last {h['consecutive']} optimiser steps had a non-finite gradient norm and were skipped "
                                     f"({h['skipped']} in the run); first non-finite gradient of the most recent one: {culprit}")
    import warnings
    warnings.warn(f"epoch {epoch}: {h['skipped'] - skipped_before} optimiser step(s) skipped for a non-finite gradient norm ({h['skipped']} in the "
                  f"run); first non-finite gradient of the most recent one: {culprit}", RuntimeWarning, stacklevel=3)
    return h["skipped"]
