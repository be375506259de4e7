"""MobileNetV1-style backbone of the pose estimator on MI355X.

Drop-in for the reference's `trackertraincode/backbones/mobilenet_v1.py` (`MobileNet` :95-189,
`DepthWiseBlock` :36-92): same constructor signature, attribute / state-dict names and return
convention `(features[B,F], [z65, z33, z17, z9, z5])`, but the arithmetic is one autograd node whose
forward and backward launch the HIP kernels of ../../csrc through the C-ABI (include/ttk.h):

    stem 5x5 s2 -> 13 x (depthwise 3x3 -> pointwise 1x1 on fp32 MFMA) -> global average pool

Data layout in HBM: activations are fp32 in channel blocks of 32, `[C/32][B*H*W][32]` (include/ttk.h, "Activation layout"): the
tensors below are allocated with the nominal shape `[B, H, W, C]` but only ever travel from kernel to kernel; what PyTorch sees
(the pooled features, the intermediate maps through ttk_bn_act) is plain.  Every conv writes its RAW output once, BatchNorm statistics
come out of the conv's epilogue, and BN + ReLU (+ residual) are applied by the consumer while
loading (forward) - backward mirrors this with three per-channel coefficients (see include/ttk.h).

There is no PyTorch fallback for training: on CUDA tensors the HIP path runs or raises.
CPU tensors are accepted in eval mode only (the ONNX-export / checkpoint-inspection surface of
scripts/export_model.py), through plain torch ops.
"""
from __future__ import annotations

import math
import os
from typing import NamedTuple

import torch
import torch.nn as nn
import torch.nn.functional as F

import sys

from .. import _hip
from ..neuralnets.modelcomponents import BlurPool2D
from . import _mobilenet_bc

_THIS = sys.modules[__name__]

__all__ = ["MobileNet", "DepthWiseBlock"]

NormalizationLayer = nn.BatchNorm2d
ActivationFunc = nn.ReLU

# (name, in, out, stride) of the 13 depthwise-separable blocks - reference mobilenet_v1.py:128-140
_BLOCKS = (
    ("dw2_1", 32, 64, 1), ("dw2_2", 64, 128, 2), ("dw3_1", 128, 128, 1), ("dw3_2", 128, 256, 2),
    ("dw4_1", 256, 256, 1), ("dw4_2", 256, 512, 2), ("dw5_1", 512, 512, 1), ("dw5_2", 512, 512, 1),
    ("dw5_3", 512, 512, 1), ("dw5_4", 512, 512, 1), ("dw5_5", 512, 512, 1), ("dw5_6", 512, 1024, 2),
    ("dw6", 1024, 1024, 1),
)
_INTERMEDIATES = ("dw2_1", "dw3_1", "dw4_1", "dw5_5", "dw6")
_STEM_CHANNELS = 32


def _scaled_blocks(widen_factor):
    """(stem channels, block table) of MobileNet(widen_factor): every channel count truncated as the reference does, int(c * widen_factor)
    (reference mobilenet_v1.py:113-146).  The HIP kernels take multiples of 8 in 8..2048; anything else raises ValueError."""
    def ch(c):
        v = int(c * widen_factor)
        if v < 8 or v > 2048 or v % 8:
            raise ValueError(f"widen_factor={widen_factor} gives a channel count int({c} * {widen_factor}) = {v}; the HIP backbone takes "
                             "multiples of 8 in 8..2048 (e.g. widen_factor 0.25, 0.5, 0.75, 1.0, 1.5, 2.0)")
        return v
    return ch(_STEM_CHANNELS), tuple((name, ch(cin), ch(cout), stride) for name, cin, cout, stride in _BLOCKS)


def _tuned_c(c) -> bool:
    """Channel counts of the tuned kernels (ttk_dwconv3x3_*, ttk_pwconv1x1_*, ttk_avgpool_*, ttk_bn_act): powers of two in 32..1024.
    Every other count runs on the any-channel-count family (ttk_anyc_*, include/ttk.h)."""
    return 32 <= c <= 1024 and (c & (c - 1)) == 0


class DepthWiseBlock(nn.Module):
    """Parameter container with the reference's names (conv_dw, bn_dw, conv_sep, bn_sep); the
    arithmetic of `forward` lives in the fused backbone function below.  Reference :36-92."""

    def __init__(self, inplanes, planes, stride=1, momentum=0.1, stochastic_depth=None, use_blurpool=True):
        super().__init__()
        assert stride in (1, 2)
        self.inplanes, self.planes = inplanes, planes = int(inplanes), int(planes)
        self.stride = stride
        if stochastic_depth:
            raise NotImplementedError("stochastic_depth is never enabled by the reference's pose estimator")
        self.blurpool = stride == 2 and bool(use_blurpool)
        if self.blurpool:  # reference :43-55: blur + downsample, then the depthwise conv at stride 1 (state-dict names conv_dw.0.kernel, conv_dw.1.weight)
            self.conv_dw = nn.Sequential(
                BlurPool2D(kernel_size=3, stride=2, channels=inplanes),
                nn.Conv2d(inplanes, inplanes, kernel_size=3, padding=1, stride=1, groups=inplanes, bias=False),
            )
        else:
            self.conv_dw = nn.Conv2d(inplanes, inplanes, kernel_size=3, padding=1, stride=stride, groups=inplanes, bias=False)
        self.bn_dw = NormalizationLayer(inplanes, momentum=momentum)
        self.conv_sep = nn.Conv2d(inplanes, planes, kernel_size=1, stride=1, padding=0, bias=False)
        self.bn_sep = NormalizationLayer(planes, momentum=momentum)
        self.relu = nn.ReLU(inplace=True)
        self.skip_connection = not (stride != 1 or inplanes != planes)
        self.stochastic_depth = None

    @property
    def dw_weight(self):
        """The trainable depthwise weight [C,1,3,3] (conv_dw.weight, or conv_dw.1.weight behind a BlurPool2D)."""
        return self.conv_dw[1].weight if self.blurpool else self.conv_dw.weight

    def forward(self, x):  # eval/export path in plain torch ops (CPU); training goes through MobileNet
        out = self.relu(self.bn_dw(self.conv_dw(x)))
        out = self.bn_sep(self.conv_sep(out))
        if self.skip_connection:
            out = out + x
        return self.relu(out)


# Precision of the TRAINING kernels, an attribute of every MobileNet INSTANCE (`MobileNet.precision`, `MobileNet.set_precision`; not part of
# `get_config()` / the state dict, so checkpoints load in the reference unchanged):
#   "fp32"          the reference's precision - activations, gradients and arithmetic fp32 (the default, `bench.py`'s headline);
#   "bf16-compute"  BASELINE config 5's bf16 leg: activation-sized tensors and their gradients bf16 in 64-channel blocks AND bf16 operands of
#                   the pointwise products (one MFMA product, fp32 accumulation); launch sequences in _mobilenet_bc.py, kernels csrc/bc_*.hip.
# The storage-only variants of rounds 2-4 ("bf16" / "bf16-all": bf16 tensors under the fp32 kernels, slower than fp32) are retired.
_PRECISIONS = ("fp32", "bf16-compute")
_RETIRED = ("bf16", "bf16-all")
_DEFAULT_PRECISION = "fp32"


def _check_precision(mode):
    mode = {torch.float32: "fp32", "f32": "fp32"}.get(mode, mode)
    if mode in _RETIRED or mode is torch.bfloat16:
        raise ValueError(f'precision "{mode}" (bf16 storage under the fp32 kernels) was retired: it ran slower than fp32; use "bf16-compute"')
    if mode not in _PRECISIONS:
        raise ValueError(f'precision must be "fp32" or "bf16-compute", got {mode}')
    return mode


def set_activation_dtype(mode):
    """Default precision of MobileNet instances that have not been given one of their own (`MobileNet.set_precision`): "fp32" or
    "bf16-compute".  Kept for the scripts' `--precision` flag; two networks of different precision in one process use `set_precision`."""
    global _DEFAULT_PRECISION
    _DEFAULT_PRECISION = _check_precision(mode)


def bf16_compute() -> bool:
    """Is the module-wide DEFAULT precision bf16-compute (instances may override it)."""
    return _DEFAULT_PRECISION == "bf16-compute"


def get_activation_dtype():
    """(activation, gradient) storage types of the module-wide default precision."""
    t = torch.bfloat16 if bf16_compute() else torch.float32
    return t, t


# Who issues the launches of a forward / backward pass, an attribute of every MobileNet INSTANCE like the precision (`MobileNet.sequence`,
# `MobileNet.set_sequence`; not part of `get_config()` / the state dict):
#   "python"  _forward_impl / _backward_impl below (and _mobilenet_bc.py): one ctypes call and one torch allocation per launch - the default;
#   "native"  ONE C call per direction (ttk_mobilenet_forward / ttk_mobilenet_backward, csrc/mobilenet_seq.hip), which issues the same entry points
#             in the same order with the same arguments from one workspace allocation: the host enqueue of the eager step (data-parallel runs,
#             which cannot replay a graph) without the per-launch Python.  Results are those of "python" (tests/test_native_sequence_gpu.py:
#             launch lists equal, forward bitwise, gradients bitwise wherever "python" repeats itself bitwise).
_SEQUENCES = ("python", "native")
_DEFAULT_SEQUENCE = "python"


def _check_sequence(mode):
    if mode not in _SEQUENCES:
        raise ValueError(f'sequence must be "python" or "native", got {mode!r}')
    return mode


def set_sequence(mode):
    """Default launch sequence of MobileNet instances that have not been given one of their own (`MobileNet.set_sequence`): "python" or
    "native".  Kept for the scripts' `--sequence` flag."""
    global _DEFAULT_SEQUENCE
    mode = _check_sequence(mode)
    if mode == "native":
        _check_native_product()
    _DEFAULT_SEQUENCE = mode


def get_sequence() -> str:
    return _DEFAULT_SEQUENCE


def _check_native_product():
    """The native sequence is the PRODUCT configuration of the launch sequences and nothing else: with an experiment switch off its product value
    it refuses instead of silently running something other than what was asked for."""
    for name, value in (("_ELIDE_HEAD_INPUT", ("dw3_1", "dw4_1")), ("_EXP_TENSOR_HOOK", None)):
        have = globals()[name]
        if type(have) is not type(value) or have != value:
            raise ValueError(f'sequence "native" issues the product launch sequence only: mobilenet_v1.{name} is {have!r}, the product '
                             f'value is {value!r}; use sequence "python" for this experiment')


_BN_ROWS = _hip.TTK["BN_ROWS"]  # scale, beta, mean, rstd, ga, gb, gmean, aux - see include/ttk.h


class _BnArena:
    """The BatchNorm constant blocks bn[TTK_BN_ROWS][C] of all layers of one step, cut from ONE zeroed allocation:
    row TTK_BN_AUX (the operand magnitude bounds of the fp16-split GEMMs, include/ttk.h) must start at zero because
    the kernels raise it with atomicMax - one fill launch per step instead of one per layer."""

    def __init__(self, channels, device):
        self._buf = torch.zeros(sum(_BN_ROWS * c for c in channels), dtype=torch.float32, device=device)
        self._off = 0

    def take(self, C) -> torch.Tensor:
        n = _BN_ROWS * C
        blk = self._buf[self._off:self._off + n].view(_BN_ROWS, C)
        self._off += n
        return blk


class _Stage(NamedTuple):
    y: torch.Tensor            # raw conv output [B,H,W,C]
    bn: torch.Tensor           # BatchNorm constant block [8, C]
    skip: torch.Tensor | None  # residual input added before the ReLU of this stage's output
    skip_bn: torch.Tensor | None = None  # None: `skip` is a stored activation; else `skip` is a RAW conv output and this its constant block (ttk_*_rawskip)


def _part_buffer(B, H, W, device, blur=False, blocks=_BLOCKS, c0=_STEM_CHANNELS):
    """One scratch buffer large enough for every layer's [rows][2][C] partial sums."""
    L = _hip.lib()
    need = 0
    h = (H + 1) // 2
    need = max(need, (L.partial_rows_elementwise(B * h * h * 8) if c0 == _STEM_CHANNELS else L.anyc_partial_rows(B * h * h)) * 2 * c0)
    for _, cin, cout, stride in blocks:
        ho = (h - 1) // stride + 1
        if _tuned_c(cin):
            need = max(need, L.partial_rows_dwconv(B, h, h, cin, stride, True) * 2 * cin)     # dw bwd-data
            need = max(need, L.partial_rows_dwconv(B, h, h, cin, stride, False) * 2 * cin)    # dw fwd
            if blur and stride == 2:  # the stride-1 depthwise conv behind the blur
                need = max(need, L.partial_rows_dwconv(B, ho, ho, cin, 1, False) * 2 * cin, L.partial_rows_dwconv(B, ho, ho, cin, 1, True) * 2 * cin)
        else:  # (the family's rows depend on the pixel count alone: the input's covers forward, backward and the pair behind a blur)
            need = max(need, L.anyc_partial_rows(B * h * h) * 2 * cin)
        if _tuned_c(cin) and _tuned_c(cout):
            need = max(need, L.partial_rows_gemm(B * ho * ho, cin, cout) * 2 * cout, L.partial_rows_gemm(B * ho * ho, cout, cin, True) * 2 * cin)  # pw fwd / bwd-data
        else:
            need = max(need, L.partial_rows_gemm(B * ho * ho) * 2 * max(cin, cout))
        if _tuned_c(cout):
            need = max(need, L.partial_rows_elementwise(B * ho * ho * (cout // 4)) * 2 * cout)  # pool bwd
        else:
            need = max(need, L.anyc_partial_rows(B * ho * ho) * 2 * cout)
        h = ho
    return torch.empty(need, dtype=torch.float32, device=device)


class _Ctx:
    """Everything one forward pass leaves behind for its backward."""
    __slots__ = ("x", "stages", "a_in", "part", "dims", "pool_skip", "wparams", "HW", "B", "prep", "bf16_compute", "frozen", "blur", "blocks")


_FP32_STORAGE = 0  # the trailing TTK_STORE_* argument of the fp32 entry points with NO bit set (the header names the bits, not their absence): fp32 tensors


def _check_forward_inputs(x, params, buffers, blur, nblocks):
    """What comes from outside is checked once per forward call (everything else is allocated by the sequence itself) -> `blur` as a list per block."""
    blur = list(blur) if blur is not None else [None] * nblocks
    _hip.check_tensors([x], "input")
    _hip.check_tensors(params, "parameter")
    _hip.check_tensors(buffers, "BatchNorm buffer")
    _hip.check_tensors(blur, "blur kernel")
    return blur


def _grad_arena(params, device, zero):
    """One arena for every parameter gradient, each padded to 64 floats -> (arena, offs, grads): parameter i owns arena[offs[i]:offs[i + 1]],
    grads[i] is its view in the parameter's shape.  `zero`: the Python sequences' weight-gradient kernels accumulate into it (one fill launch)."""
    offs, total = [], 0
    for q in params:
        offs.append(total)
        total += (q.numel() + 63) // 64 * 64
    offs.append(total)
    arena = (torch.zeros if zero else torch.empty)(total, dtype=torch.float32, device=device)
    return arena, offs, [arena[o:o + q.numel()].view(q.shape) for o, q in zip(offs, params)]


def _announce(arena, offs, params, first, last):
    """Parameters first .. last-1 are final: their slices of the arena (padding included) may travel - to `grad_ready_hook`, where one is set."""
    if grad_ready_hook is not None:
        grad_ready_hook(arena, [(params[i], offs[i], offs[i + 1]) for i in range(first, last)])


_IDENTITY_BN: dict = {}


def _identity_bn(C, device):
    """A fresh constant block of the identity map (scale = rstd = 1, beta = mean = 0): the blurred tensor of a BlurPool block has
    no BatchNorm of its own, but every consumer forms its input as relu(bn(y)) on load - relu(t) = t for a blur of
    non-negative activations.  The backward rows (ga, gb, gmean) are written by ttk_bn_bwd_frozen."""
    key = (device.type, device.index, C)
    if key not in _IDENTITY_BN:
        t = torch.zeros((_BN_ROWS, C), dtype=torch.float32, device=device)
        t[_hip.TTK["BN_SCALE"]] = 1.0
        t[_hip.TTK["BN_RSTD"]] = 1.0
        _IDENTITY_BN[key] = t
    return _IDENTITY_BN[key].clone()


def _forward_impl(x, params, buffers, momentum, eps, training, frozen=False, blur=None, blocks=_BLOCKS):
    """Launches the forward kernels.  `params`: flat list [conv1.w, bn1.w, bn1.b, (dw.w, bn_dw.w,
    bn_dw.b, pw.w, bn_sep.w, bn_sep.b) x 13]; `buffers`: flat list of (running_mean, running_var,
    num_batches_tracked) per BN in the same order; `blur`: per block, the BlurPool2D kernel as a depthwise weight
    [Cin,1,3,3] (use_blurpool, strided blocks) or None; `blocks`: the instance's (width-scaled) block table.  Per layer, a shape the
    tuned kernels accept runs on them; every other layer runs on the any-channel-count family (ttk_anyc_*) - same contracts, same layout."""
    L = _hip.lib()
    blur = _check_forward_inputs(x, params, buffers, blur, len(blocks))
    c0 = params[0].shape[0]
    p = _hip.fast_ptr
    dev = x.device
    B, _, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    part = _part_buffer(B, H, W, dev, any(b is not None for b in blur), blocks, c0)
    ctx = _Ctx()
    ctx.x, ctx.part, ctx.B, ctx.blocks = x, part, B, blocks
    ctx.blur = []
    ctx.frozen = frozen  # backward through eval-mode BatchNorm: the fixed affine map (ttk_bn_bwd_frozen)
    ctx.stages, ctx.a_in, ctx.dims = [], [], []
    ctx.bf16_compute = False
    bns = _BnArena([c0] + [c for _, cin, cout, _ in blocks for c in (cin, cout)], dev)

    def pivot(bi):
        """The statistics pivot of BatchNorm `bi` (include/ttk.h): its running mean - the producer sums y - pivot, the finalisation adds
        it back (and only then updates the running mean)."""
        return p(buffers[3 * bi])

    def finalize(bn, rows, C, count, gamma, beta, bi):
        rm, rv, nbt = buffers[3 * bi], buffers[3 * bi + 1], buffers[3 * bi + 2]
        if training:
            L.call("ttk_bn_fwd_finalize", p(part), pivot(bi), rows, C, count, p(gamma), p(beta), p(rm), p(rv), p(nbt),
                   float(momentum), float(eps), p(bn))
        else:
            L.call("ttk_bn_eval_prepare", p(gamma), p(beta), p(rm), p(rv), float(eps), C, p(bn))
            # eval-mode statistics: the fp16-split GEMMs (forward here; the backward too when the convolutions train with frozen
            # statistics) still scale their operands by a bound of THIS batch's activations, from the producers' partial sums - without
            # it the pieces are unscaled: values above 65 504 overflow, small activations fall into fp16's subnormal range
            L.call("ttk_bn_frozen_bound", p(part), pivot(bi), rows, C, count, p(bn))

    def exp_hook(k, y):
        if _EXP_TENSOR_HOOK is not None:
            _EXP_TENSOR_HOOK("y", k, y)

    part_arg = p(part)
    # forward and data-gradient weight operands of all 13 pointwise convs, one launch
    # (the tuned pointwise layers; the any-channel-count GEMMs read the raw weights)
    tuned_pw = [k for k, (_, cin, cout, _) in enumerate(blocks) if _tuned_c(cin) and _tuned_c(cout)]
    ctx.prep = [None] * len(blocks)
    if tuned_pw:
        sizes = [L.pwconv_prepared_bytes(blocks[k][1], blocks[k][2]) for k in tuned_pw]
        pool = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
        for k, t in zip(tuned_pw, torch.split(pool, sizes)):
            ctx.prep[k] = t
        L.pwconv_prepare_weights([params[3 + 6 * k + 3] for k in tuned_pw], [ctx.prep[k] for k in tuned_pw])
    # ---- stem (reference :122-126,161-163)
    y0 = torch.empty((B, Ho, Wo, c0), dtype=torch.float32, device=dev)
    bn = bns.take(c0)
    if c0 == _STEM_CHANNELS:
        L.call("ttk_stem_fwd", p(x), p(params[0]), p(y0), part_arg, pivot(0), B, H, W, _FP32_STORAGE)
        finalize(bn, L.partial_rows_elementwise(B * Ho * Wo * 8), 32, B * Ho * Wo, params[1], params[2], 0)
    else:
        L.call("ttk_anyc_stem_fwd", p(x), p(params[0]), p(y0), part_arg, pivot(0), B, H, W, c0)
        finalize(bn, L.anyc_partial_rows(B * Ho * Wo), c0, B * Ho * Wo, params[1], params[2], 0)
    prev = _Stage(y0, bn, None)
    ctx.stages.append(prev)
    h, w_ = Ho, Wo
    pi, bi = 3, 1
    def dw_fwd(st, a_out, w, y, pv, hh, ww, C, stride):
        """One depthwise launch on the output of stage `st` -> the rows of partial sums it wrote."""
        yprev, bn_prev, skip_prev = st.y, st.bn, st.skip
        if _tuned_c(C):
            if st.skip_bn is not None:
                L.call("ttk_dwconv3x3_fwd_rawskip", p(yprev), p(bn_prev), p(skip_prev), p(st.skip_bn), p(a_out), p(w), p(y), part_arg, pv, B, hh, ww, C, stride)
            else:
                L.call("ttk_dwconv3x3_fwd", p(yprev), p(bn_prev), p(skip_prev), p(a_out), p(w), p(y), part_arg, pv, B, hh, ww, C, stride, _FP32_STORAGE)
            return L.partial_rows_dwconv(B, hh, ww, C, stride, False)
        L.call("ttk_anyc_dw_fwd", p(yprev), p(bn_prev), p(skip_prev), p(a_out), p(w), p(y), part_arg, pv, B, hh, ww, C, stride)
        return L.anyc_partial_rows(B * ((hh - 1) // stride + 1) * ((ww - 1) // stride + 1))

    for name, cin, cout, stride in blocks:
        w_dw, g_dw, b_dw, w_pw, g_pw, b_pw = params[pi:pi + 6]
        pi += 6
        has_skip = stride == 1 and cin == cout
        ho, wo = (h - 1) // stride + 1, (w_ - 1) // stride + 1
        # The input of a residual block is stored (a_in: written by its depthwise forward, read back by its depthwise backward) - except for the
        # FIRST block of a chain where _ELIDE_HEAD_INPUT says so: its input relu(bn(y_prev)) has no residual of its own, every consumer either
        # loads y_prev already or loads it in place of the stored tensor (the raw residual operand, include/ttk.h).  (The any-channel-count
        # family keeps storing.)
        head = has_skip and prev.skip is None and _tuned_c(cin) and (_ELIDE_HEAD_INPUT is True or (bool(_ELIDE_HEAD_INPUT) and name in _ELIDE_HEAD_INPUT))
        a_in = torch.empty_like(prev.y) if (has_skip and not head) else None
        ydw = torch.empty((B, ho, wo, cin), dtype=torch.float32, device=dev)
        k = len(ctx.dims)
        if blur[k] is not None:
            # reference :43-55 - BlurPool2D (binomial 3x3, stride 2) then the depthwise conv at stride 1: two launches of the
            # same depthwise kernel; the blurred tensor crosses HBM once with the identity constant block (its partial sums
            # are written to the scratch rows and overwritten by the next launch)
            t = torch.empty((B, ho, wo, cin), dtype=torch.float32, device=dev)
            dw_fwd(prev, None, blur[k], t, None, h, w_, cin, stride)
            st_t = _Stage(t, _identity_bn(cin, dev), None)
            dw_rows = dw_fwd(st_t, None, w_dw, ydw, pivot(bi), ho, wo, cin, 1)
            ctx.blur.append((st_t, blur[k]))
        else:
            dw_rows = dw_fwd(prev, a_in, w_dw, ydw, pivot(bi), h, w_, cin, stride)
            ctx.blur.append(None)
        exp_hook(k, ydw)
        bn_dw = bns.take(cin)
        finalize(bn_dw, dw_rows, cin, B * ho * wo, g_dw, b_dw, bi)
        ypw = torch.empty((B, ho, wo, cout), dtype=torch.float32, device=dev)
        M = B * ho * wo
        if ctx.prep[k] is not None:
            L.call("ttk_pwconv1x1_fwd", p(ydw), p(bn_dw), None, p(ypw), part_arg, pivot(bi + 1), M, cin, cout, p(ctx.prep[k]), _FP32_STORAGE)
            pw_rows = L.partial_rows_gemm(M, cin, cout)
        else:
            L.call("ttk_anyc_pw_fwd", p(ydw), p(bn_dw), p(w_pw), p(ypw), part_arg, pivot(bi + 1), M, cin, cout)
            pw_rows = L.partial_rows_gemm(M)
        exp_hook(k, ypw)
        bn_pw = bns.take(cout)
        finalize(bn_pw, pw_rows, cout, M, g_pw, b_pw, bi + 1)
        bi += 2
        ctx.stages.append(_Stage(ydw, bn_dw, None))
        prev = _Stage(ypw, bn_pw, skip=prev.y, skip_bn=prev.bn) if head else _Stage(ypw, bn_pw, a_in)
        ctx.stages.append(prev)
        ctx.a_in.append(a_in)
        ctx.dims.append((h, w_, ho, wo, cin, cout, stride, has_skip))
        h, w_ = ho, wo
    C = prev.y.shape[-1]
    feat = torch.empty((B, C), dtype=torch.float32, device=dev)
    if _tuned_c(C) and prev.skip_bn is not None:
        L.call("ttk_avgpool_fwd_rawskip", p(prev.y), p(prev.bn), p(prev.skip), p(prev.skip_bn), p(feat), B, h * w_, C)
    elif _tuned_c(C):
        L.call("ttk_avgpool_fwd", p(prev.y), p(prev.bn), p(prev.skip), p(feat), B, h * w_, C, _FP32_STORAGE)
    else:
        L.call("ttk_anyc_avgpool_fwd", p(prev.y), p(prev.bn), p(prev.skip), p(feat), B, h * w_, C)
    ctx.HW = h * w_
    return feat, ctx


# Data-parallel hook: called as hook(arena, [(param, lo, hi), ...]) whenever a block's parameter gradients - elements
# [lo, hi) of the flat gradient arena - are final, in reverse layer order (trackertraincode.parallel.GradAllReduce.on_ready
# all-reduces the ranges in place).
grad_ready_hook = None


# Settled A/Bs of the backward sequence (the losing arms are in the git history):
#   everything on ONE stream - weight-gradient GEMMs on a second stream measured slower (69.4 k against 70.1 k crops/s);
#   weight and data gradient of the early pointwise layers in one kernel wherever ttk_pwconv1x1_bwd_fused_rows() > 0 (profiles/pw_bwd_fused_wide.txt);
#   depthwise weight gradient as workgroup rows folded by the launch that finalises the producer's BatchNorm backward: 68.9 k against 68.4 k (atomics)
#   and 67.3 k (rows + a fold launch of their own) - profiles/r05_bc_gemm_variants.txt.
_USE_WGRAD_STREAM = False  # inert: bench.py saves and restores it, nothing reads it
# TTK_DETERMINISTIC=1: every weight-gradient reduction runs in a fixed order (slices of M stored to scratch and folded
# by a second kernel instead of fp32 atomics): two runs of a step give bitwise equal gradients.
_DETERMINISTIC = os.environ.get("TTK_DETERMINISTIC", "0") != "0"
# The first block of a chain of residual blocks (dw3_1, dw4_1, dw5_1, dw6) need not store its input: it is relu(bn(y)) of the producer alone, and its
# consumers can form it on load (the ttk_*_rawskip entry points).  True: none of the four stores it; False: all do (the stored form: the A/B run,
# tests/test_rawskip_gpu.py); a tuple of block names: those blocks do not.  The product elides the two large ones.  Behind dw5_1 and dw6 the raw form's
# consumer measured slower than the stored one (the 9 x 9 x 512 forward of dw5_2 54.1 -> 60.1 us, the pool forward 22.7 -> 23.3 us: the stored input was
# still in the memory-side cache, the raw tensor three launches back is not), so these two keep storing - profiles/head_block_input.txt.
_ELIDE_HEAD_INPUT = ("dw3_1", "dw4_1")
# Experiment hook of tools/soak.py (None in the product): called as _EXP_TENSOR_HOOK(kind, block, tensor) right after a kernel has produced
# a gradient ("g": with respect to a conv output before its BatchNorm) or an activation ("y": a raw conv output) of the fp32 path, e.g. to round it
# to the bf16 grid in place - how much of the bf16-compute path's soak gap each tensor class explains (profiles/r06_soak_rounding_ab.txt).
_EXP_TENSOR_HOOK = None


def _backward_impl(ctx: _Ctx, gfeat, params):
    L = _hip.lib()
    _hip.check_tensors([gfeat], "gradient")
    _hip.check_tensors(params, "parameter")
    p = _hip.fast_ptr
    B, part, blocks = ctx.B, ctx.part, ctx.blocks
    arena, offs, grads = _grad_arena(params, gfeat.device, zero=True)

    def exp_hook(k, g):
        if _EXP_TENSOR_HOOK is not None:
            _EXP_TENSOR_HOOK("g", k, g)
    last = ctx.stages[-1]
    C = last.y.shape[-1]

    def bwd_finalize(stage: _Stage, rows, count, gi):
        """BatchNorm backward constants of `stage` + its dgamma/dbeta -> grads[gi], grads[gi+1]"""
        Cc = stage.y.shape[-1]
        if ctx.frozen:  # frozen statistics (fine-tuning): no sums, no gamma / beta gradient
            L.call("ttk_bn_bwd_frozen", p(stage.bn), Cc)
            return
        L.call("ttk_bn_bwd_finalize", p(part), rows, Cc, count, p(params[gi]), p(stage.bn), p(grads[gi]), p(grads[gi + 1]), 0)

    # Scratch of the tuned layers' weight gradients; every launch of this backward runs on the one current stream, so each buffer serves one launch after the other.
    wg_scratch = dw_rows = None
    if _DETERMINISTIC:
        # one scratch buffer for every weight-gradient reduction of this backward (used one after the other on one stream):
        # slices / workgroups store partial results there and a second kernel folds them in a fixed order
        pw_dims = [d for d in ctx.dims if _tuned_c(d[4]) and _tuned_c(d[5])]
        dw_dims = [(d, bl) for d, bl in zip(ctx.dims, ctx.blur) if _tuned_c(d[4])]
        need = max([L.pwconv_wgrad_partial_bytes(B * d[2] * d[3], d[4], d[5]) for d in pw_dims] + [0])
        need = max(need, L.cdll.ttk_stem_wgrad_partial_bytes())
        need = max([need] + [L.cdll.ttk_pwconv1x1_bwd_fused_partial_bytes(B * d[2] * d[3], d[4], d[5]) for d in pw_dims])
        need = max([need] + [L.partial_rows_dwconv(B, d[0], d[1], d[4], d[6], True) * 9 * d[4] * 4 for d, _ in dw_dims])
        need = max([need] + [L.partial_rows_dwconv(B, d[2], d[3], d[4], 1, True) * 9 * d[4] * 4 for d, bl in dw_dims if bl is not None])
        wg_scratch = torch.empty(need // 4, dtype=torch.float32, device=gfeat.device)
    # the weight gradient of the wide pointwise layers (Cin, Cout multiples of 256) always reduces slice partials in a fixed order
    # (csrc/pwconv_r.hip: faster than float atomics for 256 x 256 tiles): its scratch, in every mode
    pw_need = max([L.pwconv_wgrad_scratch_bytes(B * d[2] * d[3], d[4], d[5]) for d in ctx.dims if _tuned_c(d[4]) and _tuned_c(d[5])] + [0])
    pw_scratch = wg_scratch if (wg_scratch is not None and wg_scratch.numel() * 4 >= pw_need) else (
        torch.empty(pw_need // 4, dtype=torch.float32, device=gfeat.device) if pw_need else None)
    # the fused depthwise weight gradient: workgroup rows, folded by the launch that finalises the producer's BatchNorm backward
    # (the BlurPool blocks and frozen fine-tuning keep float atomics unless deterministic: they pass `wg_scratch`, not these rows)
    rows_layers = [d for d, bl in zip(ctx.dims, ctx.blur) if bl is None and _tuned_c(d[4])]
    if rows_layers and not _DETERMINISTIC and not ctx.frozen:
        need = max(L.partial_rows_dwconv(B, d[0], d[1], d[4], d[6], True) * 9 * d[4] for d in rows_layers)
        dw_rows = torch.empty(need, dtype=torch.float32, device=gfeat.device)

    # The any-channel-count layers (width-scaled backbones): ONE scratch buffer for their weight gradients - workgroup / slice rows that
    # the entry points fold in a fixed order (no atomics in that family, in any mode); used by one launch after the other on this stream.
    _, _, H, W = ctx.x.shape
    c0 = ctx.stages[0].y.shape[-1]
    any_need = 0 if c0 == _STEM_CHANNELS else L.anyc_wgrad_scratch_bytes("stem", B, H, W, c0)
    for d, bl in zip(ctx.dims, ctx.blur):
        if not _tuned_c(d[4]):
            any_need = max(any_need, L.anyc_wgrad_scratch_bytes("dw", B, d[2], d[3], d[4]) if bl is not None else L.anyc_wgrad_scratch_bytes("dw", B, d[0], d[1], d[4]))
        if not (_tuned_c(d[4]) and _tuned_c(d[5])):
            any_need = max(any_need, L.anyc_wgrad_scratch_bytes("pw", B * d[2] * d[3], d[4], d[5]))
    any_scratch = torch.empty(any_need // 4, dtype=torch.float32, device=gfeat.device) if any_need else None

    g = torch.empty(last.y.shape, dtype=torch.float32, device=last.y.device)
    if _tuned_c(C):
        if last.skip_bn is not None:
            L.call("ttk_avgpool_bwd_rawskip", p(gfeat), p(last.y), p(last.bn), p(last.skip), p(last.skip_bn), p(g), p(part), B, ctx.HW, C)
        else:
            L.call("ttk_avgpool_bwd", p(gfeat), p(last.y), p(last.bn), p(last.skip), p(g), p(part), B, ctx.HW, C, _FP32_STORAGE)
        bwd_finalize(last, L.partial_rows_elementwise(B * ctx.HW * (C // 4)), B * ctx.HW, len(params) - 2)
    else:
        L.call("ttk_anyc_avgpool_bwd", p(gfeat), p(last.y), p(last.bn), p(last.skip), p(g), p(part), B, ctx.HW, C)
        bwd_finalize(last, L.anyc_partial_rows(B * ctx.HW), B * ctx.HW, len(params) - 2)
    exp_hook(len(blocks), g)

    def dw_bwd(g_dw, st_dw, w, skip_grad, st_prev, a_in, g_prev, dw, acc, rows, hh, ww, C, stride):
        """One tuned depthwise data-gradient launch into the output of stage `st_prev` (its residual operand stored or raw)."""
        if st_prev.skip_bn is not None and a_in is None:
            L.call("ttk_dwconv3x3_bwd_data_rawskip", p(g_dw), p(st_dw.y), p(st_dw.bn), p(w), p(skip_grad), p(st_prev.y), p(st_prev.bn), p(st_prev.skip),
                   p(st_prev.skip_bn), p(g_prev), p(part), p(dw), acc, p(rows), B, hh, ww, C, stride)
        else:
            # (a stored a_in stands for the whole block input: the residual operand, stored or raw, is not read)
            L.call("ttk_dwconv3x3_bwd_data", p(g_dw), p(st_dw.y), p(st_dw.bn), p(w), p(skip_grad), p(st_prev.y), p(st_prev.bn),
                   p(st_prev.skip if st_prev.skip_bn is None else None), p(a_in), p(g_prev), p(part), p(dw), acc, p(rows), B, hh, ww, C, stride, _FP32_STORAGE)

    for k in range(len(blocks) - 1, -1, -1):
        h, w_, ho, wo, cin, cout, stride, has_skip = ctx.dims[k]
        pi = 3 + 6 * k
        w_dw, w_pw = params[pi], params[pi + 3]
        st_prev, st_dw, st_pw = ctx.stages[2 * k], ctx.stages[2 * k + 1], ctx.stages[2 * k + 2]
        a_in = ctx.a_in[k]
        M = B * ho * wo
        # -- pointwise: weight gradient, data gradient (+ bn_dw backward sums)
        dW = grads[pi + 3]
        g_dw = torch.empty(st_dw.y.shape, dtype=torch.float32, device=st_dw.y.device)
        pw_tuned = ctx.prep[k] is not None
        fused_rows = L.cdll.ttk_pwconv1x1_bwd_fused_rows(M, cin, cout) if pw_tuned else 0
        if not pw_tuned:
            # any-channel-count layer: exact-fp32 MFMA GEMMs from the raw weights; the weight gradient is slice rows + a fixed-order fold
            L.call("ttk_anyc_pw_bwd_weight", p(g), p(st_pw.y), p(st_pw.bn), p(st_dw.y), p(st_dw.bn), p(dW), 0, p(any_scratch), M, cin, cout)
            L.call("ttk_anyc_pw_bwd_data", p(g), p(st_pw.y), p(st_pw.bn), p(w_pw), p(st_dw.y), p(st_dw.bn), p(g_dw), p(part), M, cin, cout)
            bwd_finalize(st_dw, L.partial_rows_gemm(M), M, pi + 1)
        elif fused_rows > 0:
            # the first five pointwise layers (32 -> 64 .. 256 -> 256: HBM-bound, the largest activations): weight and data gradient in ONE kernel - g,
            # the conv output and the depthwise output are read once instead of twice (csrc/pw_bwd_fused.hip)
            L.call("ttk_pwconv1x1_bwd_fused", p(g), p(st_pw.y), p(st_pw.bn), p(w_pw), p(ctx.prep[k]), p(st_dw.y), p(st_dw.bn), p(g_dw), p(dW),
                   p(wg_scratch), p(part), M, cin, cout)
            bwd_finalize(st_dw, fused_rows, M, pi + 1)
        else:
            partial = wg_scratch if _DETERMINISTIC else (pw_scratch if L.pwconv_wgrad_scratch_bytes(M, cin, cout) else None)
            L.call("ttk_pwconv1x1_bwd_weight", p(g), p(st_pw.y), p(st_pw.bn), p(st_dw.y), p(st_dw.bn), p(dW), p(partial), M, cin, cout, _FP32_STORAGE)
            L.call("ttk_pwconv1x1_bwd_data", p(g), p(st_pw.y), p(st_pw.bn), None, p(st_dw.y), p(st_dw.bn), p(g_dw), p(part), M,
                   cin, cout, p(ctx.prep[k]), _FP32_STORAGE)
            bwd_finalize(st_dw, L.partial_rows_gemm(M, cout, cin, True), M, pi + 1)
        exp_hook(k, g_dw)
        # -- depthwise: data gradient (+ residual gradient, + producer's bn sums) with the fused weight gradient
        dWd = grads[pi]
        g_prev = torch.empty(st_prev.y.shape, dtype=torch.float32, device=st_prev.y.device)
        gi_prev = pi - 2 if k > 0 else 1
        if not _tuned_c(cin):
            # any-channel-count layer (BlurPool blocks: the same two steps as below)
            if ctx.blur[k] is not None:
                st_t, w_blur = ctx.blur[k]
                g_t = torch.empty(st_t.y.shape, dtype=torch.float32, device=st_t.y.device)
                L.call("ttk_anyc_dw_bwd_data", p(g_dw), p(st_dw.y), p(st_dw.bn), p(w_dw), None, p(st_t.y), p(st_t.bn), None, None, p(g_t),
                       p(part), p(dWd), 0, p(any_scratch), B, ho, wo, cin, 1)
                L.call("ttk_bn_bwd_frozen", p(st_t.bn), cin)
                L.call("ttk_anyc_dw_bwd_data", p(g_t), p(st_t.y), p(st_t.bn), p(w_blur), None, p(st_prev.y), p(st_prev.bn), p(st_prev.skip),
                       None, p(g_prev), p(part), None, 0, None, B, h, w_, cin, stride)
            else:
                L.call("ttk_anyc_dw_bwd_data", p(g_dw), p(st_dw.y), p(st_dw.bn), p(w_dw), p(g) if has_skip else None, p(st_prev.y),
                       p(st_prev.bn), p(st_prev.skip), p(a_in), p(g_prev), p(part), p(dWd), 0, p(any_scratch), B, h, w_, cin, stride)
            bwd_finalize(st_prev, L.anyc_partial_rows(B * h * w_), B * h * w_, gi_prev)
        elif ctx.blur[k] is not None:
            # BlurPool block: through the stride-1 conv to the blurred tensor (its "BatchNorm" is the identity: ga = 1, gb = gmean = 0;
            # the mask [t > 0] only drops gradient that the producer's own mask drops as well - t = 0 means every tap was 0), then
            # through the fixed blur kernel (no weight gradient) to the block input
            st_t, w_blur = ctx.blur[k]
            g_t = torch.empty(st_t.y.shape, dtype=torch.float32, device=st_t.y.device)
            dw_bwd(g_dw, st_dw, w_dw, None, st_t, None, g_t, dWd, 1, wg_scratch, ho, wo, cin, 1)  # (float atomics unless deterministic: rows + an own fold launch measured slower)
            L.call("ttk_bn_bwd_frozen", p(st_t.bn), cin)
            dw_bwd(g_t, st_t, w_blur, None, st_prev, None, g_prev, None, 0, None, h, w_, cin, stride)
            bwd_finalize(st_prev, L.partial_rows_dwconv(B, h, w_, cin, stride, True), B * h * w_, gi_prev)
        elif not _DETERMINISTIC and not ctx.frozen:
            # workgroup rows, folded by the launch that finalises the producer's BatchNorm backward
            rows = L.partial_rows_dwconv(B, h, w_, cin, stride, True)
            dw_bwd(g_dw, st_dw, w_dw, g if has_skip else None, st_prev, a_in, g_prev, dWd, 2, dw_rows, h, w_, cin, stride)
            L.call("ttk_bc_bn_bwd_finalize_fold", p(part), rows, cin, B * h * w_, p(params[gi_prev]), p(st_prev.bn), p(grads[gi_prev]), p(grads[gi_prev + 1]), 0,
                   p(dw_rows), rows, 9 * cin, p(dWd), 1)
        else:
            dw_bwd(g_dw, st_dw, w_dw, g if has_skip else None, st_prev, a_in, g_prev, dWd, 1, wg_scratch, h, w_, cin, stride)
            bwd_finalize(st_prev, L.partial_rows_dwconv(B, h, w_, cin, stride, True), B * h * w_, gi_prev)
        g = g_prev
        exp_hook(k, g)
        _announce(arena, offs, params, pi, pi + 6)  # this block's conv + bn_dw gradients and its own bn_sep gradients are final
    st0 = ctx.stages[0]
    if c0 == _STEM_CHANNELS:
        L.call("ttk_stem_bwd_weight", p(g), p(st0.y), p(st0.bn), p(ctx.x), p(grads[0]), 1, p(wg_scratch), B, H, W, _FP32_STORAGE)
    else:
        L.call("ttk_anyc_stem_bwd_weight", p(g), p(st0.y), p(st0.bn), p(ctx.x), p(grads[0]), 0, p(any_scratch), B, H, W, c0)
    _announce(arena, offs, params, 0, 3)
    return grads


class _NativeCtx:
    """What a native forward pass leaves behind for its backward: the plan, ONE workspace and the inputs the backward reads again."""
    __slots__ = ("plan", "ws", "x", "blur", "blur_arr")


def _ptr_array(ts):
    return (_hip.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _native_forward(x, params, buffers, momentum, eps, mode, blur, precision, blocks):
    """ttk_mobilenet_forward: the launches of _forward_impl / _mobilenet_bc.forward_impl as one C call.  `mode`: "train" | "frozen" | "eval"."""
    _check_native_product()
    L = _hip.lib()
    blur = _check_forward_inputs(x, params, buffers, blur, len(blocks))
    B, _, H, W = x.shape
    plan =L.mobilenet_plan(B, H, W, params[0].shape[0], tuple((cin, cout, stride) for _, cin, cout, stride in blocks), tuple(b is not None for b in blur),
                            mode, precision, _DETERMINISTIC)
    c = _NativeCtx()
    c.plan, c.x, c.blur = plan, x, blur  # (blur: the tensors behind blur_arr stay alive)
    c.blur_arr = _ptr_array(blur) if any(b is not None for b in blur) else None
    c.ws = torch.empty(plan.ws_bytes[0], dtype=torch.uint8, device=x.device)
    feat = torch.empty((B, blocks[-1][2]), dtype=torch.float32, device=x.device)
    L.mobilenet_forward(plan, x, _ptr_array(params), _ptr_array(buffers), c.blur_arr, float(momentum), float(eps), c.ws, feat)
    return feat, c


def _native_backward(c: _NativeCtx, gfeat, params):
    """ttk_mobilenet_backward; the gradient arena and `grad_ready_hook` as in _backward_impl (the C side announces parameter ranges through a callback)."""
    L = _hip.lib()
    _hip.check_tensors([gfeat], "gradient")
    _hip.check_tensors(params, "parameter")
    plan = c.plan
    arena, offs, grads = _grad_arena(params, gfeat.device, zero=False)  # (zeroed by the C side on this stream)
    if offs[-1] != plan.arena_floats or len(params) != plan.nparams:
        raise RuntimeError(f"native backward: the parameters take {offs[-1]} arena floats in {len(params)} tensors, the plan {plan.arena_floats} in {plan.nparams}")
    bws = torch.empty(plan.ws_bytes[1], dtype=torch.uint8, device=gfeat.device)
    cb, failed = None, []
    if grad_ready_hook is not None:
        def ready(_user, first, last):  # (an exception must not unwind through the C frames: kept, raised after the call)
            if not failed:
                try:
                    _announce(arena, offs, params, first, last)
                except BaseException as e:  # noqa: BLE001
                    failed.append(e)
        cb = _hip.MOBILENET_READY_FN(ready)
    L.mobilenet_backward(plan, gfeat, c.x, _ptr_array(params), c.blur_arr, c.ws, bws, arena, cb)
    if failed:
        raise failed[0]
    return grads


class _MobileNetFn(torch.autograd.Function):
    """One autograd node for the whole backbone: saves raw conv outputs + BN constants."""

    @staticmethod
    def forward(ctx, x, momentum, eps, buffers, frozen, blur, precision, blocks, sequence, *params):
        if sequence == "native":
            feat, c = _native_forward(x, params, buffers, momentum, eps, "frozen" if frozen else "train", blur, precision, blocks)
        elif precision == "bf16-compute":
            feat, c = _mobilenet_bc.forward_impl(_THIS, x, params, buffers, momentum, eps, training=not frozen, frozen=frozen, blur=blur)
        else:
            feat, c = _forward_impl(x, params, buffers, momentum, eps, training=not frozen, frozen=frozen, blur=blur, blocks=blocks)
        ctx.c = c
        ctx.nparams = len(params)
        ctx.save_for_backward(*params)
        return feat

    @staticmethod
    def backward(ctx, gfeat):
        params = ctx.saved_tensors
        if isinstance(ctx.c, _NativeCtx):
            grads = _native_backward(ctx.c, gfeat.contiguous(), params)
        elif ctx.c.bf16_compute:
            grads = _mobilenet_bc.backward_impl(_THIS, ctx.c, gfeat.contiguous(), params)
        else:
            grads = _backward_impl(ctx.c, gfeat.contiguous(), params)
        ctx.c = None
        return (None, None, None, None, None, None, None, None, None, *grads)


class MobileNet(nn.Module):
    """Reference :95-189.  `forward(x) -> (features, [out1..out5])`."""

    def __init__(self, num_classes=1000, widen_factor=1.0, input_channel=1, momentum=0.1, dropout=0.0,
                 use_blurpool=False, return_only_featuremap=False):
        super().__init__()
        if input_channel != 1:
            raise NotImplementedError("the HIP backbone is built for input_channel=1 (the pose estimator's configuration, models.py:220)")
        self.widen_factor = widen_factor
        c0, self._blocks = _scaled_blocks(widen_factor)  # ValueError for a width the kernels do not take
        if return_only_featuremap:
            raise NotImplementedError("return_only_featuremap is not used by the pose estimator")

        def block(inplanes, planes, stride=1):
            return DepthWiseBlock(inplanes, planes, stride=stride, momentum=momentum, use_blurpool=use_blurpool)

        self.use_blurpool = bool(use_blurpool)
        self.sequence = None   # None = the module-wide default (set_sequence); "python" | "native" through MobileNet.set_sequence
        self.precision = None  # None = the module-wide default (set_activation_dtype); "fp32" | "bf16-compute" through set_precision
        self.conv1 = nn.Conv2d(input_channel, c0, kernel_size=5, stride=2, padding=2, bias=False)
        self.bn1 = NormalizationLayer(c0, momentum=momentum)
        self.relu = ActivationFunc(inplace=True)
        for name, cin, cout, stride in self._blocks:
            setattr(self, name, block(cin, cout, stride))
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.num_features = int(1024 * widen_factor)  # reference :146,150
        self.num_intermediate_features = [cout for name, _, cout, _ in self._blocks if name in _INTERMEDIATES]
        if num_classes:
            self.drop = nn.Dropout(p=dropout) if dropout > 0.0 else nn.Identity()
            self.fc = nn.Linear(self.num_features, num_classes)
        # reference :155-158 - N(0, sqrt(2/(k*k*Cout))) for EVERY conv, 1x1 included
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2.0 / n))

    # ---- precision of the training kernels (an attribute of the instance; not in the checkpoint) ------------------
    def set_precision(self, mode):
        """"fp32" | "bf16-compute" for THIS backbone (None: follow the module-wide default again).  Returns self."""
        mode = None if mode is None else _check_precision(mode)
        self._check_width_precision(mode)
        self.precision = mode
        return self

    # ---- who issues the launches (an attribute of the instance; not in the checkpoint) ---------------------------
    def set_sequence(self, mode):
        """"python" | "native" for THIS backbone (None: follow the module-wide default again).  Returns self."""
        mode = None if mode is None else _check_sequence(mode)
        if mode == "native":
            _check_native_product()
        self.sequence = mode
        return self

    def effective_sequence(self) -> str:
        return self.sequence if getattr(self, "sequence", None) is not None else _DEFAULT_SEQUENCE

    def effective_precision(self) -> str:
        return self.precision if getattr(self, "precision", None) is not None else _DEFAULT_PRECISION

    def _check_width_precision(self, mode):
        if mode == "bf16-compute" and self._blocks != _BLOCKS:
            raise ValueError(f'precision "bf16-compute" is built for widen_factor=1.0 only (its kernels work on 64-channel blocks); this backbone '
                             f'has widen_factor={self.widen_factor}: use "fp32"')

    def kernel_plan(self):
        """[(layer, "tuned" | "anyc"), ...] in launch order: which kernel family runs each layer of the fp32 HIP path.  A shape the tuned
        kernels accept (channel counts that are powers of two in 32..1024) runs on them; every other layer runs on the any-channel-count
        family (ttk_anyc_*).  Pure Python; needs no GPU."""
        fam = lambda ok: "tuned" if ok else "anyc"
        plan = [("conv1", fam(self.conv1.out_channels == _STEM_CHANNELS))]
        for name, cin, cout, _ in self._blocks:
            plan.append((f"{name}.conv_dw", fam(_tuned_c(cin))))
            plan.append((f"{name}.conv_sep", fam(_tuned_c(cin) and _tuned_c(cout))))
        plan.append(("avgpool", fam(_tuned_c(self.num_features))))
        return plan

    # ---- parameter plumbing -----------------------------------------------------------------
    def _bns(self):
        yield self.bn1
        for name, *_ in self._blocks:
            blk = getattr(self, name)
            yield blk.bn_dw
            yield blk.bn_sep

    def _flat_params(self):
        ps = [self.conv1.weight, self.bn1.weight, self.bn1.bias]
        for name, *_ in self._blocks:
            b = getattr(self, name)
            ps += [b.dw_weight, b.bn_dw.weight, b.bn_dw.bias, b.conv_sep.weight, b.bn_sep.weight, b.bn_sep.bias]
        return ps

    def _blur_weights(self):
        """Per block: the BlurPool2D kernel as a depthwise weight (use_blurpool, strided blocks) or None."""
        if not self.use_blurpool:
            return None
        return [getattr(self, name).conv_dw[0].depthwise_weight() if getattr(self, name).blurpool else None for name, *_ in self._blocks]

    def _flat_buffers(self):
        out = []
        for bn in self._bns():
            out += [bn.running_mean, bn.running_var, bn.num_batches_tracked]
        return out

    def _check(self, x):
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 1:
            raise ValueError(f"expected float32 [B,1,H,W] input, got {tuple(x.shape)} {x.dtype}")
        moms = {bn.momentum for bn in self._bns()}
        epss = {bn.eps for bn in self._bns()}
        if len(moms) != 1 or len(epss) != 1 or None in moms:
            raise NotImplementedError("all BatchNorm layers must share one momentum/eps")
        return moms.pop(), epss.pop()

    def forward_features(self, x: torch.Tensor) -> torch.Tensor:
        """[B,1,H,W] -> [B,1024]; the path NetworkWithPointHead uses (it discards the intermediates)."""
        if not x.is_cuda:
            return self._forward_torch(x)[0]
        momentum, eps = self._check(x)
        self._check_width_precision(self.effective_precision())
        x = x.contiguous()
        bn_training = [bn.training for bn in self._bns()]
        if self.training and all(bn_training):
            return _MobileNetFn.apply(x, momentum, eps, self._flat_buffers(), False, self._blur_weights(), self.effective_precision(), self._blocks, self.effective_sequence(), *self._flat_params())
        if any(bn_training):
            raise NotImplementedError("mixed train/eval BatchNorm layers are not supported by the fused backbone")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._flat_params()):
            # every BatchNorm in eval mode, convolutions trainable: fine-tuning with frozen statistics (reference
            # models.py:391-394 + modelcomponents.py:208-215, which also freezes gamma and beta)
            if any(p.requires_grad for bn in self._bns() for p in bn.parameters()):
                raise NotImplementedError("eval-mode BatchNorm layers with trainable weight / bias are not built: freeze them "
                                          "(modelcomponents.freeze_norm_stats) or put the layers in training mode")
            return _MobileNetFn.apply(x, momentum, eps, self._flat_buffers(), True, self._blur_weights(), self.effective_precision(), self._blocks, self.effective_sequence(), *self._flat_params())
        if self.effective_sequence() == "native":
            feat, _ = _native_forward(x, [q.detach() for q in self._flat_params()], self._flat_buffers(), momentum, eps, "eval", self._blur_weights(),
                                      self.effective_precision(), self._blocks)
        elif self.effective_precision() == "bf16-compute":
            feat, _ = _mobilenet_bc.forward_impl(_THIS, x, [q.detach() for q in self._flat_params()], self._flat_buffers(), momentum, eps, False,
                                                 blur=self._blur_weights())
        else:
            feat, _ = _forward_impl(x, [q.detach() for q in self._flat_params()], self._flat_buffers(), momentum, eps, False, blur=self._blur_weights(),
                                    blocks=self._blocks)
        return feat

    def forward(self, x):
        if not x.is_cuda:
            return self._forward_torch(x)
        feat = self.forward_features(x)
        if hasattr(self, "fc"):
            feat = self.fc(self.drop(feat))
        return feat, self._intermediates(x)

    @torch.no_grad()
    def _intermediates(self, x):
        """[z65, z33, z17, z9, z5] post-activation block outputs (reference :165-186), recomputed without
        autograd on request: the pose network never reads them (models.py:343)."""
        momentum, eps = self._check(x)
        bufs = [b.clone() for b in self._flat_buffers()]  # do not double-update running statistics
        training = self.training
        _, c = _forward_impl(x.contiguous(), [q.detach() for q in self._flat_params()], bufs, momentum, eps, training, blur=self._blur_weights(),
                             blocks=self._blocks)
        L, p = _hip.lib(), _hip.ptr
        outs = []
        for k, (name, *_r) in enumerate(self._blocks):
            if name in _INTERMEDIATES:
                st = c.stages[2 * k + 2]
                skip = st.skip
                if st.skip_bn is not None:  # a raw residual operand: materialise relu(bn(skip)) first (an inspection path)
                    skip = torch.empty_like(st.skip)
                    L.call("ttk_bn_act", p(st.skip), p(st.skip_bn), None, p(skip), skip.numel() // skip.shape[-1], skip.shape[-1])
                    skip = _hip.to_blocks(skip)
                a = torch.empty_like(st.y)
                L.call("ttk_bn_act" if _tuned_c(a.shape[-1]) else "ttk_anyc_bn_act", p(st.y), p(st.bn), p(skip), p(a), a.numel() // a.shape[-1], a.shape[-1])
                outs.append(a.permute(0, 3, 1, 2))  # NCHW view of the channels-last copy ttk_bn_act wrote
        return outs

    def _forward_torch(self, x):
        """Plain-torch eval path for CPU tensors (ONNX export / checkpoint inspection).  Training on
        the CPU is not a supported path of this package."""
        if self.training:
            raise RuntimeError("the MI355X training path needs CUDA tensors; CPU tensors are accepted in eval() mode only")
        x = self.relu(self.bn1(self.conv1(x)))
        outs = []
        for name, *_ in self._blocks:
            x = getattr(self, name)(x)
            if name in _INTERMEDIATES:
                outs.append(x)
        x = self.avgpool(x)
        x = x.view(x.size(0), -1)
        if hasattr(self, "fc"):
            x = self.fc(self.drop(x))
        return x, outs

    def prepare_finetune(self):
        return [[*ch.parameters()] for ch in self.children()]
