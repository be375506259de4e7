"""ctypes binding of libttk_hip.so (C-ABI: include/ttk.h).

The header is the one definition of the ABI: the prototypes bound here and the integer constants (TTK) are read from it, not restated.

There is NO fallback: if the shared object is missing or a symbol is absent, importing the kernels
raises; an entry point that returns non-zero raises RuntimeError(ttk_last_error_string()).
"""
from __future__ import annotations

import functools

import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint, c_void_p
from typing import NamedTuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TTK_LIB") or os.path.join(os.path.dirname(_HERE), "libttk_hip.so")  # TTK_LIB: A/B builds
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "ttk.h")

_P, _I, _L, _F, _D = c_void_p, c_int, c_int64, c_float, c_double

# by-value C types of the header; anything with a `*` binds as c_void_p (a `const char*` return as c_char_p)
_CTYPES = {"int": _I, "int64_t": _L, "float": _F, "double": _D, "size_t": c_size_t, "unsigned": c_uint, "ttk_stream_t": _P,
           "ttk_mobilenet_ready_fn": _P}
_C_TYPE_WORDS = set(_CTYPES) | {"void", "char", "short", "long", "signed"}


class Prototype(NamedTuple):
    restype: type
    argtypes: list   # every parameter, the stream included
    stream: bool     # the last parameter is a ttk_stream_t: an entry point that launches (call())


def _ctype(decl: str, fn: str, ret: bool = False):
    """One parameter (`const float* const* w`, `int64_t M`, `float`) or return declaration -> its ctypes class."""
    if "*" in decl:
        return c_char_p if ret and re.sub(r"\s|\bconst\b", "", decl) == "char*" else _P
    words = [w for w in decl.split() if w != "const"]
    if len(words) > 1 and words[-1] not in _C_TYPE_WORDS:
        words.pop()  # the parameter's name
    if " ".join(words) not in _CTYPES:
        raise RuntimeError(f"{fn}: the binding has no ctypes type for `{decl.strip()}` (_hip._CTYPES)")
    return _CTYPES[" ".join(words)]


def parse_header(text: str) -> tuple[dict[str, Prototype], dict[str, int]]:
    """The C ABI as include/ttk.h declares it -> (prototypes by name, integer constants by name without the TTK_ prefix: every
    `#define TTK_X <integer>` and every enumerator).  Relies on the header's style: one prototype per `;`, no parentheses inside a
    parameter list.  A declaration it cannot read raises and names the function; it never skips one."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {m[1]: int(m[2], 0) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+TTK_(\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, re.M)}
    for body in re.findall(r"\benum\s*\w*\s*\{([^}]*)\}", text):
        value = 0
        for item in filter(None, map(str.strip, body.split(","))):
            name, _, explicit = map(str.strip, item.partition("="))
            value = int(explicit, 0) if explicit else value
            consts[name.removeprefix("TTK_")] = value
            value += 1
    protos = {}
    for stmt in re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M).split(";"):
        named = re.search(r"\b(ttk_\w+)\s*\(", stmt)
        if named is None or stmt.split()[0] == "typedef":
            continue
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(ttk_\w+)\s*\(([^()]*)\)\s*", stmt)
        if m is None:
            raise RuntimeError(f"{named[1]}: the binding cannot read this declaration (one prototype per `;`, no nested parentheses)")
        params = [] if m[3].strip() in ("", "void") else m[3].split(",")
        protos[m[2]] = Prototype(_ctype(m[1], m[2], ret=True), [_ctype(p, m[2]) for p in params],
                                 bool(params) and params[-1].split()[0] == "ttk_stream_t")
    return protos, consts


def read_header(path: str):
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: the ctypes binding is derived from the C header of libttk_hip.so (include/ttk.h of the source "
                           "tree). There is no second definition of the ABI to fall back to.")
    with open(path) as f:
        return parse_header(f.read())


# Read once, when this module is imported: the constants size the ctypes structures below.  (TTK_LIB builds are bound by the tree's header
# too; the ABI-version check refuses a library of another version.)
_PROTOTYPES, TTK = read_header(HEADER_PATH)

# name -> argument types of the launching entry points, without the trailing stream (call() appends it)
_SIGNATURES = {name: p.argtypes[:-1] for name, p in _PROTOTYPES.items() if p.stream}

ABI_VERSION = TTK["ABI_VERSION"]
ADAM_HEALTH_SKIPPED, ADAM_HEALTH_CONSECUTIVE, ADAM_HEALTH_CULPRIT, ADAM_HEALTH_WORDS = (
    TTK["ADAM_HEALTH_" + n] for n in ("SKIPPED", "CONSECUTIVE", "CULPRIT", "WORDS"))
MOBILENET_MAX_BLOCKS, MOBILENET_MAX_BUFFERS = TTK["MOBILENET_MAX_BLOCKS"], TTK["MOBILENET_MAX_BUFFERS"]
MOBILENET_MODES = {n: TTK["MOBILENET_" + n.upper()] for n in ("train", "frozen", "eval")}
MOBILENET_PRECISIONS = {"fp32": TTK["MOBILENET_FP32"], "bf16-compute": TTK["MOBILENET_BF16_COMPUTE"]}


class MobileNetPlan(ctypes.Structure):
    """ttk_mobilenet_plan (include/ttk.h): the caller-owned plan of the backbone-level calls ttk_mobilenet_forward / _backward."""
    _fields_ = [(n, c_int) for n in ("B", "H", "W", "c0", "nblocks", "mode", "precision", "deterministic")] + \
               [(n, c_int * MOBILENET_MAX_BLOCKS) for n in ("cin", "cout", "stride", "blur")] + \
               [("check", ctypes.c_uint64), ("nparams", c_int), ("nbuffers", c_int), ("launches", c_int * 2), ("nbuf", c_int * 2),
                ("ws_bytes", ctypes.c_uint64 * 2), ("arena_floats", ctypes.c_uint64),
                ("buf_off", (ctypes.c_uint64 * MOBILENET_MAX_BUFFERS) * 2), ("buf_bytes", (ctypes.c_uint64 * MOBILENET_MAX_BUFFERS) * 2)] + \
               [(n, c_int) for n in ("i_part", "i_bn", "i_prep", "i_y0")] + \
               [(n, c_int * MOBILENET_MAX_BLOCKS) for n in ("i_ain", "i_t", "i_idbn", "i_ydw", "i_ypw")] + \
               [("prep_off", ctypes.c_uint64 * MOBILENET_MAX_BLOCKS), ("prep_bytes", ctypes.c_uint64 * MOBILENET_MAX_BLOCKS), ("i_g", c_int * 2)] + \
               [(n, c_int) for n in ("i_gdw", "i_gt", "i_wg", "i_pw", "i_dwrows", "i_any")]


MOBILENET_READY_FN = ctypes.CFUNCTYPE(None, c_void_p, c_int, c_int)  # ttk_mobilenet_ready_fn


class LossOp(ctypes.Structure):
    """ttk_loss_op (include/ttk.h): one loss op of a ttk_loss_batch launch."""
    _fields_ = [("kind", c_int), ("items", c_int), ("p", c_void_p * 6), ("i", c_int * 4), ("f", c_float * 2), ("d", c_double)]


LOSS_BATCH_MAX = TTK["LOSS_BATCH_MAX"]
# entry point ttk_loss_<name> -> (kind TTK_OP_<NAME>, threads the op needs as a function of its argument tuple); the arguments are
# packed into p[] / i[] / f[] / d in signature order
_n = lambda k: (lambda a: a[k])
LOSS_BATCH_OPS = {"ttk_loss_" + name: (TTK["OP_" + name.upper()], items) for name, items in {
    "rot_fwd": _n(2), "rot_bwd": _n(3), "rot6d_fwd": _n(2), "rot6d_bwd": _n(2),
    "ortho6d_fwd": _n(1), "ortho6d_bwd": _n(2), "quatreg_fwd": _n(1), "quatreg_bwd": _n(2),
    "mse_rows_fwd": lambda a: a[2] * 64, "mse_rows_bwd": lambda a: a[3] * a[4],
    "mse_cols_fwd": lambda a: a[2] * 64, "mse_cols_bwd": lambda a: a[3] * a[4],
    "points_fwd": lambda a: a[2] * 64, "points_bwd": lambda a: a[3] * 204,
    "nllrot_fwd": _n(3), "nllrot_bwd": _n(4), "nllcoord_fwd": _n(3), "nllcoord_bwd": _n(4),
    "normal_fwd": lambda a: a[3] * 64, "normal_bwd": lambda a: a[4] * (204 if a[6] else a[5]),
    "gmm_fwd": lambda a: a[6] * 64, "gmm_bwd": lambda a: a[7] * 50,
}.items()}

# The one hand-written part of the binding: pointer parameters of the ttk_mobilenet_* family that bind TYPED (callers pass a MobileNetPlan,
# int arrays, a callback) instead of as c_void_p.  function -> {parameter index: type}; everything else of these functions is the header's.
_PLAN_P, _INT_P = ctypes.POINTER(MobileNetPlan), ctypes.POINTER(c_int)
_TYPED_POINTERS = {
    "ttk_mobilenet_plan_init": {0: _PLAN_P, 6: _INT_P, 7: _INT_P, 8: _INT_P, 9: _INT_P},
    "ttk_mobilenet_forward_workspace_bytes": {0: _PLAN_P},
    "ttk_mobilenet_backward_workspace_bytes": {0: _PLAN_P},
    "ttk_mobilenet_describe": {0: _PLAN_P, 2: c_char_p, 4: ctypes.POINTER(c_size_t)},
    "ttk_mobilenet_forward": {0: _PLAN_P},
    "ttk_mobilenet_backward": {0: _PLAN_P, 12: MOBILENET_READY_FN},
}


class _Library:
    def __init__(self):
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP kernels are not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
                "neuralnet-tracker-traincode_amd/csrc`). There is no CPU/PyTorch fallback for the training path."
            )
        self.cdll = ctypes.CDLL(LIB_PATH)
        v = self.cdll.ttk_abi_version()
        if v != ABI_VERSION:
            raise RuntimeError(f"libttk_hip.so ABI version {v}, host expects {ABI_VERSION}: rebuild")
        self._fns = {}  # what call() launches: the entry points that end in a stream
        self._stale_reported = False
        for name, typed in _TYPED_POINTERS.items():
            declared = _PROTOTYPES[name].argtypes if name in _PROTOTYPES else []
            if any(i >= len(declared) or declared[i] is not _P for i in typed):
                raise RuntimeError(f"_hip._TYPED_POINTERS[{name!r}] types a parameter that include/ttk.h does not declare as a pointer")
        for name, proto in _PROTOTYPES.items():
            fn = getattr(self.cdll, name)  # AttributeError if the symbol is missing: loud by design
            typed = _TYPED_POINTERS.get(name, {})
            fn.argtypes = [typed.get(i, ty) for i, ty in enumerate(proto.argtypes)]
            fn.restype = proto.restype
            if proto.stream:
                self._fns[name] = fn
        self._clear = self.cdll.ttk_clear_error
        if self.cdll.ttk_mobilenet_plan_bytes() != ctypes.sizeof(MobileNetPlan):
            raise RuntimeError(f"ttk_mobilenet_plan is {self.cdll.ttk_mobilenet_plan_bytes()} bytes in libttk_hip.so, {ctypes.sizeof(MobileNetPlan)} in "
                               "_hip.MobileNetPlan: the two definitions differ")

    def clear_stale_error(self, where: str = "") -> int:
        """Drops (and reports once) a HIP error that an EARLIER, unrelated call of the process left pending - entry points report launch
        failures through the sticky per-thread hipGetLastError().  Called when the library is loaded and once per training / evaluation
        step (train.training_step, eval.Predictor), not before every launch: that was a second ctypes round trip in front of each of the
        ~160 launches of a step (round 3: host_enqueue_ms_per_step 3.2)."""
        stale = self._clear()
        if stale and not self._stale_reported:
            self._stale_reported = True
            import warnings
            warnings.warn(f"a HIP error (hipError_t {stale}) from an earlier launch was pending{' at ' + where if where else ''}; it was dropped, "
                          "not raised", RuntimeWarning, stacklevel=2)
        return stale

    def call(self, name: str, *args):
        # (the raw handle of torch's current stream on the current device: two C calls.  `torch.cuda.current_stream().cuda_stream` builds a Stream
        # object and resolves the device index in Python - 10 us per launch, 1.5 ms of the ~160 launches of a step until round 5)
        rc = self._fns[name](*args, _raw_stream(_cur_device()))
        if rc != 0:
            msg = self.cdll.ttk_last_error_string().decode(errors="replace")
            hint = "" if rc < 0 else " (a positive code is a hipError_t read from the sticky hipGetLastError(): an earlier launch of this step may have left it)"
            raise RuntimeError(f"{name} failed (code {rc}): {msg}{hint}")

    @staticmethod
    def pack_loss_ops(chunk):
        """[(entry point name, argument tuple as for call()), ...] -> ttk_loss_op array: the arguments go to p[] / i[] / f[] / d in signature order."""
        arr = (LossOp * len(chunk))()
        for o, (name, args) in zip(arr, chunk):
            kind, items = LOSS_BATCH_OPS[name]
            o.kind, o.items = kind, int(items(args))
            np_ = ni = nf = 0
            for ty, v in zip(_SIGNATURES[name], args):
                if ty is _P:
                    o.p[np_] = v
                    np_ += 1
                elif ty is _I:
                    o.i[ni] = int(v)
                    ni += 1
                elif ty is _F:
                    o.f[nf] = float(v)
                    nf += 1
                else:
                    o.d = float(v)
        return arr

    def loss_batch(self, ops, tag_sets=None, tag_code=None):
        """ttk_loss_batch: `ops` = [(entry point name, argument tuple as for call()), ...], mutually independent; one launch
        per LOSS_BATCH_MAX ops.  With `tag_code` (int32 device tensor, one Tag code per row) and `tag_sets` (one 32-bit set of Tag
        codes per op): ttk_loss_batch_rows - rows whose code is not in their op's set are dead (value and gradients 0, inputs unread)."""
        if tag_code is not None and (tag_code.dtype != torch.int32 or tag_sets is None or len(tag_sets) != len(ops)):
            raise RuntimeError("loss_batch: tag_code must be an int32 tensor and tag_sets must hold one set per op")
        for lo in range(0, len(ops), LOSS_BATCH_MAX):
            chunk = ops[lo:lo + LOSS_BATCH_MAX]
            arr = self.pack_loss_ops(chunk)
            if tag_code is None:
                self.call("ttk_loss_batch", len(chunk), arr)
            else:
                sets = (ctypes.c_uint * len(chunk))(*[int(m) & 0xFFFFFFFF for m in tag_sets[lo:lo + LOSS_BATCH_MAX]])
                self.call("ttk_loss_batch_rows", len(chunk), arr, sets, ptr(tag_code))

    def _raise(self, name, rc):
        msg = self.cdll.ttk_last_error_string().decode(errors="replace")
        raise RuntimeError(f"{name} failed (code {rc}): {msg}")

    @functools.lru_cache(maxsize=64)
    def mobilenet_plan(self, B, H, W, c0, blocks, blur, mode, precision, deterministic) -> MobileNetPlan:
        """ttk_mobilenet_plan_init: the plan of the backbone-level calls for one shape (cached: plain data, read-only afterwards).  `blocks`:
        ((cin, cout, stride), ...); `blur`: one flag per block; `mode`: "train" | "frozen" | "eval"; `precision`: "fp32" | "bf16-compute".
        A refusal (a channel count outside the kernels' domains, bf16-compute at another width, 32-bit limits) raises ValueError."""
        n = len(blocks)
        if n > MOBILENET_MAX_BLOCKS:
            raise ValueError(f"the backbone-level calls take up to {MOBILENET_MAX_BLOCKS} blocks, got {n}")
        plan = MobileNetPlan()
        IA = c_int * n
        rc = self.cdll.ttk_mobilenet_plan_init(ctypes.byref(plan), B, H, W, c0, n, IA(*[b[0] for b in blocks]), IA(*[b[1] for b in blocks]),
                                               IA(*[b[2] for b in blocks]), IA(*[int(bool(f)) for f in blur]), MOBILENET_MODES[mode],
                                               MOBILENET_PRECISIONS[precision], int(bool(deterministic)))
        if rc != 0:
            raise ValueError(self.cdll.ttk_last_error_string().decode(errors="replace"))
        return plan

    def mobilenet_describe(self, plan: MobileNetPlan, backward: bool) -> list[str]:
        """ttk_mobilenet_describe: the entry points the plan's forward / backward issues, in order."""
        need = ctypes.c_size_t(0)
        if self.cdll.ttk_mobilenet_describe(ctypes.byref(plan), int(backward), None, 0, ctypes.byref(need)) < 0:  # (names == NULL: the size query)
            self._raise("ttk_mobilenet_describe", -1)
        buf = ctypes.create_string_buffer(max(1, need.value))
        n = self.cdll.ttk_mobilenet_describe(ctypes.byref(plan), int(backward), buf, len(buf), None)
        if n < 0:
            self._raise("ttk_mobilenet_describe", n)
        names = buf.value.decode().split("\n") if buf.value else []
        assert len(names) == n, (len(names), n)
        return names

    def mobilenet_forward(self, plan, x, params, buffers, blur, momentum, eps, workspace, feat):
        """ttk_mobilenet_forward on torch's current stream.  `params` / `buffers` / `blur`: ctypes arrays of device pointers (blur: or None)."""
        rc = self.cdll.ttk_mobilenet_forward(ctypes.byref(plan), x.data_ptr(), params, len(params), buffers, len(buffers), blur, momentum, eps,
                                             workspace.data_ptr(), workspace.numel(), feat.data_ptr(), _raw_stream(_cur_device()))
        if rc != 0:
            self._raise("ttk_mobilenet_forward", rc)

    def mobilenet_backward(self, plan, gfeat, x, params, blur, fws, bws, arena, on_ready):
        rc = self.cdll.ttk_mobilenet_backward(ctypes.byref(plan), gfeat.data_ptr(), x.data_ptr(), params, len(params), blur, fws.data_ptr(), fws.numel(),
                                              bws.data_ptr(), bws.numel(), arena.data_ptr(), arena.numel(),
                                              on_ready if on_ready is not None else MOBILENET_READY_FN(), None, _raw_stream(_cur_device()))
        if rc != 0:
            self._raise("ttk_mobilenet_backward", rc)

    def pwconv_prepared_bytes(self, cin: int, cout: int) -> int:
        return self.cdll.ttk_pwconv_prepared_bytes(cin, cout)

    def conv_wgrad_partial_bytes(self, B, H, W, cin, cout, k, stride) -> int:
        """Scratch bytes of ttk_conv_bwd_weight's slice-wise (atomic-free) weight gradient; 0 = the call takes none."""
        return self.cdll.ttk_conv_wgrad_partial_bytes(B, H, W, cin, cout, k, k, stride, k // 2)

    def pwconv_wgrad_partial_bytes(self, m: int, cin: int, cout: int) -> int:
        """Scratch bytes of the deterministic (fixed-order) weight-gradient reduction; 0 = this shape has none."""
        return self.cdll.ttk_pwconv_wgrad_partial_bytes(m, cin, cout)

    @functools.lru_cache(maxsize=None)
    def pwconv_wgrad_scratch_bytes(self, m: int, cin: int, cout: int) -> int:
        """Scratch bytes ttk_pwconv1x1_bwd_weight wants as `partial` in the DEFAULT mode (0: the shape runs its atomic form)."""
        return self.cdll.ttk_pwconv_wgrad_scratch_bytes(m, cin, cout)

    def conv_prepare_weights(self, weights, w_fwd, w_bwd):
        """ttk_conv_prepare_weights: `weights[i]` [Cout, Cin, k, k] fp32, `w_fwd[i]` / `w_bwd[i]` int16 buffers of 3 * numel
        elements (either may be None)."""
        n = len(weights)
        PA, IA = c_void_p * n, c_int * n
        self.call("ttk_conv_prepare_weights", n, PA(*[ptr(w) for w in weights]), PA(*[ptr(t) for t in w_fwd]), PA(*[ptr(t) for t in w_bwd]),
                  IA(*[int(w.shape[0]) for w in weights]), IA(*[int(w.shape[1]) for w in weights]), IA(*[int(w.shape[2]) for w in weights]))

    def pwconv_prepare_weights(self, weights, prepared):
        """One launch: forward and data-gradient weight operands of every pointwise layer (`weights[i]`: [Cout, Cin(,1,1)]
        fp32, `prepared[i]`: uint8 scratch of pwconv_prepared_bytes)."""
        n = len(weights)
        wp = (c_void_p * n)(*[ptr(w) for w in weights])
        pp = (c_void_p * n)(*[ptr(q) for q in prepared])
        ci = (c_int * n)(*[int(w.shape[1]) for w in weights])
        co = (c_int * n)(*[int(w.shape[0]) for w in weights])
        self.call("ttk_pwconv_prepare_weights", n, wp, ci, co, pp)

    def bc_prepare_weights(self, weights, prepared):
        """ttk_bc_prepare_weights: the bf16 weight images (forward + data gradient) of every pointwise layer, one launch."""
        n = len(weights)
        wp = (c_void_p * n)(*[ptr(w) for w in weights])
        pp = (c_void_p * n)(*[ptr(q) for q in prepared])
        ci = (c_int * n)(*[int(w.shape[1]) for w in weights])
        co = (c_int * n)(*[int(w.shape[0]) for w in weights])
        self.call("ttk_bc_prepare_weights", n, wp, ci, co, pp)

    def multi_copy(self, srcs, dsts):
        """dsts[k].copy_(srcs[k]) (None: zero fill) for up to 32 contiguous float32 tensors per launch."""
        for i in range(0, len(dsts), 32):
            s, d = srcs[i:i + 32], dsts[i:i + 32]
            n = len(d)
            for a, b in zip(s, d):
                if b.dtype != torch.float32 or not b.is_contiguous() or (a is not None and (a.dtype != torch.float32 or not a.is_contiguous() or a.numel() != b.numel())):
                    raise RuntimeError("multi_copy: contiguous float32 tensors of matching sizes expected")
            self.call("ttk_multi_copy", n, (c_void_p * n)(*[ptr(a) for a in s]), (c_void_p * n)(*[ptr(b) for b in d]),
                      (c_int64 * n)(*[b.numel() for b in d]))

    @functools.lru_cache(maxsize=None)
    def anyc_partial_rows(self, pixels: int) -> int:
        """Rows of partial sums the pixel-wise kernels of the any-channel-count family write for `pixels` pixels."""
        return self.cdll.ttk_anyc_partial_rows(pixels)

    @functools.lru_cache(maxsize=None)
    def anyc_wgrad_scratch_bytes(self, kind: str, *shape) -> int:
        """Scratch bytes of a weight gradient of the any-channel-count family: kind "stem" (B, H, W, Cout), "dw" (B, H, W, C), "pw" (M, Cin, Cout)."""
        return getattr(self.cdll, f"ttk_anyc_{kind}_wgrad_scratch_bytes")(*shape)

    # (pure functions of their integer arguments, asked ~80 times per step: cached)
    @functools.lru_cache(maxsize=None)
    def partial_rows_elementwise(self, items: int) -> int:
        return self.cdll.ttk_partial_rows_elementwise(items)

    @functools.lru_cache(maxsize=None)
    def partial_rows_dwconv(self, B, H, W, C, stride, backward) -> int:
        return self.cdll.ttk_partial_rows_dwconv(B, H, W, C, stride, int(backward))

    @functools.lru_cache(maxsize=None)
    def partial_rows_gemm(self, m: int, k: int | None = None, nout: int | None = None, dgrad: bool = False) -> int:
        """Rows of BatchNorm partial sums a GEMM epilogue writes for m rows.  With (k, nout): of ttk_pwconv1x1_fwd (k = Cin, nout = Cout) /
        ttk_pwconv1x1_bwd_data (k = Cout, nout = Cin, dgrad=True), whose tiling depends on the shape; without: the 128-row form (convolutions)."""
        if k is None:
            return self.cdll.ttk_partial_rows_gemm(m)
        return self.cdll.ttk_partial_rows_pwconv(m, k, nout, int(dgrad))


# hipGraph captures run in "global" error mode: a HIP call that another thread makes while a capture is open (an allocation, a copy on
# another stream) invalidates it.  Whoever captures holds this lock (train.GraphedTrainStep); background threads that touch the GPU
# (datasets.resident's host-frame prefetch) take it around their GPU work.
import threading

CAPTURE_LOCK = threading.RLock()

_lib: _Library | None = None


_raw_stream = torch._C._cuda_getCurrentRawStream
_cur_device = torch._C._cuda_getDevice


def lib() -> _Library:
    global _lib
    if _lib is None:
        _lib = _Library()
        if torch.cuda.is_available():
            _lib.clear_stale_error("library load")
    return _lib


def ptr(t: torch.Tensor | None):
    """Device pointer of a contiguous CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("HIP entry point received a non-CUDA tensor")
    if not t.is_contiguous():
        raise RuntimeError("HIP entry point received a non-contiguous tensor")
    return t.data_ptr()


def check_tensors(ts, what="tensor"):
    """The checks of ptr() for a list of tensors at once (the backbones validate their parameters and inputs ONCE per call and then
    take the addresses of those and of the tensors they allocate themselves with fast_ptr)."""
    for t in ts:
        if t is not None and not (t.is_cuda and t.is_contiguous()):
            raise RuntimeError(f"HIP entry point received a non-CUDA or non-contiguous {what}")


def fast_ptr(t: torch.Tensor | None):
    """Device pointer without ptr()'s checks: for tensors the caller allocated itself or has run through check_tensors."""
    return None if t is None else t.data_ptr()


CHANNEL_BLOCK = 32  # kCB of csrc/ttk_common.h


def to_blocks(t: torch.Tensor) -> torch.Tensor:
    """Channels-last values [..., C] -> the storage order of the MobileNet kernels' activation tensors (include/ttk.h, "Activation
    layout": channel blocks [C/32][pixels][32]).  The result keeps the nominal shape of `t`; only its memory order differs.  Host code
    never needs this - activations are produced and consumed by kernels - tests and tools do."""
    C = t.shape[-1]
    if C <= CHANNEL_BLOCK:
        return t.contiguous()
    return t.reshape(-1, C // CHANNEL_BLOCK, CHANNEL_BLOCK).transpose(0, 1).contiguous().view(t.shape)


def to_blocks_any(t: torch.Tensor) -> torch.Tensor:
    """`to_blocks` for any channel count (include/ttk.h, "Activation layout"): blocks of 32 and one narrower last block,
    [M][32], ..., [M][32], [M][C mod 32].  Equal to `to_blocks` for C a multiple of 32; plain rows for C < 32."""
    C = t.shape[-1]
    if C % CHANNEL_BLOCK == 0:
        return to_blocks(t)
    full = C // CHANNEL_BLOCK * CHANNEL_BLOCK
    rows = t.reshape(-1, C)
    parts = [to_blocks(rows[:, :full]).reshape(-1)] if full else []
    return torch.cat(parts + [rows[:, full:].reshape(-1)]).view(t.shape)


def from_blocks_any(t: torch.Tensor) -> torch.Tensor:
    """Inverse of `to_blocks_any`."""
    C = t.shape[-1]
    if C % CHANNEL_BLOCK == 0:
        return from_blocks(t)
    full = C // CHANNEL_BLOCK * CHANNEL_BLOCK
    flat = t.reshape(-1)
    M = flat.numel() // C
    tail = flat[M * full:].view(M, C - full)
    if not full:
        return tail.reshape(t.shape)
    return torch.cat([from_blocks(flat[:M * full].view(M, full)), tail], dim=1).reshape(t.shape)


def from_blocks(t: torch.Tensor) -> torch.Tensor:
    """Inverse of `to_blocks`: a tensor whose memory holds channel blocks -> the channels-last values, same nominal shape."""
    C = t.shape[-1]
    if C <= CHANNEL_BLOCK:
        return t
    return t.reshape(C // CHANNEL_BLOCK, -1, CHANNEL_BLOCK).transpose(0, 1).reshape(t.shape)


CHANNEL_BLOCK_BC = 64  # bf16-compute path (csrc/bc_common.h)


def to_blocks64(t: torch.Tensor) -> torch.Tensor:
    """Channels-last values [..., C] -> the bf16-compute path's storage order (channel blocks [C/64][pixels][64]); tests and tools only."""
    C = t.shape[-1]
    if C <= CHANNEL_BLOCK_BC:
        return t.contiguous()
    return t.reshape(-1, C // CHANNEL_BLOCK_BC, CHANNEL_BLOCK_BC).transpose(0, 1).contiguous().view(t.shape)


def from_blocks64(t: torch.Tensor) -> torch.Tensor:
    C = t.shape[-1]
    if C <= CHANNEL_BLOCK_BC:
        return t
    return t.reshape(C // CHANNEL_BLOCK_BC, -1, CHANNEL_BLOCK_BC).transpose(0, 1).reshape(t.shape)


def exported_symbols() -> list[str]:
    return list(_PROTOTYPES)
