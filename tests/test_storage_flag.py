"""The storage argument of the fp32 kernel family (include/ttk.h, `act_bf16`): the depthwise, pointwise and pooling entry points take float32
tensors only.  They keep the argument for ABI stability, and either storage bit is refused WITH THE ARGUMENT CHECKS - before any launch, memset
or tiling query - naming the bf16-compute path.  No GPU is needed: the checks run first, so the (host) pointers are never dereferenced and a
refused call makes no HIP call; a call that got as far as a launch on a host without a GPU would return a positive HIP error instead of -1."""
import ctypes
import os
import re

import pytest

from util import PKG, REPO

P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64

# name -> (argument types, arguments): a small valid shape; "p" = a non-null pointer, None = NULL; the storage flag is the argument
# before the stream
CASES = {
    "ttk_dwconv3x3_fwd": ([P] * 8 + [I] * 6 + [P],  # yprev, bn_prev, skip_prev, a_out, w, y, part, pivot, B, H, W, C, stride
                          ["p", "p", None, None, "p", "p", "p", None, 2, 5, 5, 32, 1]),
    "ttk_dwconv3x3_bwd_data": ([P] * 12 + [I] + [P] + [I] * 6 + [P],  # ..., g_prev, part, dw = NULL, dw_accumulate, dw_partial, B, H, W, C, stride
                               ["p", "p", "p", "p", None, "p", "p", None, None, "p", "p", None, 0, None, 2, 5, 5, 32, 1]),
    "ttk_pwconv1x1_fwd": ([P] * 6 + [L, I, I, P, I, P],  # ydw, bn_dw, w, y, part, pivot, M, Cin, Cout, wsplit
                          ["p", "p", "p", "p", "p", None, 50, 32, 64, None]),
    "ttk_pwconv1x1_bwd_data": ([P] * 8 + [L, I, I, P, I, P],  # g, y, bn_pw, wt, ydw, bn_dw, g_dw, part, M, Cin, Cout, wsplit
                               ["p", "p", "p", "p", "p", "p", "p", "p", 50, 32, 64, None]),
    "ttk_pwconv1x1_bwd_weight": ([P] * 7 + [L, I, I, I, P],  # g, y, bn_pw, ydw, bn_dw, dw, partial, M, Cin, Cout
                                 ["p", "p", "p", "p", "p", "p", None, 50, 32, 64]),
    "ttk_avgpool_fwd": ([P] * 4 + [I] * 4 + [P], ["p", "p", None, "p", 2, 25, 32]),  # y, bn, skip, feat, B, HW, C
    "ttk_avgpool_bwd": ([P] * 6 + [I] * 4 + [P], ["p", "p", "p", None, "p", "p", 2, 25, 32]),  # gfeat, y, bn, skip, g, part, B, HW, C
}
STEM_PAIR = {"ttk_stem_fwd", "ttk_stem_bwd_weight"}  # fp32 or both bits: also serves the bf16-compute path


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(PKG, "libttk_hip.so")
    assert os.path.exists(path), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(path)
    lib.ttk_last_error_string.restype = ctypes.c_char_p
    return lib


def _declarations():
    header = open(os.path.join(REPO, "include", "ttk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    return {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(ttk_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header)}


def test_cases_are_every_fp32_only_entry_point_with_a_storage_flag():
    with_flag = {name for name, params in _declarations().items() if "act_bf16" in params}
    assert with_flag - STEM_PAIR == set(CASES) and STEM_PAIR <= with_flag


@pytest.mark.parametrize("name", sorted(CASES))
def test_declaration_keeps_the_storage_flag_before_the_stream(name):
    params = _declarations()[name]
    assert params.endswith("int act_bf16, ttk_stream_t stream"), params


@pytest.mark.parametrize("flag", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_storage_bits_are_refused_before_any_launch(lib, name, flag):
    argtypes, args = CASES[name]
    assert len(argtypes) == len(args) + 2
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = argtypes, ctypes.c_int
    host = (ctypes.c_float * 16)()  # never read or written: the refusal comes first
    ptr = ctypes.cast(host, ctypes.c_void_p)
    rc = fn(*[ptr if a == "p" else a for a in args], flag, None)
    assert rc < 0, f"{name}(act_bf16={flag}) returned {rc}"
    msg = lib.ttk_last_error_string().decode()
    assert "bf16-compute" in msg and name[len("ttk_"):] in msg, msg
    assert all(v == 0.0 for v in host)
