"""The ctypes binding is derived from include/ttk.h (trackertraincode/_hip.py: parse_header): the reader on small synthetic headers, then
the real header against the built library, with the argument widths pinned where a wrong type would corrupt arguments silently."""
import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint, c_void_p

import pytest

import trackertraincode._hip as H
from util import REPO

HEADER = open(os.path.join(REPO, "include", "ttk.h")).read()
NO_COMMENTS = re.sub(r"/\*.*?\*/|//[^\n]*", " ", HEADER, flags=re.S)


def test_reader_on_synthetic_prototypes():
    protos, consts = H.parse_header("""
        #ifndef X_H_
        #define X_H_
        typedef void* ttk_stream_t;
        typedef void (*ttk_mobilenet_ready_fn)(void* user, int a, int b);
        /* ttk_in_block_comment(int a, ttk_stream_t stream); is prose,
           int ttk_on_its_own_line(int a); too */
        // int ttk_in_line_comment(int a);
        int ttk_multi_line(const float* x, float* const y,
                           int64_t M,   /* rows; not ttk_rows(M) */
                           unsigned flags, double tol,
                           ttk_stream_t stream);
        int ttk_pointer_table(int n, const float* const* w, void* const* prepared, const int* cin, float scale, ttk_stream_t stream);
        int ttk_no_args(void);
        size_t ttk_scratch_bytes(int64_t M, int C);
        const char* ttk_text(void);
        int ttk_callback(ttk_mobilenet_ready_fn on_ready, void* user, size_t n);
        int ttk_unnamed(int, const float*, float, ttk_stream_t);
        #endif
    """)
    assert list(protos) == ["ttk_multi_line", "ttk_pointer_table", "ttk_no_args", "ttk_scratch_bytes", "ttk_text", "ttk_callback", "ttk_unnamed"]
    assert protos["ttk_multi_line"] == (c_int, [c_void_p, c_void_p, c_int64, c_uint, c_double, c_void_p], True)
    assert protos["ttk_pointer_table"] == (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p], True)
    assert protos["ttk_no_args"] == (c_int, [], False)
    assert protos["ttk_scratch_bytes"] == (c_size_t, [c_int64, c_int], False)
    assert protos["ttk_text"] == (c_char_p, [], False)
    assert protos["ttk_callback"] == (c_int, [c_void_p, c_void_p, c_size_t], False)
    assert protos["ttk_unnamed"] == (c_int, [c_int, c_void_p, c_float, c_void_p], True)
    assert consts == {}  # (X_H_ has no value and no TTK_ prefix)


def test_reader_on_synthetic_constants():
    _, consts = H.parse_header("""
        #define TTK_ABI_VERSION 7
        #define TTK_MASK 0x10   /* a comment behind the value */
        #define TTK_NOT_AN_INTEGER (1 << 3)
        #define OTHER_PREFIX 5
        // #define TTK_IN_COMMENT 9
        enum { TTK_A, TTK_B, TTK_C = 5, /* TTK_GHOST = 6, */ TTK_D,
               TTK_E = 2, TTK_F };
        enum ttk_named { TTK_ONE = 1 };
    """)
    assert consts == {"ABI_VERSION": 7, "MASK": 16, "A": 0, "B": 1, "C": 5, "D": 6, "E": 2, "F": 3, "ONE": 1}


@pytest.mark.parametrize("decl,named", [
    ("int ttk_long_double(long double x, ttk_stream_t stream);", "ttk_long_double"),       # a by-value type outside the vocabulary
    ("int ttk_by_value_struct(ttk_mobilenet_plan plan);", "ttk_by_value_struct"),
    ("int ttk_uchar(unsigned char c);", "ttk_uchar"),                                      # not silently bound as `unsigned`
    ("int ttk_ok(int a);\nuint64_t ttk_returns_u64(int a);", "ttk_returns_u64"),           # ... in a return type
    ("int ttk_inline_fn_pointer(void (*cb)(int), int n);", "ttk_inline_fn_pointer"),       # a declaration outside the header's style
])
def test_reader_raises_and_names_the_function(decl, named):
    with pytest.raises(RuntimeError, match=named):
        H.parse_header(decl)


def test_missing_header_raises(tmp_path):
    with pytest.raises(RuntimeError, match=r"ttk\.h not found"):
        H.read_header(str(tmp_path / "ttk.h"))


def test_every_declared_function_is_derived_and_resolves():
    declared = set(re.findall(r"\b(ttk_[a-z0-9_]+)\s*\(", NO_COMMENTS))
    assert len(declared) > 140
    assert set(H._PROTOTYPES) == declared == set(H.exported_symbols())  # nothing is skipped
    cdll = H.lib().cdll
    for name, proto in H._PROTOTYPES.items():
        fn = getattr(cdll, name)
        assert fn.restype is proto.restype and len(fn.argtypes) == len(proto.argtypes), name
        typed = H._TYPED_POINTERS.get(name, {})
        assert all(a is b for i, (a, b) in enumerate(zip(fn.argtypes, proto.argtypes)) if i not in typed), name
    # call() launches exactly the functions that end in a stream; _SIGNATURES is their argument list without it
    streamed = {n for n in declared if re.search(r"\b" + n + r"\s*\([^;]*\bttk_stream_t\s+stream\s*\)\s*;", NO_COMMENTS)}
    assert set(H.lib()._fns) == set(H._SIGNATURES) == streamed and len(streamed) > 100
    assert all(H._SIGNATURES[n] == H._PROTOTYPES[n].argtypes[:-1] for n in streamed)


def _param(fn, name):
    """(index, declaration text) of parameter `name` of `fn`, from the header text."""
    params = re.search(r"\b" + fn + r"\s*\(([^;]*)\)\s*;", NO_COMMENTS).group(1).split(",")
    (i,) = [k for k, p in enumerate(params) if p.split()[-1].lstrip("*") == name]
    return i, " ".join(params[i].split())


@pytest.mark.parametrize("fn,param,text,ctype", [
    ("ttk_bn_fwd_finalize", "count", "int64_t count", c_int64),
    ("ttk_bn_fwd_finalize", "momentum", "float momentum", c_float),
    ("ttk_bn_fwd_finalize", "eps", "float eps", c_float),
    ("ttk_pwconv1x1_fwd", "M", "int64_t M", c_int64),
    ("ttk_loss_gmm_fwd", "fudge", "double fudge", c_double),
    ("ttk_mobilenet_forward", "workspace_bytes", "size_t workspace_bytes", c_size_t),
])
def test_widths_where_a_wrong_type_corrupts_silently(fn, param, text, ctype):
    i, decl = _param(fn, param)
    assert decl == text  # what the header says ...
    assert getattr(H.lib().cdll, fn).argtypes[i] is ctype  # ... is what is bound


def test_return_types_of_the_queries():
    cdll = H.lib().cdll
    queries = [n for n in H._PROTOTYPES if n.endswith("_bytes")]
    assert len(queries) >= 15
    for name in queries:
        assert re.search(r"\bsize_t\s+" + name + r"\s*\(", NO_COMMENTS), name
        assert getattr(cdll, name).restype is c_size_t, name
    assert re.search(r"\bconst char\*\s*ttk_last_error_string\s*\(void\)", NO_COMMENTS)
    assert cdll.ttk_last_error_string.restype is c_char_p and cdll.ttk_last_error_string.argtypes == []


def test_typed_pointers_of_the_mobilenet_family():
    """The hand-written part: a MobileNetPlan instance, int arrays and the callback bind typed; every position is a pointer in the header."""
    cdll = H.lib().cdll
    assert set(H._TYPED_POINTERS) == {n for n in H._PROTOTYPES if n.startswith("ttk_mobilenet_")} - {"ttk_mobilenet_plan_bytes"}
    for name, typed in H._TYPED_POINTERS.items():
        for i, ty in typed.items():
            assert H._PROTOTYPES[name].argtypes[i] is c_void_p and getattr(cdll, name).argtypes[i] is ty, (name, i)
    assert cdll.ttk_mobilenet_plan_init.argtypes[0] is ctypes.POINTER(H.MobileNetPlan)
    assert cdll.ttk_mobilenet_backward.argtypes[_param("ttk_mobilenet_backward", "on_ready")[0]] is H.MOBILENET_READY_FN
    assert cdll.ttk_mobilenet_forward_workspace_bytes(H.MobileNetPlan()) == 0  # an instance passes by reference; a zeroed plan is not valid


def test_constants_come_from_the_header():
    lib = H.lib()
    assert H.TTK["ABI_VERSION"] == lib.cdll.ttk_abi_version() == H.ABI_VERSION
    assert sorted(kind for kind, _ in H.LOSS_BATCH_OPS.values()) == list(range(H.TTK["OP_COUNT"]))
    assert all(H.TTK["OP_" + name[len("ttk_loss_"):].upper()] == kind for name, (kind, _) in H.LOSS_BATCH_OPS.items())
    assert ctypes.sizeof(H.MobileNetPlan) == lib.cdll.ttk_mobilenet_plan_bytes()
    assert (H.TTK["BN_ROWS"], H.TTK["BN_SCALE"], H.TTK["BN_RSTD"], H.TTK["BN_AUX"]) == (8, 0, 3, 7)
    assert (H.ADAM_HEALTH_SKIPPED, H.ADAM_HEALTH_CONSECUTIVE, H.ADAM_HEALTH_CULPRIT, H.ADAM_HEALTH_WORDS) == (0, 1, 2, 4)
    assert H.MOBILENET_MODES == {"train": 0, "frozen": 1, "eval": 2} and H.MOBILENET_PRECISIONS == {"fp32": 0, "bf16-compute": 1}
    assert (H.MOBILENET_MAX_BLOCKS, H.MOBILENET_MAX_BUFFERS, H.LOSS_BATCH_MAX) == (16, 96, 32)
    from trackertraincode.backbones import _mobilenet_bc, mobilenet_v1, resnet
    assert mobilenet_v1._BN_ROWS == resnet._BN_ROWS == 8 and _mobilenet_bc._BF == 3 and mobilenet_v1._FP32_STORAGE == 0
