"""achip_decoded_size_batch / achip_plan_outputs without a device: both symbols are exported and typed, and the checks of the value arguments come before
anything touches a context, so a caller's mistake reads the same on a machine without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 3
DECODE_OPS = (0, 2, 4, 6, 8, 10, 12)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library()
    import aircompressor_amd as A
    return A.load_library()


def test_both_symbols_are_exported_and_typed(lib):
    from aircompressor_amd import native
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIBRARY_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (achip_[a-z0-9_]+)", out))
    i32, i64p, vp = ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p
    assert "achip_decoded_size_batch" in exported and "achip_plan_outputs" in exported
    assert native.SIGNATURES["achip_decoded_size_batch"] == (i32, [vp, i32, vp, vp, vp, i64p, vp, vp, i32])
    assert native.SIGNATURES["achip_plan_outputs"] == (i32, [vp, vp, vp, i32, i32, vp, vp, vp])
    header = open(os.path.join(ROOT, "include", "aircompressor_hip.h")).read()
    assert re.search(r"int32_t achip_decoded_size_batch\(achip_ctx\* ctx, int32_t codecOp, const void\* srcBase, const int64_t\* srcOff, const int32_t\* srcLen,\s*"
                     r"int64_t\* outSize, int32_t\* status, int64_t\* errOffset, int32_t nBlocks\);", header)
    assert re.search(r"int32_t achip_plan_outputs\(achip_ctx\* ctx, const int64_t\* outSize, const int32_t\* status, int32_t nBlocks, int32_t align,\s*"
                     r"int64_t\* dstOff, int32_t\* dstCap, int64_t\* total", header)


def test_argument_checks_need_no_device(lib):
    a = np.zeros(4, dtype=np.int64)
    p = a.ctypes.data
    for op in (1, 3, 5, 7, 9, 11, 13, 14, -1, 15):  # compress ops, and no op at all
        assert lib.achip_status_class(lib.achip_decoded_size_batch(None, op, p, p, p, p, p, p, 1)) == INVALID_ARGUMENT, op
    for op in DECODE_OPS:
        assert lib.achip_status_class(lib.achip_decoded_size_batch(None, op, p, p, p, p, p, p, -1)) == INVALID_ARGUMENT
        assert lib.achip_decoded_size_batch(None, op, p, p, p, p, p, p, 0) == 0
        assert lib.achip_status_class(lib.achip_decoded_size_batch(None, op, p, p, p, p, p, p, 1)) == INVALID_ARGUMENT  # (no context)
    for align in (0, 3, 8192, -16, 24):
        assert lib.achip_status_class(lib.achip_plan_outputs(None, p, p, 0, align, p, p, p)) == INVALID_ARGUMENT, align
    assert b"align" in lib.achip_last_error()
    for align in (1, 2, 16, 4096):
        assert lib.achip_plan_outputs(None, p, p, 0, align, p, p, p) == 0
        assert lib.achip_status_class(lib.achip_plan_outputs(None, p, p, -1, align, p, p, p)) == INVALID_ARGUMENT
        assert lib.achip_status_class(lib.achip_plan_outputs(None, p, p, 1, align, p, p, p)) == INVALID_ARGUMENT  # (no context)


def test_batch_codec_methods_reach_the_library(lib):
    """HipBatchCodec's thin methods without a device: an empty batch goes through the binding (argument count and carriers) and launches nothing; a bad
    argument comes back as the exception the other batch calls raise"""
    import types
    import aircompressor_amd as A
    for name in ("decoded_sizes", "plan_outputs", "decompress_unsized"):
        assert callable(getattr(A.HipBatchCodec, name))
    codec = object.__new__(A.HipBatchCodec)  # (no context: the constructor wants a GPU)
    codec.lib = lib
    codec.native = types.SimpleNamespace(ctx=None)
    a = np.zeros(4, dtype=np.int64)
    p = a.ctypes.data
    codec.decoded_sizes(A.OP_ZSTD_DECOMPRESS, p, p, p, p, p, p, 0)
    codec.plan_outputs(p, p, 0, 16, p, p, p)
    with pytest.raises(A.IllegalArgumentException):
        codec.decoded_sizes(A.OP_ZSTD_COMPRESS, p, p, p, p, p, p, 0)
    with pytest.raises(A.IllegalArgumentException):
        codec.plan_outputs(p, p, 0, 24, p, p, p)
