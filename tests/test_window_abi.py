"""achip_window_* without a GPU: the four symbols exported and typed, the argument checks that come before any context is touched, the constants of the Python
binding, and HipBatchCodec's methods reaching the library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("achip_window_decompress_batch", "achip_window_compress_batch", "achip_window_decompress", "achip_window_compress")
DECODE_OPS, ENCODE_OPS = (8, 10, 12), (9, 11, 13)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library()
    import aircompressor_amd as A
    return A.load_library()


def test_symbols_exported_and_typed(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "aircompressor_amd", "libaircompressor_hip.so")], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (achip_[a-z0-9_]+)", out))
    from aircompressor_amd import native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aircompressor_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert name in exported, name
        restype, argtypes = native.SIGNATURES[name]
        decl = re.search(r"int32_t\s+%s\(([^;]*)\);" % name, header).group(1)
        params = [p.strip() for p in decl.split(",")]
        assert restype is ctypes.c_int32 and len(argtypes) == len(params), name
        for p, t in zip(params, argtypes):  # pointer <-> pointer, int32 <-> int32
            pointer = "*" in p
            assert pointer == (t is ctypes.c_void_p or hasattr(t, "contents")), (name, p, t)
            assert pointer or t is ctypes.c_int32, (name, p, t)
    assert len(re.search(r"achip_window_decompress_batch\(([^;]*)\);", header).group(1).split(",")) == 16
    assert len(re.search(r"achip_window_decompress\(([^;]*)\);", header).group(1).split(",")) == 12


def test_constants():
    from aircompressor_amd import native
    header = open(os.path.join(ROOT, "include", "aircompressor_hip.h")).read()
    for name, value in (("WINDOW_FIRST", 1), ("WINDOW_LAST", 2), ("STOP_END", 0), ("STOP_NEED_INPUT", 1), ("STOP_NEED_ROOM", 2), ("STOP_FAILED", 3)):
        assert getattr(native, name) == value
        assert re.search(r"#define ACHIP_%s\s+%d\b" % (name, value), header), name


def test_argument_checks_without_a_device(lib):
    """wrong op, null arrays with nBlocks > 0, nBlocks == 0: decided before the context is looked at (ctx is NULL throughout)"""
    z = np.zeros(8, dtype=np.int64)
    p = z.ctypes.data
    arrays = [p] * 10
    for fn, good, bad in ((lib.achip_window_decompress_batch, DECODE_OPS, ENCODE_OPS + (0, 4, 6, 14, -1, 15)), (lib.achip_window_compress_batch, ENCODE_OPS, DECODE_OPS + (1, 5, 7, 14, -1, 15))):
        for op in bad:
            assert lib.achip_status_class(fn(None, op, *arrays, 1, p, p, p)) == 3, op
            assert b"codecOp" in lib.achip_last_error()
            assert lib.achip_status_class(fn(None, op, *arrays, 0, p, p, p)) == 3, op  # (the op is checked first)
        for op in good:
            assert fn(None, op, *([None] * 10), 0, None, None, None) == 0             # nothing to do: nothing launched, nothing looked at
            assert lib.achip_status_class(fn(None, op, *arrays, -1, p, p, p)) == 3
            for missing in (0, 2, 3, 5, 6, 7, 8, 9):                                     # flags, srcOff, srcLen, dstOff, dstCap, outLen, status, errOffset
                a = list(arrays)
                a[missing] = None
                assert lib.achip_status_class(fn(None, op, *a, 1, p, p, p)) == 3, (op, missing)
                assert b"null array" in lib.achip_last_error()
            for missing in range(3):                                                     # consumed, stop, need
                tail = [p, p, p]
                tail[missing] = None
                assert lib.achip_status_class(fn(None, op, *arrays, 1, *tail)) == 3, (op, missing)
            r = fn(None, op, *arrays, 1, p, p, p)
            assert lib.achip_status_class(r) == 3 and b"ctx is null" in lib.achip_last_error()
    out = [ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()]
    refs = [ctypes.byref(x) for x in out]
    buf = np.zeros(64, dtype=np.uint8)
    for fn, good, bad in ((lib.achip_window_decompress, DECODE_OPS, ENCODE_OPS + (0, 14)), (lib.achip_window_compress, ENCODE_OPS, DECODE_OPS + (1, 14))):
        for op in bad:
            assert lib.achip_status_class(fn(None, op, 3, buf.ctypes.data, 8, buf.ctypes.data, 8, *refs)) == 3 and b"codecOp" in lib.achip_last_error()
        for op in good:
            assert lib.achip_status_class(fn(None, op, 3, buf.ctypes.data, -1, buf.ctypes.data, 8, *refs)) == 3 and b"negative" in lib.achip_last_error()
            assert lib.achip_status_class(fn(None, op, 4, buf.ctypes.data, 8, buf.ctypes.data, 8, *refs)) == 3 and b"flag" in lib.achip_last_error()
            assert lib.achip_status_class(fn(None, op, 3, None, 8, buf.ctypes.data, 8, *refs)) == 3 and b"null buffer" in lib.achip_last_error()
            assert lib.achip_status_class(fn(None, op, 3, buf.ctypes.data, 8, buf.ctypes.data, 8, *(refs[:2] + [None] + refs[3:]))) == 3
            assert lib.achip_status_class(fn(None, op, 3, buf.ctypes.data, 8, buf.ctypes.data, 8, *refs)) == 3 and b"ctx is null" in lib.achip_last_error()


def test_batch_codec_methods_reach_the_library(lib):
    """HipBatchCodec.window_decompress / window_compress / window_host hand their arguments to the four entry points: through a codec over a NULL context the
    library's own argument checks answer"""
    import aircompressor_amd as A

    class NoContext:
        ctx = None

        def __init__(self, lib):
            self.lib = lib

    codec = A.HipBatchCodec(native_ctx=NoContext(lib))
    z = np.zeros(8, dtype=np.int64)
    p = z.ctypes.data
    for method, good, bad in ((codec.window_decompress, A.OP_LZ4HADOOP_DECOMPRESS, A.OP_LZ4HADOOP_COMPRESS), (codec.window_compress, A.OP_SNAPPYFRAMED_COMPRESS, A.OP_ZSTD_COMPRESS)):
        method(good, None, None, None, None, None, None, None, None, None, None, 0, None, None, None)  # nBlocks == 0: returns
        with pytest.raises(A.IllegalArgumentException):
            method(bad, p, p, p, p, p, p, p, p, p, p, 1, p, p, p)
        with pytest.raises(A.IllegalArgumentException):
            method(good, p, p, p, p, p, p, p, p, p, p, 1, p, p, p)  # (ctx is null)
        assert b"ctx is null" in lib.achip_last_error()
    for compress, op in ((False, A.OP_SNAPPYHADOOP_DECOMPRESS), (True, A.OP_SNAPPYHADOOP_COMPRESS)):
        with pytest.raises(A.IllegalArgumentException):
            codec.window_host(op, A.native.WINDOW_FIRST, b"12345678", 64, compress=compress)
        assert b"ctx is null" in lib.achip_last_error()
        with pytest.raises(A.IllegalArgumentException):
            codec.window_host(op ^ 1, 0, b"12345678", 64, compress=compress)
    for name in ("HipWindowInputStream", "HipWindowOutputStream", "SnappyFramedHipInputStream", "SnappyFramedHipOutputStream", "Lz4HadoopHipInputStream", "Lz4HadoopHipOutputStream",
                 "SnappyHadoopHipInputStream", "SnappyHadoopHipOutputStream"):
        assert all(hasattr(getattr(A, name), m) for m in (("read", "readall", "close") if "Input" in name else ("write", "finish", "close"))), name
