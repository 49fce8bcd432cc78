"""achip_compress_bound_batch / achip_pack_outputs without a device: both symbols are exported, typed and declared, and the checks of the value arguments come
before anything touches a context, so a caller's mistake reads the same on a machine without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 3
COMPRESS_OPS = (1, 3, 5, 7, 9, 11, 13, 14)


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
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert "achip_compress_bound_batch" in exported and "achip_pack_outputs" in exported
    assert native.SIGNATURES["achip_compress_bound_batch"] == (i32, [vp, i32, vp, vp, vp, i32])
    assert native.SIGNATURES["achip_pack_outputs"] == (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, i64, vp, vp, vp, vp])
    header = open(os.path.join(ROOT, "include", "aircompressor_hip.h")).read()
    assert re.search(r"int32_t achip_compress_bound_batch\(achip_ctx\* ctx, int32_t codecOp, const int32_t\* srcLen,\s*int64_t\* outSize, int32_t\* status, int32_t nBlocks\);", header)
    assert re.search(r"int32_t achip_pack_outputs\(achip_ctx\* ctx, const void\* srcBase, const int64_t\* srcOff, const int32_t\* outLen, const int32_t\* status,\s*"
                     r"const void\* rawBase, const int64_t\* rawOff, const int32_t\* rawLen,[^;]*?"
                     r"int32_t nBlocks, int32_t align, void\* packedBase, int64_t packedCap,\s*"
                     r"int64_t\* packedOff, int32_t\* packedLen, int32_t\* stored[^;]*?, int64_t\* total[^;]*\);", header)
    # each declaration cites the reference interface it stands in for
    section = header[header.index("achip_compress_bound_batch:"):header.index("int32_t achip_pack_outputs(")]
    assert "Compressor.maxCompressedLength" in section and "M/Compressor.java" in section and "OutputStream.java" in section


def test_argument_checks_need_no_device(lib):
    a = np.zeros(4, dtype=np.int64)
    p = a.ctypes.data
    cls = lib.achip_status_class

    def pack(n=0, align=1, raw=(None, None, None), stored=None, base=p, cap=16):
        return lib.achip_pack_outputs(None, p, p, p, p, raw[0], raw[1], raw[2], n, align, base, cap, p, p, stored, p)

    for op in (0, 2, 4, 6, 8, 10, 12, -1, 15):  # decode ops, and no op at all
        assert cls(lib.achip_compress_bound_batch(None, op, p, p, p, 1)) == INVALID_ARGUMENT, op
        assert cls(lib.achip_compress_bound_batch(None, op, p, p, p, 0)) == INVALID_ARGUMENT, op
    for op in COMPRESS_OPS:
        assert cls(lib.achip_compress_bound_batch(None, op, p, p, p, -1)) == INVALID_ARGUMENT
        assert lib.achip_compress_bound_batch(None, op, p, p, p, 0) == 0
        assert cls(lib.achip_compress_bound_batch(None, op, p, p, p, 1)) == INVALID_ARGUMENT  # (no context)
    for align in (0, 3, 8192, -16, 24):
        assert cls(pack(align=align)) == INVALID_ARGUMENT, align
    assert b"align" in lib.achip_last_error()
    for align in (1, 2, 16, 4096):
        assert pack(align=align) == 0
        assert pack(align=align, base=None, cap=0) == 0
        assert cls(pack(n=-1, align=align)) == INVALID_ARGUMENT
        assert cls(pack(n=1, align=align)) == INVALID_ARGUMENT  # (no context)
    for given in range(1, 7):  # the raw arrays partly given, with and without `stored`
        raw = tuple(p if (given >> k) & 1 else None for k in range(3))
        assert cls(pack(raw=raw)) == INVALID_ARGUMENT, given
        assert cls(pack(raw=raw, stored=p)) == INVALID_ARGUMENT, given
    assert b"raw" in lib.achip_last_error()
    assert cls(pack(stored=p)) == INVALID_ARGUMENT  # stored without raw
    assert cls(pack(raw=(p, p, p))) == INVALID_ARGUMENT  # raw without stored
    assert b"stored" in lib.achip_last_error()
    assert pack(raw=(p, p, p), stored=p) == 0
    assert cls(pack(raw=(p, p, p), stored=p, n=1)) == INVALID_ARGUMENT  # (no context)


def test_host_bound_functions_are_the_restated_formulas(lib):
    """the host functions now call the helpers the bound kernel calls: they still return what the formulas say"""
    from tests import pack_cases as cases
    for name in cases.COMPRESS_OPS:
        for buffer_size in ((cases.HADOOP_DEFAULT_BUFFER, cases.HADOOP_OTHER_BUFFER, 64) if "hadoop" in name else (0,)):
            for n in [x for x in cases.BOUND_LENGTHS if x >= 0] + [1000003, 262144 * 7 + 5]:
                exact = cases.exact_bound(name, n, buffer_size)
                if exact <= cases.INT32_MAX:
                    assert cases.host_bound(lib, name, n, buffer_size) == exact, (name, n, buffer_size)
    for name in ("lz4frame", "snappyframed", "zstdstream", "lz4hadoop"):  # the checked ones refuse a negative length and an overflow as before
        assert cases.host_bound(lib, name, -1) < 0
    assert lib.achip_lz4frame_max_compressed_length(cases.INT32_MAX) < 0 and lib.achip_snappyframed_max_compressed_length(cases.INT32_MAX) < 0
    assert lib.achip_lz4_max_compressed_length(-1) == 15 and lib.achip_snappy_max_compressed_length(-6) == 25  # (the unchecked ones: plain int arithmetic)


def test_batch_codec_methods_reach_the_library(lib):
    """HipBatchCodec's thin methods without a device: an empty batch goes through the binding (argument count and carriers) and launches nothing; a bad
    argument comes back as the exception the other batch calls raise"""
    import types
    import aircompressor_amd as A
    for name in ("compress_bounds", "pack_outputs", "compress_packed"):
        assert callable(getattr(A.HipBatchCodec, name))
    codec = object.__new__(A.HipBatchCodec)  # (no context: the constructor wants a GPU)
    codec.lib = lib
    codec.native = types.SimpleNamespace(ctx=None)
    a = np.zeros(4, dtype=np.int64)
    p = a.ctypes.data
    codec.compress_bounds(A.OP_ZSTD_COMPRESS, p, p, p, 0)
    codec.pack_outputs(p, p, p, p, 0, 16, p, 32, p, p, p)
    codec.pack_outputs(p, p, p, p, 0, 16, None, 0, p, p, p, raw=p, raw_off=p, raw_len=p, stored=p)
    with pytest.raises(A.IllegalArgumentException):
        codec.compress_bounds(A.OP_ZSTD_DECOMPRESS, p, p, p, 0)
    with pytest.raises(A.IllegalArgumentException):
        codec.pack_outputs(p, p, p, p, 0, 24, p, 32, p, p, p)
    with pytest.raises(A.IllegalArgumentException):
        codec.pack_outputs(p, p, p, p, 0, 16, p, 32, p, p, p, raw=p)
