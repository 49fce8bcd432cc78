"""The LZO surface of the C ABI without a device: symbols exported and bound, the bound's arithmetic, the new ops accepted and "no op" (15) still refused, empty
batches, detail messages, options, and the Python classes failing loudly where there is no GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 3
SYMBOLS = ("achip_lzo_max_compressed_length", "achip_lzo_decompress_batch", "achip_lzo_compress_batch", "achip_lzo_decompress", "achip_lzo_compress")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library()
    import aircompressor_amd as A
    return A.load_library()


def test_symbols_are_exported_bound_and_declared(lib):
    from aircompressor_amd import native
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIBRARY_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (achip_[a-z0-9_]+)", out))
    header = open(os.path.join(ROOT, "include", "aircompressor_hip.h")).read()
    java = open(os.path.join(ROOT, "java", "io", "airlift", "compress", "v3", "hip", "HipNative.java")).read()
    for name in SYMBOLS:
        assert name in exported and name in native.SIGNATURES and re.search(r"\b%s\(" % name, header) and '"%s"' % name in java, name
    assert native.SIGNATURES["achip_lzo_decompress_batch"] == native.SIGNATURES["achip_lz4_decompress_batch"]
    assert native.SIGNATURES["achip_lzo_compress"] == native.SIGNATURES["achip_lz4_compress"]
    assert re.search(r"#define ACHIP_OP_LZO_DECOMPRESS 16\b", header) and re.search(r"#define ACHIP_OP_LZO_COMPRESS 17\b", header)
    assert not re.search(r"#define ACHIP_OP_\w+ 15\b", header)
    assert "OP_LZO_DECOMPRESS = 16" in java and "OP_LZO_COMPRESS = 17" in java
    import aircompressor_amd as A
    assert (A.OP_LZO_DECOMPRESS, A.OP_LZO_COMPRESS) == (16, 17)
    for cls in ("LzoHipCompressor", "LzoHipDecompressor"):
        assert os.path.exists(os.path.join(ROOT, "java", "io", "airlift", "compress", "v3", "lzo", cls + ".java")) and hasattr(A, cls)


def test_max_compressed_length(lib):
    from tests import lzo_ref
    for n, want in ((0, 16), (1, 17), (254, 270), (255, 272), (65536, 65809)):
        assert lib.achip_lzo_max_compressed_length(n) == want == lzo_ref.max_compressed_length(n)
    assert lib.achip_lzo_max_compressed_length(-1) == 15 == lzo_ref.max_compressed_length(-1)  # Java's int arithmetic: -1 + -1 / 255 + 16
    assert lib.achip_lzo_max_compressed_length(-1000) == lzo_ref.max_compressed_length(-1000) == -987
    assert lib.achip_lzo_max_compressed_length(0x7E000000) == lzo_ref.max_compressed_length(0x7E000000)


def test_ops_16_and_17_are_taken_and_15_is_refused(lib):
    a = np.zeros(4, dtype=np.int64)
    p = a.ctypes.data
    # sizes: 16 is a decode op, 17 and 15 are not
    assert lib.achip_decoded_size_batch(None, 16, p, p, p, p, p, p, 0) == 0
    assert lib.achip_status_class(lib.achip_decoded_size_batch(None, 16, p, p, p, p, p, p, 1)) == INVALID_ARGUMENT and b"ctx" in lib.achip_last_error()
    for op in (15, 17, 18):
        assert lib.achip_status_class(lib.achip_decoded_size_batch(None, op, p, p, p, p, p, p, 0)) == INVALID_ARGUMENT, op
        assert b"codecOp" in lib.achip_last_error()
    # bounds: 17 is a compress op, 16 and 15 are not
    assert lib.achip_compress_bound_batch(None, 17, p, p, p, 0) == 0
    assert lib.achip_status_class(lib.achip_compress_bound_batch(None, 17, p, p, p, 1)) == INVALID_ARGUMENT and b"ctx" in lib.achip_last_error()
    for op in (15, 16, 18):
        assert lib.achip_status_class(lib.achip_compress_bound_batch(None, op, p, p, p, 0)) == INVALID_ARGUMENT, op
        assert b"codecOp" in lib.achip_last_error()


def test_empty_batches_and_missing_contexts(lib):
    a = np.zeros(4, dtype=np.int64)
    p = a.ctypes.data
    batch = (p, p, p, p, p, p, p, p, p)
    for fn in (lib.achip_lzo_decompress_batch, lib.achip_lzo_compress_batch):
        assert lib.achip_status_class(fn(None, *batch, 0)) == INVALID_ARGUMENT  # (as the LZ4 twins: the context is looked at first)
        assert lib.achip_status_class(fn(None, *batch, 1)) == INVALID_ARGUMENT
    assert lib.achip_status_class(lib.achip_lz4_decompress_batch(None, *batch, 0)) == INVALID_ARGUMENT
    eo = ctypes.c_int64()
    for fn in (lib.achip_lzo_decompress, lib.achip_lzo_compress):
        assert lib.achip_status_class(fn(None, p, p, 1, 1, ctypes.byref(eo))) == INVALID_ARGUMENT
    one_null = (ctypes.c_void_p * 1)(None)
    for op in (16, 17):
        assert lib.achip_status_class(lib.achip_multi_batch_host(one_null, 1, op, None, p, p, p, p, p, p, p, p, p, 1, None)) == INVALID_ARGUMENT
        assert b"null" in lib.achip_last_error()


def test_detail_messages(lib):
    assert lib.achip_detail_message(111) == b"Malformed input"
    assert lib.achip_detail_message(112) == b"Max input length exceeded"
    assert lib.achip_detail_message(113).startswith(b"Max output length must be larger than")
    st = -(1 + 16 * 111)
    assert lib.achip_status_class(st) == 1 and lib.achip_status_detail(st) == 111
    header = open(os.path.join(ROOT, "include", "aircompressor_hip.h")).read()
    for name, value in (("ACHIP_D_LZO_MALFORMED", 111), ("ACHIP_D_LZO_MAX_INPUT", 112), ("ACHIP_D_LZO_MAX_OUTPUT", 113)):
        assert re.search(r"\b%s = %d\b" % (name, value), header)
    values = re.findall(r"\bACHIP_D_\w+ = (\d+)", header)
    assert len(values) == len(set(values))  # the new details sit on free numbers


def test_codecs_fail_loudly_without_gpu(lib):
    import aircompressor_amd as A
    if lib.achip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    assert not A.LzoHipCompressor.is_enabled() and not A.LzoHipDecompressor.is_enabled()
    for cls in (A.LzoHipCompressor, A.LzoHipDecompressor):
        with pytest.raises(A.HipUnavailableError):
            cls()
