"""achip_ctx_set_snappyframed_writer / _get_, achip_ctx_set_snappyframed_verify_checksums / _get_ and achip_snappyframed_max_compressed_length_for without a device:
the symbols are exported, typed, declared and bound in Java; the setters check their values before the context is looked at, in the reference constructor's order
and with its texts; the bound is the model's formula, overflow included; the Python classes refuse bad arguments before they ask for a device.  A context cannot
be made without a device, so the store behind the setters and getters (achip_settings.h: plain C++) is compiled with g++ and driven directly: the defaults, what a
set stores, that a refused set keeps every value, that a copy of the settings carries them.  (The same on a live context: tests/test_gpu_snf_params.py.)"""
import ctypes
import math
import os
import re
import subprocess

import pytest

from tests import snf_params_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, BAD_ARGUMENT = 3, 102
RATIO_TEXT = "minCompressionRatio %s must be between (0,1.0]."
BLOCK_TEXT = "blockSize must be in (0, 65536]"
SYMBOLS = ("achip_ctx_set_snappyframed_writer", "achip_ctx_get_snappyframed_writer", "achip_ctx_set_snappyframed_verify_checksums",
           "achip_ctx_get_snappyframed_verify_checksums", "achip_snappyframed_max_compressed_length_for")
BITS = ref.ratio_bits


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library()
    import aircompressor_amd as A
    return A.load_library()


def refused(lib, r):
    return lib.achip_status_class(r) == INVALID_ARGUMENT and lib.achip_status_detail(r) == BAD_ARGUMENT


def test_symbols_are_exported_typed_declared_and_bound(lib):
    from aircompressor_amd import native
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIBRARY_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (achip_[a-z0-9_]+)", out))
    assert set(SYMBOLS) <= exported
    i32, i64, vp, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER
    assert native.SIGNATURES["achip_ctx_set_snappyframed_writer"] == (i32, [vp, i32, i32, i64])
    assert native.SIGNATURES["achip_ctx_get_snappyframed_writer"] == (i32, [vp, P(i32), P(i32), P(i64)])
    assert native.SIGNATURES["achip_ctx_set_snappyframed_verify_checksums"] == (i32, [vp, i32])
    assert native.SIGNATURES["achip_ctx_get_snappyframed_verify_checksums"] == (i32, [vp])
    assert native.SIGNATURES["achip_snappyframed_max_compressed_length_for"] == (i32, [i32, i32])
    for method in ("set_snappyframed_writer", "get_snappyframed_writer", "set_snappyframed_verify_checksums", "get_snappyframed_verify_checksums"):
        assert callable(getattr(native.HipNative, method)), method
    header = open(os.path.join(ROOT, "include", "aircompressor_hip.h")).read()
    for decl in ("int32_t achip_ctx_set_snappyframed_writer(achip_ctx* ctx, int32_t writeChecksums, int32_t blockSize, int64_t minCompressionRatioBits);",
                 "int32_t achip_ctx_get_snappyframed_writer(achip_ctx* ctx, int32_t* writeChecksums, int32_t* blockSize, int64_t* minCompressionRatioBits);",
                 "int32_t achip_ctx_set_snappyframed_verify_checksums(achip_ctx* ctx, int32_t verify);",
                 "int32_t achip_ctx_get_snappyframed_verify_checksums(achip_ctx* ctx);",
                 "int32_t achip_snappyframed_max_compressed_length_for(int32_t uncompressedSize, int32_t blockSize);"):
        assert decl in header, decl
    assert re.search(r"#define ACHIP_SNF_DEFAULT_BLOCK_SIZE 65536\b", header) and re.search(r"#define ACHIP_SNF_MAX_BLOCK_SIZE +65536\b", header)
    assert re.search(r"#define ACHIP_SNF_DEFAULT_MIN_RATIO_BITS 0x3FEB333333333333LL", header)
    assert BITS(0.85) == 0x3FEB333333333333 == BITS(ref.DEFAULT_MIN_COMPRESSION_RATIO)
    # no double crosses the boundary: every type is one NativeLoader.getMemoryLayout binds
    for name in SYMBOLS:
        assert "double" not in re.search(r"[^;]*\b%s\([^;]*;" % name, header).group(0), name
    # the declaration cites the reference, and says what the values apply to and what they leave alone
    section = header[header.index("SnappyFramedOutputStream(compressor, out, writeChecksums, blockSize, minCompressionRatio)"):header.index("int32_t achip_snappyframed_max_compressed_length_for")]
    for words in ("M/snappy/SnappyFramedOutputStream.java:77-91", "M/snappy/SnappyFramedInputStream.java:74-79", ":65-69", "achip_snappyframed_compress_batch", "achip_batch_host",
                  "achip_mixed_batch", "achip_multi_batch_host", "achip_window_compress_batch", "achip_window_decompress", "achip_compress_bound_batch", "ACHIP_D_SNF_MAX_OUTPUT",
                  "do NOT change", "raw Snappy", "Hadoop Snappy", "achip_decoded_size_batch", "helper contexts take a copy", RATIO_TEXT % "<value>".replace("\n", " "), BLOCK_TEXT):
        assert words in " ".join(section.replace(" * ", " ").split()), words
    java = open(os.path.join(ROOT, "java", "io", "airlift", "compress", "v3", "hip", "HipNative.java")).read()
    assert '@NativeSignature(name = "achip_ctx_set_snappyframed_writer", returnType = int.class, argumentTypes = {MemorySegment.class, int.class, int.class, long.class})' in java
    assert '@NativeSignature(name = "achip_ctx_set_snappyframed_verify_checksums", returnType = int.class, argumentTypes = {MemorySegment.class, int.class})' in java
    assert '@NativeSignature(name = "achip_snappyframed_max_compressed_length_for", returnType = int.class, argumentTypes = {int.class, int.class})' in java
    assert "Double.doubleToRawLongBits(minCompressionRatio)" in java and "Double.longBitsToDouble(" in java
    twin = open(os.path.join(ROOT, "java", "io", "airlift", "compress", "v3", "snappy", "SnappyFramedHip.java")).read()
    assert "newChecksumFreeBenchmark" in twin and "setSnappyFramedWriter(writeChecksums, blockSize, minCompressionRatio)" in twin and "setSnappyFramedVerifyChecksums(verifyChecksums)" in twin
    # not entries of the option table
    table = re.search(r"kOptions\[\] = \{(.*?)\n\};", open(os.path.join(ROOT, "aircompressor_amd", "csrc", "achip_settings.h")).read(), re.S).group(1)
    assert "snf" not in table and "Checksums" not in table


def test_the_writer_setter_checks_ratio_then_block_size_then_flags_without_a_device(lib):
    set_writer = lib.achip_ctx_set_snappyframed_writer
    # the ratio: > 0 and <= 1.0, NaN refused; the text prints the double as Java does -- and it comes first, whatever else is wrong
    for ratio, text in ((0.0, "0.0"), (-0.0, "-0.0"), (-1.0, "-1.0"), (1.5, "1.5"), (math.nextafter(1.0, 2.0), "1.0000000000000002"), (float("nan"), "NaN"),
                        (float("inf"), "Infinity"), (float("-inf"), "-Infinity"), (1e10, "1.0E10"), (-2.5e-7, "-2.5E-7"), (100.0, "100.0")):
        for block_size, flag in ((65536, 1), (0, 1), (65537, 7)):
            assert refused(lib, set_writer(None, flag, block_size, BITS(ratio))), (ratio, block_size)
            assert lib.achip_last_error().decode() == RATIO_TEXT % text, (ratio, block_size)
    # then the block size
    for block_size in (0, -1, 65537, 1 << 30, -(1 << 31)):
        for flag in (1, 2):
            assert refused(lib, set_writer(None, flag, block_size, BITS(0.85))), block_size
            assert lib.achip_last_error().decode() == BLOCK_TEXT, block_size
    # then the flag
    for flag in (2, -1, 256):
        assert refused(lib, set_writer(None, flag, 65536, BITS(0.85))), flag
        assert "writeChecksums" in lib.achip_last_error().decode()
    # good values, the context missing: still INVALID_ARGUMENT, another text
    for flag, block_size, ratio in ((1, 65536, 0.85), (0, 1, 1.0), (1, 65535, ref.SMALLEST_RATIO), (0, 4096, math.nextafter(1.0, 0.0))):
        assert refused(lib, set_writer(None, flag, block_size, BITS(ratio))), (flag, block_size, ratio)
        text = lib.achip_last_error().decode()
        assert "minCompressionRatio" not in text and "blockSize" not in text and "writeChecksums" not in text and "ctx" in text
    a, b, c = ctypes.c_int32(-5), ctypes.c_int32(-5), ctypes.c_int64(-5)
    assert refused(lib, lib.achip_ctx_get_snappyframed_writer(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))) and (a.value, b.value, c.value) == (-5, -5, -5)


def test_the_verify_setter_checks_its_flag_without_a_device(lib):
    for flag in (2, -1, 256):
        assert refused(lib, lib.achip_ctx_set_snappyframed_verify_checksums(None, flag)), flag
        assert "verifyChecksums" in lib.achip_last_error().decode()
    for flag in (0, 1):
        assert refused(lib, lib.achip_ctx_set_snappyframed_verify_checksums(None, flag))
        assert "verifyChecksums" not in lib.achip_last_error().decode()
    assert refused(lib, lib.achip_ctx_get_snappyframed_verify_checksums(None))


def test_the_bound_is_the_models_formula(lib):
    bound = lib.achip_snappyframed_max_compressed_length_for
    for block_size in (1, 2, 3, 63, 64, 4096, 65535, 65536):
        for n in (0, 1, block_size - 1, block_size, block_size + 1, 3 * block_size + 7, 1000003, (1 << 27) + 1):
            assert bound(n, block_size) == ref.max_compressed_length(n, block_size) == 10 + 8 * math.ceil(n / block_size) + n, (n, block_size)
    for n in (0, 1, 65535, 65536, 65537, 1 << 30, 0x7FFFFFFF - 10 - 8 * 32768):  # at the default block size: the one-argument function, which is unchanged
        assert bound(n, 65536) == lib.achip_snappyframed_max_compressed_length(n), n
    assert lib.achip_snappyframed_max_compressed_length(100000) == 10 + 8 * 2 + 100000
    # beyond an int: the largest n that fits, and the first that does not
    for block_size in (1, 2, 63, 4096, 65536):
        lo, hi = 0, 0x7FFFFFFF  # (the bound grows with n: the last n that fits, by bisection over the model's formula)
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if ref.max_compressed_length(mid, block_size) <= 0x7FFFFFFF else (lo, mid - 1)
        fits = lo
        assert bound(fits, block_size) == ref.max_compressed_length(fits, block_size) > 0, block_size
        assert refused(lib, bound(fits + 1, block_size)), block_size
        assert "exceeds Integer.MAX_VALUE" in lib.achip_last_error().decode()
    assert refused(lib, bound(1 << 30, 1)) and bound(1 << 30, 65536) > 0
    assert refused(lib, bound(0x7FFFFFFF, 65536)) and refused(lib, bound(0x7FFFFFFF, 1))
    # a negative size, a block size outside (0, 65536]
    for n in (-1, -(1 << 31)):
        assert refused(lib, bound(n, 65536)) and "negative" in lib.achip_last_error().decode()
    for block_size in (0, -1, 65537, -(1 << 31)):
        assert refused(lib, bound(100, block_size)) and lib.achip_last_error().decode() == BLOCK_TEXT


def test_python_classes_refuse_before_they_ask_for_a_device(lib):
    import io
    import aircompressor_amd as A
    for make in (lambda **kw: A.SnappyFramedHipCompressor(**kw), lambda **kw: A.SnappyFramedHipOutputStream(io.BytesIO(), **kw)):
        for ratio, text in ((0.0, "0.0"), (1.5, "1.5"), (float("nan"), "NaN"), (-1.0, "-1.0")):
            with pytest.raises(A.IllegalArgumentException) as e:
                make(block_size=0, min_compression_ratio=ratio)
            assert str(e.value) == RATIO_TEXT % text
        for block_size in (0, -1, 65537):
            with pytest.raises(A.IllegalArgumentException) as e:
                make(block_size=block_size)
            assert str(e.value) == BLOCK_TEXT
        if lib.achip_device_count() <= 0:
            with pytest.raises(A.HipUnavailableError):  # (good values get as far as the device)
                make(write_checksums=False, block_size=4096, min_compression_ratio=1.0)
    if lib.achip_device_count() <= 0:
        with pytest.raises(A.HipUnavailableError):
            A.SnappyFramedHipDecompressor(verify_checksums=False)
    from aircompressor_amd import native
    assert native.double_bits(0.85) == 0x3FEB333333333333 and native.bits_double(0x3FEB333333333333) == 0.85


def test_both_bindings_print_a_refused_ratio_as_java_does(lib):
    """Double.toString, restated in abi_context.cpp and in native.py: the two give the same text for every value, and the text Java gives for these"""
    from aircompressor_amd import native
    known = [(0.0, "0.0"), (-0.0, "-0.0"), (-1.0, "-1.0"), (1.5, "1.5"), (2.0, "2.0"), (100.0, "100.0"), (1e10, "1.0E10"), (1e7, "1.0E7"), (9999999.0, "9999999.0"), (12345678.0, "1.2345678E7"),
             (-2.5e-7, "-2.5E-7"), (-0.001, "-0.001"), (-0.00099, "-9.9E-4"), (-4.9e-324, "-4.9E-324"), (1.7976931348623157e308, "1.7976931348623157E308"), (float("inf"), "Infinity"),
             (float("-inf"), "-Infinity"), (math.nextafter(1.0, 2.0), "1.0000000000000002"), (-0.1, "-0.1"), (123.456, "123.456"), (-2.2250738585072014e-308, "-2.2250738585072014E-308")]
    values = [v for v, _ in known] + [float("nan")] + [-(10.0 ** e) * m for e in range(-30, 31, 3) for m in (1.0, 1.25, 3.3333333333333335)]
    for v in values:
        assert refused(lib, lib.achip_ctx_set_snappyframed_writer(None, 1, 65536, BITS(v))), v
        text = lib.achip_last_error().decode()
        assert text == RATIO_TEXT % native.java_double_text(v), v
    for v, want in known:
        assert native.java_double_text(v) == want, v


DRIVER = r"""
#include "achip_settings.h"
#include <initializer_list>
#include <cstdio>
#include <cstdlib>
static void show(const char* what, int r, const achip::KernelSettings& k)
{
    printf("%s %d : %d %d %lld %d\n", what, r, k.snfWriteChecksums, k.snfBlockSize, (long long)k.snfMinRatioBits, k.snfVerifyChecksums);
}
int main(int argc, char** argv)
{
    achip::Settings s;
    show("defaults", 0, s.kernel);
    for (int i = 1; i + 2 < argc; i += 3) {
        const int r = (int)achip::set_snf_writer(s.kernel, atoi(argv[i]), atoi(argv[i + 1]), strtoll(argv[i + 2], nullptr, 10));
        show("writer", r, s.kernel);
    }
    for (int v : {0, 2, -1, 1}) {
        const int r = (int)achip::set_snf_verify(s.kernel, v);
        show("verify", r, s.kernel);
    }
    achip::Settings copy = s;  // what a mixed batch's helper contexts take
    show("copy", 0, copy.kernel);
}
"""


def test_settings_hold_the_values_and_a_refused_set_keeps_them(tmp_path):
    """the context's store (achip_settings.h, which the setters and getters of abi_context.cpp go through), compiled with g++ as tests/test_options.py compiles it:
    the defaults, what a set stores and the getters read, that a refused set -- for each of the three reasons -- leaves every value as it was, and that a copy of
    the settings (a mixed batch's helper context) carries them"""
    src = tmp_path / "snf_settings.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "snf_settings")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aircompressor_amd", "csrc"), "-o", exe, str(src)], check=True)
    NONE, RATIO, BLOCK, FLAG = 0, 1, 2, 3
    edge = math.nextafter(0.5, 0.0)
    calls = [(0, 4096, BITS(0.5), NONE), (1, 4096, BITS(1.5), RATIO), (1, 0, BITS(0.0), RATIO), (1, 65537, BITS(0.85), BLOCK), (1, 0, BITS(0.85), BLOCK), (2, 1, BITS(1.0), FLAG),
             (1, 1, BITS(float("nan")), RATIO), (1, 1, BITS(edge), NONE), (1, 65536, BITS(1.0), NONE), (0, 65535, BITS(ref.SMALLEST_RATIO), NONE)]
    out = subprocess.run([exe] + [str(v) for c in calls for v in c[:3]], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == "defaults 0 : 1 65536 %d 1" % 0x3FEB333333333333
    held = (1, 65536, 0x3FEB333333333333)
    for line, (checksums, block_size, bits, want) in zip(out[1:], calls):
        if want == NONE:
            held = (checksums, block_size, bits)
        assert line == "writer %d : %d %d %d 1" % ((want,) + held), (line, checksums, block_size, bits)
    assert held == (0, 65535, 1)  # (the smallest positive double is bit pattern 1)
    assert out[1 + len(calls):] == ["verify 0 : 0 65535 1 0", "verify %d : 0 65535 1 0" % FLAG, "verify %d : 0 65535 1 0" % FLAG, "verify 0 : 0 65535 1 1", "copy 0 : 0 65535 1 1"]
