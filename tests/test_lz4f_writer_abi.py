"""achip_ctx_set_lz4frame_writer / _get_ and achip_lz4frame_max_compressed_length_for without a device: the symbols are exported, typed, declared and bound in
Java; the setter checks its values in the order of its arguments, before the context is looked at; the bound is the model's formula, the INT32_MAX edge included;
the Python class refuses bad arguments before it asks for a device.  A context cannot be made without a device, so the store behind the setter and getter
(achip_settings.h: plain C++) is compiled with g++ and driven directly: the defaults, what a set stores, that a refused set keeps every value, that a copy of the
settings carries them, which writer a launch takes.  (The same on a live context: tests/test_gpu_lz4f_writer.py.)"""
import ctypes
import os
import re
import subprocess

import pytest

from tests import lz4f_writer_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, BAD_ARGUMENT = 3, 102
SYMBOLS = ("achip_ctx_set_lz4frame_writer", "achip_ctx_get_lz4frame_writer", "achip_lz4frame_max_compressed_length_for")
BLOCK_TEXT, BC_TEXT, CC_TEXT, CS_TEXT = ref.REFUSALS


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
    i32, vp, P = ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER
    assert native.SIGNATURES["achip_ctx_set_lz4frame_writer"] == (i32, [vp, i32, i32, i32, i32])
    assert native.SIGNATURES["achip_ctx_get_lz4frame_writer"] == (i32, [vp, P(i32), P(i32), P(i32), P(i32)])
    assert native.SIGNATURES["achip_lz4frame_max_compressed_length_for"] == (i32, [i32, i32, i32, i32, i32])
    for method in ("set_lz4frame_writer", "get_lz4frame_writer"):
        assert callable(getattr(native.HipNative, method)), method
    header = open(os.path.join(ROOT, "include", "aircompressor_hip.h")).read()
    for decl in ("int32_t achip_ctx_set_lz4frame_writer(achip_ctx* ctx, int32_t blockMaxSize, int32_t blockChecksum, int32_t contentChecksum, int32_t contentSize);",
                 "int32_t achip_ctx_get_lz4frame_writer(achip_ctx* ctx, int32_t* blockMaxSize, int32_t* blockChecksum, int32_t* contentChecksum, int32_t* contentSize);",
                 "int32_t achip_lz4frame_max_compressed_length_for(int32_t uncompressedSize, int32_t blockMaxSize, int32_t blockChecksum, int32_t contentChecksum, int32_t contentSize);"):
        assert decl in header, decl
    assert re.search(r"#define ACHIP_LZ4F_DEFAULT_BLOCK_MAX_SIZE 4194304\b", header)
    # the declaration says what the values apply to and what they leave alone
    section = header[header.index("Lz4FrameCompression.compress writes one shape of frame"):header.index("int32_t achip_lz4frame_max_compressed_length_for")]
    for words in ("M/lz4/Lz4FrameCompression.java:98-132", "achip_lz4frame_compress_batch", "achip_lz4frame_compress,", "achip_batch_host", "achip_mixed_batch", "achip_multi_batch_host",
                  "achip_compress_bound_batch", "ACHIP_D_LZ4F_MAX_OUTPUT", "ACHIP_D_UNSUPPORTED", "do NOT change", "helper contexts take a copy", "lz4frame.compress.variant", BLOCK_TEXT,
                  "(4194304, 0, 0, 0)"):
        assert words in " ".join(section.replace(" * ", " ").split()), words
    java = open(os.path.join(ROOT, "java", "io", "airlift", "compress", "v3", "hip", "HipNative.java")).read()
    assert '@NativeSignature(name = "achip_ctx_set_lz4frame_writer", returnType = int.class, argumentTypes = {MemorySegment.class, int.class, int.class, int.class, int.class})' in java
    assert ('@NativeSignature(name = "achip_ctx_get_lz4frame_writer", returnType = int.class, argumentTypes = {MemorySegment.class, MemorySegment.class, MemorySegment.class, '
            'MemorySegment.class, MemorySegment.class})') in java
    assert '@NativeSignature(name = "achip_lz4frame_max_compressed_length_for", returnType = int.class, argumentTypes = {int.class, int.class, int.class, int.class, int.class})' in java
    twin = open(os.path.join(ROOT, "java", "io", "airlift", "compress", "v3", "lz4", "Lz4FrameHipCompressor.java")).read()
    assert "public Lz4FrameHipCompressor(int device, int acceleration, int blockMaxSize, boolean blockChecksum, boolean contentChecksum, boolean contentSize)" in twin
    assert "setLz4FrameWriter(blockMaxSize, blockChecksum, contentChecksum, contentSize)" in twin
    # the frame settings are no entries of the option table; the variant is an option
    settings = open(os.path.join(ROOT, "aircompressor_amd", "csrc", "achip_settings.h")).read()
    assert "lz4fBlock" not in re.search(r"kOptions\[\] = \{(.*?)\n\};", settings, re.S).group(1)
    assert '"lz4frame.compress.variant", &KernelSettings::lz4fCompressVariant, range(0, 1)' in settings


def test_the_setter_checks_its_arguments_in_order_without_a_device(lib):
    set_writer = lib.achip_ctx_set_lz4frame_writer
    # the block-maximum size comes first, whatever else is wrong
    for block in (0, -1, 65535, 65537, 131072, 4194305, 8388608, 1 << 30, -(1 << 31), 4, 7):
        for flags in ((0, 0, 0), (2, 2, 2), (1, -1, 0)):
            assert refused(lib, set_writer(None, block, *flags)), block
            assert lib.achip_last_error().decode() == BLOCK_TEXT, block
    # then the three flags in turn
    for bad in (2, -1, 256):
        assert refused(lib, set_writer(None, 65536, bad, bad, bad)) and lib.achip_last_error().decode() == BC_TEXT
        assert refused(lib, set_writer(None, 65536, 1, bad, bad)) and lib.achip_last_error().decode() == CC_TEXT
        assert refused(lib, set_writer(None, 65536, 0, 1, bad)) and lib.achip_last_error().decode() == CS_TEXT
    # good values, the context missing: still INVALID_ARGUMENT, another text
    for block in ref.BLOCK_SIZES:
        for flags in ((0, 0, 0), (1, 1, 1), (0, 1, 0)):
            assert refused(lib, set_writer(None, block, *flags))
            text = lib.achip_last_error().decode()
            assert "ctx" in text and "must be" not in text
    v = [ctypes.c_int32(-5) for _ in range(4)]
    assert refused(lib, lib.achip_ctx_get_lz4frame_writer(None, *(ctypes.byref(x) for x in v))) and [x.value for x in v] == [-5] * 4
    # the model refuses the same values with the same texts
    assert ref.check_arguments(65535, 0, 0, 0) == BLOCK_TEXT and ref.check_arguments(65536, 2, 0, 0) == BC_TEXT and ref.check_arguments(65536, 1, 1, 1) is None


def test_the_bound_is_the_models_formula(lib):
    bound = lib.achip_lz4frame_max_compressed_length_for
    flag_sets = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    for block in ref.BLOCK_SIZES:
        for flags in flag_sets:
            for n in (0, 1, 12, block - 1, block, block + 1, 3 * block + 777, 1000003, (1 << 27) + 1, 1 << 30):
                want = ref.max_compressed_length(n, block, *flags)
                assert bound(n, block, *flags) == want, (n, block, flags)
                each = 4 + 4 * flags[0]
                lz4 = lambda m: m + m // 255 + 16  # noqa: E731
                assert want == 7 + 8 * flags[2] + (n // block) * (each + lz4(block)) + (each + lz4(n % block) if n % block else 0) + 4 + 4 * flags[1]
            # beyond an int: the largest n that fits (by bisection over the model's formula, which grows with n), and the first that does not
            lo, hi = 0, 0x7FFFFFFF
            while lo < hi:
                mid = (lo + hi + 1) // 2
                lo, hi = (mid, hi) if ref.max_compressed_length(mid, block, *flags) <= 0x7FFFFFFF else (lo, mid - 1)
            assert 0 < lo < 0x7FFFFFFF
            assert bound(lo, block, *flags) == ref.max_compressed_length(lo, block, *flags) > 0, (block, flags)
            assert refused(lib, bound(lo + 1, block, *flags)), (block, flags)
            assert "exceeds Integer.MAX_VALUE" in lib.achip_last_error().decode()
            assert refused(lib, bound(0x7FFFFFFF, block, *flags))
    # at the Java writer's settings it is still this writer's bound, not Java's formula -- which stays what it was
    assert bound(100, *ref.DEFAULT) == 7 + 4 + 100 + 0 + 16 + 4 == lib.achip_lz4frame_max_compressed_length(100) + 16
    assert lib.achip_lz4frame_max_compressed_length((4 << 20) + 1) == 7 + 4 + (4 << 20) + 1 + 8
    # a negative size, then the setter's checks with its texts
    for n in (-1, -(1 << 31)):
        assert refused(lib, bound(n, 65536, 0, 0, 0)) and "negative" in lib.achip_last_error().decode()
        assert refused(lib, bound(n, 5, 2, 2, 2)) and "negative" in lib.achip_last_error().decode()
    for args, text in (((5, 0, 0, 0), BLOCK_TEXT), ((0, 2, 2, 2), BLOCK_TEXT), ((65536, 2, 2, 2), BC_TEXT), ((65536, 0, -1, 2), CC_TEXT), ((4194304, 1, 1, 3), CS_TEXT)):
        assert refused(lib, bound(100, *args)) and lib.achip_last_error().decode() == text, args


def test_the_python_class_refuses_before_it_asks_for_a_device(lib):
    import aircompressor_amd as A
    for kw, text in (({"block_size": 0}, BLOCK_TEXT), ({"block_size": 65535}, BLOCK_TEXT), ({"block_size": 131072, "block_checksum": 2}, BLOCK_TEXT),
                     ({"block_size": 65536, "block_checksum": 2, "content_size": 5}, BC_TEXT), ({"content_checksum": -1}, CC_TEXT), ({"content_size": 2}, CS_TEXT)):
        with pytest.raises(A.IllegalArgumentException) as e:
            A.Lz4FrameHipCompressor(**kw)
        assert str(e.value) == text, kw
    with pytest.raises(A.IllegalArgumentException) as e:  # (the acceleration's check is still there)
        A.Lz4FrameHipCompressor(acceleration=0, block_size=65536)
    assert "acceleration" in str(e.value)
    if lib.achip_device_count() <= 0:
        with pytest.raises(A.HipUnavailableError):  # (good values get as far as the device)
            A.Lz4FrameHipCompressor(block_size=65536, block_checksum=True, content_checksum=True, content_size=True)
        with pytest.raises(A.HipUnavailableError):
            A.Lz4FrameHipCompressor()


DRIVER = r"""
#include "achip_settings.h"
#include <cstdio>
#include <cstdlib>
static void show(const char* what, int r, const achip::KernelSettings& k)
{
    printf("%s %d : %d %d %d %d list %d\n", what, r, k.lz4fBlockMaxSize, k.lz4fBlockChecksum, k.lz4fContentChecksum, k.lz4fContentSize, (int)achip::lz4f_list_writer(k));
}
int main(int argc, char** argv)
{
    achip::Settings s;
    show("defaults", 0, s.kernel);
    for (int i = 1; i + 3 < argc; i += 4) {
        const int r = (int)achip::set_lz4f_writer(s.kernel, atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]));
        show("writer", r, s.kernel);
    }
    achip::Settings copy = s;  // what a mixed batch's helper contexts take
    show("copy", 0, copy.kernel);
    achip::Settings v;
    const char* refusal = nullptr;
    printf("variant %d %d", (int)achip::apply(v, "lz4frame.compress.variant", 2, &refusal), v.kernel.lz4fCompressVariant);
    printf(" %d", (int)achip::apply(v, "lz4frame.compress.variant", 1));
    show("", v.kernel.lz4fCompressVariant, v.kernel);
    printf("refusal %s\n", refusal);
}
"""


def test_settings_hold_the_values_and_a_refused_set_keeps_them(tmp_path):
    src = tmp_path / "lz4f_settings.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "lz4f_settings")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aircompressor_amd", "csrc"), "-o", exe, str(src)], check=True)
    NONE, BLOCK, BC, CC, CS = 0, 1, 2, 3, 4
    calls = [(65536, 1, 0, 1, NONE), (65535, 0, 0, 0, BLOCK), (0, 2, 2, 2, BLOCK), (262144, 2, 0, 0, BC), (262144, 0, -1, 0, CC), (262144, 0, 0, 7, CS), (1048576, 0, 1, 0, NONE),
             (4194304, 0, 0, 0, NONE), (4194304, 0, 0, 1, NONE), (4194304, 1, 1, 1, NONE), (131072, 1, 1, 1, BLOCK)]
    out = subprocess.run([exe] + [str(v) for c in calls for v in c[:4]], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == "defaults 0 : 4194304 0 0 0 list 0"
    held = ref.DEFAULT
    for line, call in zip(out[1:], calls):
        if call[4] == NONE:
            held = call[:4]
        assert line == "writer %d : %d %d %d %d list %d" % ((call[4],) + tuple(held) + (int(tuple(held) != ref.DEFAULT),)), (line, call)
    assert held == (4194304, 1, 1, 1)
    assert out[1 + len(calls)] == "copy 0 : 4194304 1 1 1 list 1"
    # the option: 0 or 1; a refused value keeps the old one; 1 takes the block list at the default settings too
    assert out[2 + len(calls)] == "variant 2 0 0 1 : 4194304 0 0 0 list 1"
    assert out[3 + len(calls)].startswith("refusal lz4frame.compress.variant: 0 ")
