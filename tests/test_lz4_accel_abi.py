"""achip_ctx_set_lz4_acceleration / achip_ctx_get_lz4_acceleration without a device: both symbols are exported, typed, declared and bound in Java; a value outside
[1, 65537] is refused with the reference's text before the context is looked at; the Python compressors refuse it the same way before they ask for a device."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, BAD_ARGUMENT = 3, 102
TEXT = "LZ4 acceleration should be in the [1, 65537] range but got %d"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library()
    import aircompressor_amd as A
    return A.load_library()


def test_symbols_are_exported_typed_declared_and_bound(lib):
    from aircompressor_amd import native
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIBRARY_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (achip_[a-z0-9_]+)", out))
    assert {"achip_ctx_set_lz4_acceleration", "achip_ctx_get_lz4_acceleration"} <= exported
    i32, vp = ctypes.c_int32, ctypes.c_void_p
    assert native.SIGNATURES["achip_ctx_set_lz4_acceleration"] == (i32, [vp, i32])
    assert native.SIGNATURES["achip_ctx_get_lz4_acceleration"] == (i32, [vp])
    assert callable(native.HipNative.set_lz4_acceleration) and callable(native.HipNative.get_lz4_acceleration)
    header = open(os.path.join(ROOT, "include", "aircompressor_hip.h")).read()
    assert "int32_t achip_ctx_set_lz4_acceleration(achip_ctx* ctx, int32_t acceleration);" in header
    assert "int32_t achip_ctx_get_lz4_acceleration(achip_ctx* ctx);" in header
    assert re.search(r"#define ACHIP_LZ4_DEFAULT_ACCELERATION 1\b", header) and re.search(r"#define ACHIP_LZ4_MAX_ACCELERATION 65537\b", header)
    # the declaration cites the reference, and says what the value applies to and what it leaves alone
    section = header[header.index("Lz4Compressor.create(int acceleration)"):header.index("int32_t achip_ctx_get_lz4_acceleration")]
    for words in ("M/lz4/Lz4Compressor.java:33-41", "M/lz4/Lz4NativeCompressor.java:34-41", "M/lz4/Lz4FrameNativeCompressor.java:37-40", "M/lz4/Lz4Native.java:49-50",
                  "achip_lz4_compress_batch", "achip_lz4frame_compress", "achip_mixed_batch", "achip_multi_batch_host", "does NOT change", "Hadoop"):
        assert words in section, words
    java = open(os.path.join(ROOT, "java", "io", "airlift", "compress", "v3", "hip", "HipNative.java")).read()
    assert '@NativeSignature(name = "achip_ctx_set_lz4_acceleration", returnType = int.class, argumentTypes = {MemorySegment.class, int.class})' in java
    assert '@NativeSignature(name = "achip_ctx_get_lz4_acceleration", returnType = int.class, argumentTypes = MemorySegment.class)' in java
    for cls in ("Lz4HipCompressor", "Lz4FrameHipCompressor"):
        text = open(os.path.join(ROOT, "java", "io", "airlift", "compress", "v3", "lz4", cls + ".java")).read()
        assert "int acceleration)" in text and "setLz4Acceleration(acceleration)" in text, cls
    # not an entry of the option table
    assert "acceleration" not in re.search(r"kOptions\[\] = \{(.*?)\n\};", open(os.path.join(ROOT, "aircompressor_amd", "csrc", "achip_settings.h")).read(), re.S).group(1)


def test_values_outside_the_range_are_refused_without_a_device(lib):
    for bad in (0, -1, 65538):
        r = lib.achip_ctx_set_lz4_acceleration(None, bad)
        assert lib.achip_status_class(r) == INVALID_ARGUMENT and lib.achip_status_detail(r) == BAD_ARGUMENT, bad
        assert lib.achip_last_error().decode() == TEXT % bad
    for good in (1, 2, 65537):  # the value is fine, the context is missing: still INVALID_ARGUMENT, another text
        r = lib.achip_ctx_set_lz4_acceleration(None, good)
        assert lib.achip_status_class(r) == INVALID_ARGUMENT and "acceleration" not in lib.achip_last_error().decode()
    assert lib.achip_status_class(lib.achip_ctx_get_lz4_acceleration(None)) == INVALID_ARGUMENT


def test_python_compressors_refuse_before_they_ask_for_a_device(lib):
    import aircompressor_amd as A
    for cls in (A.Lz4HipCompressor, A.Lz4FrameHipCompressor):
        for bad in (0, -1, 65538):
            with pytest.raises(A.IllegalArgumentException) as e:
                cls(acceleration=bad)
            assert str(e.value) == TEXT % bad
        if lib.achip_device_count() <= 0:
            with pytest.raises(A.HipUnavailableError):  # (a good value gets as far as the device)
                cls(acceleration=2)
