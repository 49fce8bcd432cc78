"""achip_ctx_set_lz4frame_linked_blocks / achip_ctx_get_lz4frame_linked_blocks without a device: the symbols are exported, typed, declared and bound in Python and
in Java; the setter checks its value before the context is looked at; the Python class takes the argument without asking for a device.  A context cannot be made
without a device, so the store behind the setter and the getter (achip_settings.h: plain C++) is compiled with g++ and driven directly: the default, what a set
stores, that a refused set keeps the value, that a copy of the settings -- a mixed batch's helper context -- carries it.  (On a live context: tests/test_gpu_lz4_linked.py.)"""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, BAD_ARGUMENT = 3, 102
SYMBOLS = ("achip_ctx_set_lz4frame_linked_blocks", "achip_ctx_get_lz4frame_linked_blocks")


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
    assert set(SYMBOLS) <= set(re.findall(r"\bT (achip_[a-z0-9_]+)", out))
    i32, vp = ctypes.c_int32, ctypes.c_void_p
    assert native.SIGNATURES["achip_ctx_set_lz4frame_linked_blocks"] == (i32, [vp, i32])
    assert native.SIGNATURES["achip_ctx_get_lz4frame_linked_blocks"] == (i32, [vp])
    for method in ("set_lz4frame_linked_blocks", "get_lz4frame_linked_blocks"):
        assert callable(getattr(native.HipNative, method)), method
    header = open(os.path.join(ROOT, "include", "aircompressor_hip.h")).read()
    for decl in ("int32_t achip_ctx_set_lz4frame_linked_blocks(achip_ctx* ctx, int32_t accept);", "int32_t achip_ctx_get_lz4frame_linked_blocks(achip_ctx* ctx);"):
        assert decl in header, decl
    # the declaration says what it replaces (nothing), what it applies to and what it leaves alone
    section = header[header.index("replaces nothing in the reference"):header.index("int32_t achip_ctx_set_lz4frame_linked_blocks")]
    section = " ".join(section.replace(" * ", " ").split())
    for words in ("M/lz4/Lz4FrameCompression.java:213-216", "OFF by default", "helper contexts take a copy", "65 535", "SAME frame", "ACHIP_D_LZ4_OFFSET_OUTSIDE",
                  "ACHIP_D_LZ4F_DICTIONARY", "achip_lz4frame_decompress_batch", "achip_lz4frame_decompress,", "achip_batch_host", "achip_mixed_batch", "achip_mixed_batch_host",
                  "achip_multi_batch_host", "achip_decoded_size_batch", "does NOT change", "any encoder", "any bound", "Hadoop LZ4 streams", "ACHIP_D_BAD_ARGUMENT",
                  "before the context is looked at"):
        assert words in section, words
    java = open(os.path.join(ROOT, "java", "io", "airlift", "compress", "v3", "hip", "HipNative.java")).read()
    assert '@NativeSignature(name = "achip_ctx_set_lz4frame_linked_blocks", returnType = int.class, argumentTypes = {MemorySegment.class, int.class})' in java
    assert '@NativeSignature(name = "achip_ctx_get_lz4frame_linked_blocks", returnType = int.class, argumentTypes = MemorySegment.class)' in java
    assert "public void setLz4FrameLinkedBlocks(boolean accept)" in java and "public boolean getLz4FrameLinkedBlocks()" in java
    reader = open(os.path.join(ROOT, "java", "io", "airlift", "compress", "v3", "lz4", "Lz4FrameHipDecompressor.java")).read()
    assert "public Lz4FrameHipDecompressor(boolean acceptLinkedBlocks)" in reader and "setLz4FrameLinkedBlocks(acceptLinkedBlocks)" in reader
    assert re.search(r"public Lz4FrameHipDecompressor\(int device\)\s*\{\s*this\(device, false\);", reader)  # the default stays the Java reader's
    # a property of the reader, not an entry of the option table
    table = re.search(r"kOptions\[\] = \{(.*?)\n\};", open(os.path.join(ROOT, "aircompressor_amd", "csrc", "achip_settings.h")).read(), re.S).group(1)
    assert "linked" not in table.lower()


def test_the_setter_checks_its_value_before_the_context(lib):
    for value in (2, -1, 256, 65536, -2147483648, 2147483647):
        assert refused(lib, lib.achip_ctx_set_lz4frame_linked_blocks(None, value)), value
        assert "accept must be 0 or 1" in lib.achip_last_error().decode()
    for value in (0, 1):  # in range: what is refused now is the context
        assert refused(lib, lib.achip_ctx_set_lz4frame_linked_blocks(None, value))
        text = lib.achip_last_error().decode()
        assert "accept" not in text and "ctx" in text
    assert refused(lib, lib.achip_ctx_get_lz4frame_linked_blocks(None))
    assert "ctx" in lib.achip_last_error().decode()


def test_the_python_reader_takes_the_argument(lib):
    """the class keeps the value and hands it to its context before every call (tests/test_gpu_lz4_linked.py sees it arrive); the default is the Java reader's"""
    import inspect
    from aircompressor_amd import codecs

    class Ctx:  # (no device: the object only stores the context)
        lib = None
        calls = []

        def set_lz4frame_linked_blocks(self, accept):
            self.calls.append(accept)
    sig = inspect.signature(codecs.Lz4FrameHipDecompressor.__init__)
    assert sig.parameters["accept_linked_blocks"].default is False
    assert codecs.Lz4FrameHipDecompressor(native_ctx=Ctx()).accept_linked_blocks is False
    d = codecs.Lz4FrameHipDecompressor(native_ctx=Ctx(), accept_linked_blocks=1)
    assert d.accept_linked_blocks is True
    d._call = lambda name, src, dst: (7, 0)
    assert d._decompress(None, None) == 7 and Ctx.calls == [True]


DRIVER = r"""
#include "achip_settings.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv)
{
    achip::Settings s;
    printf("default %d\n", s.kernel.lz4fLinkedBlocks);
    for (int i = 1; i < argc; i++) {
        const bool ok = achip::set_lz4f_linked_blocks(s.kernel, atoi(argv[i]));
        printf("set %d : %d\n", ok ? 1 : 0, s.kernel.lz4fLinkedBlocks);
    }
    achip::Settings copy = s;  // what a mixed batch's helper contexts take
    printf("copy %d\n", copy.kernel.lz4fLinkedBlocks);
    printf("others %d %d\n", s.kernel.lz4Acceleration, s.lz4FrameDecompressVariant);
}
"""


def test_settings_hold_the_value_and_a_refused_set_keeps_it(tmp_path):
    src = tmp_path / "linked_settings.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "linked_settings")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aircompressor_amd", "csrc"), "-o", exe, str(src)], check=True)
    calls = [1, 2, -1, 0, 256, 1, 65536]
    out = subprocess.run([exe] + [str(v) for v in calls], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == "default 0"
    held = 0
    for line, v in zip(out[1:], calls):
        ok = v in (0, 1)
        held = v if ok else held
        assert line == "set %d : %d" % (ok, held), (line, v)
    assert out[1 + len(calls):] == ["copy 1", "others 1 2"]
