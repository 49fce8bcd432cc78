#!/usr/bin/env python3
"""Writes tests/golden/lzo_vectors.json: what liblzo2 2.03 -- the library among the reference's test resources, src/test/resources/nativelib/Linux-amd64/liblzo2.so,
loaded through ctypes -- and the pure-Python model tests/lzo_ref.py make of every plaintext of tests/lzo_cases.py's encode catalog (and of a few small
text-like plaintexts on top: vector_inputs()).  Per plaintext:

    lzo1x_1, lzo1x_999    the two liblzo2 streams: hex up to 8 KiB, length and SHA-256 beyond (the catalog's plaintexts are small, so most are hex).  The 999 streams
                          hold commands the Java encoder never emits -- 2-byte matches behind one to three literals everywhere, the 3-byte form at 2049 .. 3072 in
                          the stream of "3-byte repeats at 2049..3072": decode vectors for the model, and through it for the kernels
    model                 length and SHA-256 (its first 16 hex digits, as everywhere in the file) of the model's compress() output, and whether liblzo2's lzo1x_decompress_safe restores the plaintext from it
    java                  length and SHA-256 of what the reference's OWN encoder makes of it: LzoRawCompressor.java transliterated to C++ by tools/j2c.py (recipe:
                          tools/lzo_j2c/; runtime: oracle/ref/jrt.h) and compiled into a temporary directory -- nothing of it is kept.  This is the pin of the
                          model's compress() against the Java code itself.  The transliterated LzoRawDecompressor also runs over the decode catalog here:
                          "java_decode" holds, per case label, the Java outcome (length and SHA-256 of the plaintext, or the exception's offset)

Runs only where the reference's checkout is (it reads that library); the tests read the JSON file.  tests/test_lzo_ref.py compares the model with it, so a change
to the model that changes an output has to show here.  Run after a deliberate change to the model or the catalog:   python tools/record_lzo_vectors.py"""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import lzo_cases as cases, lzo_ref as ref  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "lzo_vectors.json")
LIBLZO2 = "/root/reference/src/test/resources/nativelib/Linux-amd64/liblzo2.so"
HEX_LIMIT = 8192


class Liblzo2:
    def __init__(self, path=LIBLZO2):
        self.lib = ctypes.CDLL(path)
        self.version = "%x" % self.lib.lzo_version()

    def compress(self, data, level):
        fn, work = (self.lib.lzo1x_1_compress, 1 << 17) if level == 1 else (self.lib.lzo1x_999_compress, 14 * 16384 * 4)
        out = ctypes.create_string_buffer(len(data) + len(data) // 16 + 64 + 3)
        n = ctypes.c_ulong(len(out))
        r = fn(bytes(data), ctypes.c_ulong(len(data)), out, ctypes.byref(n), ctypes.create_string_buffer(work))
        assert r == 0, r
        return out.raw[:n.value]

    def decompress(self, stream, capacity):
        """-> the plaintext, or None where lzo1x_decompress_safe refuses the stream"""
        out = ctypes.create_string_buffer(capacity + 1)
        n = ctypes.c_ulong(capacity)
        r = self.lib.lzo1x_decompress_safe(bytes(stream), ctypes.c_ulong(len(stream)), out, ctypes.byref(n), None)
        return out.raw[:n.value] if r == 0 else None


class JavaLzo:
    """the reference's LzoRawCompressor / LzoRawDecompressor, transliterated and compiled into `tmp`"""

    def __init__(self, tmp):
        import subprocess
        here = os.path.join(ROOT, "tools", "lzo_j2c")
        gen = os.path.join(tmp, "ref_lzo_gen.h")
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "j2c.py"), "--root", "/root/reference/src/main/java/io/airlift/compress/v3/", "--patches",
                        os.path.join(here, "patches.txt"), "--outer", "RefL", "--manifest", os.path.join(here, "sources.txt"), "--out", gen], check=True, stdout=subprocess.DEVNULL)
        lib = os.path.join(tmp, "libjavalzo.so")
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-fwrapv", "-fno-strict-aliasing", "-w", "-I", os.path.join(ROOT, "oracle", "ref"), "-I", tmp, "-shared", "-o", lib,
                        os.path.join(here, "shim.cpp")], check=True)
        self.lib = ctypes.CDLL(lib)
        self.lib.lzo_java_compress.restype = ctypes.c_longlong
        self.lib.lzo_java_decompress.restype = ctypes.c_longlong

    def compress(self, data):
        cap = ref.max_compressed_length(len(data))
        out = ctypes.create_string_buffer(cap + 8)
        n = self.lib.lzo_java_compress(bytes(data), ctypes.c_longlong(len(data)), out, ctypes.c_longlong(cap))
        assert n >= 0, n
        return out.raw[:n]

    def decompress(self, stream, capacity):
        """-> ("ok", plaintext) or ("malformed", offset)"""
        out = ctypes.create_string_buffer(capacity + 8)
        eo = ctypes.c_longlong(0)
        n = self.lib.lzo_java_decompress(bytes(stream), ctypes.c_longlong(len(stream)), out, ctypes.c_longlong(capacity), ctypes.byref(eo))
        assert n >= -1, n
        return ("ok", out.raw[:n]) if n >= 0 else ("malformed", eo.value)


def digest(data):
    """the first 16 hex digits of the SHA-256"""
    return hashlib.sha256(data).hexdigest()[:16]


def java_verdict(verdict):
    """one short string per outcome: "ok <length> <the first 16 hex digits of the plaintext's SHA-256>" or "malformed <offset>" (tests/test_lzo_ref.py builds the same from the model)"""
    return "ok %d %s" % (len(verdict[1]), digest(verdict[1])) if verdict[0] == "ok" else "malformed %d" % verdict[1]


def write(recorded, path):
    """one vector, one decode outcome per line"""
    with open(path, "w") as f:
        f.write('{"liblzo2_version": %s,\n"vectors": {\n' % json.dumps(recorded["liblzo2_version"]))
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True, separators=(",", ":"))) for k, v in sorted(recorded["vectors"].items())))
        f.write('\n},\n"java_decode": {\n')
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(recorded["java_decode"].items())))
        f.write("\n}}\n")


def stream_entry(stream):
    return {"hex": stream.hex()} if len(stream) <= HEX_LIMIT else {"length": len(stream), "sha256": digest(stream)}


def vectors(tmp):
    lzo = Liblzo2()
    java = JavaLzo(tmp)
    out = {}
    for label, data in cases.vector_inputs():
        model = ref.compress(data)
        e = {"input_length": len(data), "input_sha256": digest(data),
             "model": {"length": len(model), "sha256": digest(model), "liblzo2_restores": len(data) == 0 or lzo.decompress(model, len(data)) == data}}
        theirs = java.compress(data)
        e["java"] = {"length": len(theirs), "sha256": digest(theirs)}
        if len(data):  # (liblzo2's encoders are not asked about nothing)
            for level in (1, 999):
                stream = lzo.compress(data, level)
                assert ref.decompress(stream, len(data)) == data, (label, level)  # (every stream is checked here; the file keeps the short ones)
                same = level == 999 and stream_entry(stream) == e["lzo1x_1"]  # (incompressible plaintexts: both levels write the same literal run)
                e["lzo1x_%d" % level] = {"same_as": "lzo1x_1"} if same else stream_entry(stream)
        assert label not in out, label
        out[label] = e
    decode = {}
    for case in cases.decode_cases() + [cases.long_run_case()]:
        for cap, _ in cases.runs(case):
            verdict = java.decompress(case[1], cap)
            decode["%s @ %d" % (case[0], cap)] = java_verdict(verdict)
    return {"liblzo2_version": lzo.version, "vectors": out, "java_decode": decode}


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        recorded = vectors(tmp)
    write(recorded, PATH)
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))
