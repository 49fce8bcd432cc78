"""Writes tests/golden/xxh3_vectors.json: XXH3-64 and XXH3-128 of the xxHash sanity buffer (TestXxHash3.java's createSanityBuffer:
buffer[i] = top byte of g, g = PRIME32 * PRIME64^i) over every length class boundary and four seeds, plus the known answers of
TestXxHash3.java itself.

The hashes are recorded from the reference's bundled libxxhash (src/main/resources/aircompressor/linux-amd64/libxxhash.so) when it is
there, else from the first XXH3 implementation found (the system libxxhash, the Python `xxhash` module); every other implementation on
the machine must agree on every entry, or nothing is written.

    python tools/record_xxh3_vectors.py [--reference DIR] [--out PATH]
"""
import argparse
import ctypes
import ctypes.util
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
PRIME32 = 2654435761            # TestXxHash3.java: a long, not sign-extended
PRIME64 = 0x9E3779B185EBCA8D
SEEDS = [0, PRIME32, PRIME64, M64]
LENGTHS = (list(range(260)) + [1024 * k + d for k in (1, 2, 3, 4) for d in (-65, -64, -63, -1, 0, 1, 63, 64, 65)]
           + [65535, 65536, 65537, 1 << 20, (1 << 20) + 7])


def sanity_buffer(n):
    out = bytearray(n)
    g = PRIME32
    for i in range(n):
        out[i] = g >> 56
        g = (g * PRIME64) & M64
    return bytes(out)


class XXH128(ctypes.Structure):
    _fields_ = [("low64", ctypes.c_uint64), ("high64", ctypes.c_uint64)]


def from_library(path):
    lib = ctypes.CDLL(path)
    lib.XXH3_64bits_withSeed.restype = ctypes.c_uint64
    lib.XXH3_64bits_withSeed.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64]
    lib.XXH3_128bits_withSeed.restype = XXH128
    lib.XXH3_128bits_withSeed.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64]
    version = lib.XXH_versionNumber() if hasattr(lib, "XXH_versionNumber") else 0
    h64 = lambda d, s: lib.XXH3_64bits_withSeed(d, len(d), s)  # noqa: E731

    def h128(d, s):
        r = lib.XXH3_128bits_withSeed(d, len(d), s)
        return r.low64, r.high64
    return "%s (%d)" % (path, version), h64, h128


def implementations(reference):
    found = []
    bundled = os.path.join(reference, "src", "main", "resources", "aircompressor", "linux-amd64", "libxxhash.so")
    if os.path.exists(bundled):
        found.append(from_library(bundled))
    system = ctypes.util.find_library("xxhash")
    if system:
        found.append(from_library(system))
    try:
        import xxhash
        found.append(("python xxhash %s" % xxhash.XXHASH_VERSION, xxhash.xxh3_64_intdigest,
                      lambda d, s: (xxhash.xxh3_128_intdigest(d, s) & M64, xxhash.xxh3_128_intdigest(d, s) >> 64)))
    except ImportError:
        pass
    return found


def java_known_answers(reference):
    """the assertions of TestXxHash3.java: [kind, length, seed, low (, high)] with the sanity buffer (length 0: the empty input)"""
    path = os.path.join(reference, "src", "test", "java", "io", "airlift", "compress", "v3", "xxhash", "TestXxHash3.java")
    text = open(path).read()
    names = {"0": 0, "PRIME32": PRIME32, "PRIME64": PRIME64}
    kats = [["64", 0, 0, int(re.search(r"EMPTY_64 = 0x([0-9A-F]+)L", text).group(1), 16)]]
    m = re.search(r"EMPTY_128 = new XxHash128\(0x([0-9A-F]+)L, 0x([0-9A-F]+)L\)", text)
    kats.append(["128", 0, 0, int(m.group(1), 16), int(m.group(2), 16)])
    m = re.search(r"hash\(empty, PRIME64\)\)\.isEqualTo\(0x([0-9A-F]+)L\)", text)
    kats.append(["64", 0, PRIME64, int(m.group(1), 16)])
    m = re.search(r"expected = new XxHash128\(0x([0-9A-F]+)L, 0x([0-9A-F]+)L\);\s*assertThat\(XxHash3Native\.hash128\(empty, PRIME32\)\)", text)
    kats.append(["128", 0, PRIME32, int(m.group(1), 16), int(m.group(2), 16)])
    for n, seed, v in re.findall(r"assertSanityHash64\((\d+), (\w+), 0x([0-9A-F]+)L\);", text):
        kats.append(["64", int(n), names[seed], int(v, 16)])
    for n, seed, lo, hi in re.findall(r"assertSanityHash128\((\d+), (\w+), 0x([0-9A-F]+)L, 0x([0-9A-F]+)L\);", text):
        kats.append(["128", int(n), names[seed], int(lo, 16), int(hi, 16)])
    return kats


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "xxh3_vectors.json"))
    args = ap.parse_args()
    impls = implementations(args.reference)
    if not impls:
        sys.exit("no XXH3 implementation on this machine")
    buf = sanity_buffer(max(LENGTHS))
    rows64, rows128 = [], []
    for n in LENGTHS:
        d = buf[:n]
        r64 = [[f64(d, s) for s in SEEDS] for _, f64, _ in impls]
        r128 = [[f128(d, s) for s in SEEDS] for _, _, f128 in impls]
        for (name, _, _), a, b in zip(impls[1:], r64[1:], r128[1:]):
            if a != r64[0] or b != r128[0]:
                sys.exit("%s disagrees with %s at length %d: nothing written" % (name, impls[0][0], n))
        rows64.append(["%016x" % v for v in r64[0]])
        rows128.append(["%016x%016x" % (hi, lo) for lo, hi in r128[0]])
    kats = java_known_answers(args.reference)
    for kat in kats:  # the recording implementation must reproduce the reference's own assertions
        d, s = buf[:kat[1]], kat[2]
        got = [impls[0][1](d, s)] if kat[0] == "64" else list(impls[0][2](d, s))
        if got != kat[3:]:
            sys.exit("%s does not reproduce TestXxHash3.java's %r: nothing written" % (impls[0][0], kat))
    doc = {
        "about": "XXH3-64 / XXH3-128 of the xxHash sanity buffer (TestXxHash3.java createSanityBuffer) by length and seed; recorded by "
                 "tools/record_xxh3_vectors.py",
        "recorded_from": os.path.basename(impls[0][0]),
        "agreeing": [os.path.basename(name) for name, _, _ in impls[1:]],
        "seeds": ["%016x" % s for s in SEEDS],
        "lengths": LENGTHS,
        "xxh3_64": rows64,
        "xxh3_128_high_low": rows128,
        "java_known_answers": [[k[0], k[1], "%016x" % k[2]] + ["%016x" % v for v in k[3:]] for k in kats],
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d lengths x %d seeds, %d known answers; %s, agreeing: %s" % (args.out, len(LENGTHS), len(SEEDS), len(kats), impls[0][0],
                                                                               ", ".join(n for n, _, _ in impls[1:])))


if __name__ == "__main__":
    main()
