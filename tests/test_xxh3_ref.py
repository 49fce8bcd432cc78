"""XXH3 without a GPU: the pure-Python reference (tests/xxh3_ref.py) that the GPU tests check the kernels against is pinned to the
recorded vectors (tests/golden/xxh3_vectors.json, tools/record_xxh3_vectors.py: the sanity buffer of TestXxHash3.java at every
length class boundary and four seeds, and TestXxHash3.java's own known answers) and to whatever XXH3 implementation this machine has;
the Python / C surface of XxHash3HipHasher refuses bad arguments the way achip_xxhash64 does and fails loudly without a GPU."""
import ctypes
import ctypes.util
import json
import os

import numpy as np
import pytest

from tests import xxh3_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "xxh3_vectors.json")) as f:
        return json.load(f)


def sanity_buffer(n):
    # TestXxHash3.java createSanityBuffer: buffer[i] = top byte of PRIME32 * PRIME64^i
    out = bytearray(n)
    g = 2654435761
    for i in range(n):
        out[i] = g >> 56
        g = (g * 0x9E3779B185EBCA8D) & M64
    return bytes(out)


def test_reference_equals_the_recorded_vectors(vectors):
    seeds = [int(s, 16) for s in vectors["seeds"]]
    buf = sanity_buffer(max(vectors["lengths"]))
    assert len(vectors["lengths"]) * len(seeds) == 1204
    for n, row64, row128 in zip(vectors["lengths"], vectors["xxh3_64"], vectors["xxh3_128_high_low"]):
        d = buf[:n]
        for seed, want64, want128 in zip(seeds, row64, row128):
            assert xxh3_ref.xxh3_64(d, seed) == int(want64, 16), (n, seed)
            lo, hi = xxh3_ref.xxh3_128(d, seed)
            assert (hi << 64) | lo == int(want128, 16), (n, seed)


def test_reference_equals_the_java_known_answers(vectors):
    kats = vectors["java_known_answers"]
    assert len(kats) >= 30
    buf = sanity_buffer(256)
    for kind, n, seed, *want in kats:
        d, s = buf[:n], int(seed, 16)
        got = [xxh3_ref.xxh3_64(d, s)] if kind == "64" else list(xxh3_ref.xxh3_128(d, s))
        assert got == [int(w, 16) for w in want], (kind, n, seed)
    # as the reference's test states them
    assert xxh3_ref.xxh3_64(b"") == 0x2D06800538D394C2
    assert xxh3_ref.xxh3_64(buf[:195], 0x9E3779B185EBCA8D) == 0xBA68003D370CB3D9
    assert xxh3_ref.xxh3_128(b"") == (0x6001C324468D497F, 0x99AA06D3014798D8)


BOUNDARY_LENGTHS = sorted(set([0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192,
                               239, 240, 241, 255, 256, 257, 319, 320, 959, 960, 1023, 1024, 1025, 1087, 1088, 2047, 2048, 2049, 4095, 4096,
                               4097, 65536 + 13, 200000]))
SEEDS = [0, 1, -1, 2654435761, 0x9E3779B185EBCA87, -2**63]


def _system_library():
    name = ctypes.util.find_library("xxhash")
    if not name:
        return None
    try:
        lib = ctypes.CDLL(name)
        lib.XXH3_64bits_withSeed
        lib.XXH3_128bits_withSeed
    except (OSError, AttributeError):
        return None

    class H128(ctypes.Structure):
        _fields_ = [("low64", ctypes.c_uint64), ("high64", ctypes.c_uint64)]
    lib.XXH3_64bits_withSeed.restype = ctypes.c_uint64
    lib.XXH3_64bits_withSeed.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64]
    lib.XXH3_128bits_withSeed.restype = H128
    lib.XXH3_128bits_withSeed.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64]
    return lib


def random_cases():
    rng = np.random.default_rng(23)
    data = rng.integers(0, 256, 200000 + 64, dtype=np.uint8).tobytes()
    return [(data[k % 7:k % 7 + n], SEEDS[k % len(SEEDS)]) for k, n in enumerate(BOUNDARY_LENGTHS)]


def test_reference_equals_libxxhash_on_random_data():
    lib = _system_library()
    if lib is None:
        pytest.skip("no libxxhash on this machine")
    for d, seed in random_cases():
        s = seed & M64
        assert xxh3_ref.xxh3_64(d, seed) == lib.XXH3_64bits_withSeed(d, len(d), s), (len(d), seed)
        r = lib.XXH3_128bits_withSeed(d, len(d), s)
        assert xxh3_ref.xxh3_128(d, seed) == (r.low64, r.high64), (len(d), seed)


def test_reference_equals_the_xxhash_module_on_random_data():
    xxhash = pytest.importorskip("xxhash")
    for d, seed in random_cases():
        s = seed & M64
        assert xxh3_ref.xxh3_64(d, seed) == xxhash.xxh3_64_intdigest(d, s), (len(d), seed)
        h = xxhash.xxh3_128_intdigest(d, s)
        assert xxh3_ref.xxh3_128(d, seed) == (h & M64, h >> 64), (len(d), seed)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library()
    import aircompressor_amd as A
    return A.load_library()


def test_hasher_without_gpu_raises_or_runs(lib):
    import aircompressor_amd as A
    if lib.achip_device_count() > 0:
        h = A.XxHash3HipHasher()  # (a GPU is visible: the hasher comes up; test_gpu_xxhash3.py checks what it computes)
        assert h.hash128(b"") == A.XxHash128(0x6001C324468D497F, 0x99AA06D3014798D8 - (1 << 64))
        return
    with pytest.raises(A.HipUnavailableError):
        A.XxHash3HipHasher()


def test_xxhash128_is_a_record_of_signed_longs():
    import aircompressor_amd as A
    h = A.XxHash128(1, -2)
    assert (h.low, h.high) == (1, -2) and h == (1, -2) and A.XxHash128._fields == ("low", "high")


def bad_calls(ctx, buf, out):
    """argument combinations achip_xxhash64[_batch] refuses: (name, single-call args, batch args)"""
    p = ctypes.c_void_p
    return [
        ("null ctx", (None, buf, 4, 0, out), (None, buf, p(1), p(1), 0, out, 1)),
        ("null out", (ctx, buf, 4, 0, None), (ctx, buf, p(1), p(1), 0, None, 1)),
        ("length < 0", (ctx, buf, -1, 0, out), None),
        ("length > 2^31 - 1", (ctx, buf, 1 << 31, 0, out), None),
        ("null src", (ctx, None, 4, 0, out), None),
        ("nBuffers < 0", None, (ctx, buf, p(1), p(1), 0, out, -1)),
        ("null offsets", None, (ctx, buf, None, p(1), 0, out, 1)),
        ("null lengths", None, (ctx, buf, p(1), None, 0, out, 1)),
    ]


def check_argument_statuses(lib, ctx):
    buf = (ctypes.c_uint8 * 8)()
    out = (ctypes.c_int64 * 2)()
    for name, single, batch in bad_calls(ctx, buf, out):
        if single is not None:
            want = lib.achip_xxhash64(*single)
            assert want < 0, name
            for fn in (lib.achip_xxhash3_64, lib.achip_xxhash3_128):
                got = fn(*single)
                assert got < 0 and lib.achip_status_class(got) == lib.achip_status_class(want), name
        if batch is not None:
            want = lib.achip_xxhash64_batch(*batch)
            assert want < 0, name
            for fn in (lib.achip_xxhash3_64_batch, lib.achip_xxhash3_128_batch):
                got = fn(*batch)
                assert got < 0 and lib.achip_status_class(got) == lib.achip_status_class(want), name


def test_argument_checks_match_xxhash64(lib):
    # without a GPU there is no context: every call is refused before it would stage or launch (null ctx first, as in achip_xxhash64)
    check_argument_statuses(lib, None)
    # nBuffers == 0 succeeds without a launch (with a null context it is refused, as achip_xxhash64_batch refuses it)
    assert lib.achip_status_class(lib.achip_xxhash3_64_batch(None, None, None, None, 0, None, 0)) == \
        lib.achip_status_class(lib.achip_xxhash64_batch(None, None, None, None, 0, None, 0))
