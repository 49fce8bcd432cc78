"""GPU parity tests for the batched XXH3-64 / XXH3-128 kernels (xxhash3.hip) through the C ABI: equal to the recorded vectors
(tests/golden/xxh3_vectors.json) on the sanity buffer and to the pure-Python reference (tests/xxh3_ref.py) on random data at every
length class boundary, several seeds, misaligned buffers, mixed batches and full size; the single-call host API and the Python
twins give the same results."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import common, xxh3_ref
from tests.test_xxh3_ref import check_argument_statuses, sanity_buffer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
SEEDS = [0, 1, -1, 2654435761, 0x9E3779B185EBCA87]


@pytest.fixture(scope="module")
def gb():
    from tests.gpu_harness import GpuBatch
    return GpuBatch(0)


def run_batch(gb, wide, buffers, seed, misalign=3):
    """hashes of `buffers` (packed at odd offsets from a misaligned base) -> unsigned ints, or (low, high) pairs when wide"""
    lib, ctx = gb.codec.lib, gb.codec.native.ctx
    n = len(buffers)
    offs, pos = [], misalign
    for b in buffers:
        offs.append(pos)
        pos += len(b) + (len(b) % 7) + 1
    src = np.zeros(pos + 64, dtype=np.uint8)
    for b, so in zip(buffers, offs):
        src[so:so + len(b)] = np.frombuffer(b, dtype=np.uint8)
    so = np.array(offs, dtype=np.int64)
    sl = np.array([len(b) for b in buffers], dtype=np.int32)
    out = np.zeros(n * (2 if wide else 1), dtype=np.int64)
    d = [lib.achip_device_alloc(ctx, a.nbytes + 64) for a in (src, so, sl, out)]
    assert all(d)
    for dp, a in zip(d[:3], (src, so, sl)):
        assert lib.achip_memcpy_h2d(ctx, dp, a.ctypes.data, a.nbytes) == 0
    fn = lib.achip_xxhash3_128_batch if wide else lib.achip_xxhash3_64_batch
    assert fn(ctx, d[0], d[1], d[2], ctypes.c_int64(seed), d[3], n) == 0
    assert lib.achip_memcpy_d2h(ctx, out.ctypes.data, d[3], out.nbytes) == 0
    assert lib.achip_ctx_synchronize(ctx) == 0
    for dp in d:
        lib.achip_device_free(ctx, dp)
    u = [int(v) & M64 for v in out]
    return [(u[2 * i], u[2 * i + 1]) for i in range(n)] if wide else u


def ref(wide, b, seed):
    return xxh3_ref.xxh3_128(b, seed) if wide else xxh3_ref.xxh3_64(b, seed)


@pytest.mark.parametrize("wide", [False, True], ids=["xxh3_64", "xxh3_128"])
def test_recorded_vectors(gb, wide):
    with open(os.path.join(ROOT, "tests", "golden", "xxh3_vectors.json")) as f:
        v = json.load(f)
    buf = sanity_buffer(max(v["lengths"]))
    buffers = [buf[:n] for n in v["lengths"]]
    for k, seed in enumerate(int(s, 16) for s in v["seeds"]):
        got = run_batch(gb, wide, buffers, seed)
        for n, row64, row128, g in zip(v["lengths"], v["xxh3_64"], v["xxh3_128_high_low"], got):
            want = int(row128[k], 16) if wide else int(row64[k], 16)
            assert ((g[1] << 64) | g[0] if wide else g) == want, (n, seed)


def lengths_around_boundaries():
    around = [1024 * k + d for k in (1, 2, 3, 4, 64) for d in range(-65, 66)]
    return sorted(set(list(range(0, 2101)) + around + [65535, 65536, 65537, (1 << 20) + 7]))


@pytest.mark.parametrize("wide", [False, True], ids=["xxh3_64", "xxh3_128"])
def test_every_length_and_seed(gb, wide):
    rng = np.random.default_rng(31)
    data = rng.integers(0, 256, (1 << 20) + 64, dtype=np.uint8).tobytes()
    lengths = lengths_around_boundaries()
    buffers = [data[i % 13:i % 13 + n] for i, n in enumerate(lengths)]
    for seed in SEEDS:
        got = run_batch(gb, wide, buffers, seed, misalign=seed & 7)
        bad = [(len(b), seed) for b, g in zip(buffers, got) if g != ref(wide, b, seed)]
        assert not bad, bad[:10]


@pytest.mark.parametrize("wide", [False, True], ids=["xxh3_64", "xxh3_128"])
def test_mixed_batch_interleaves_short_and_long(gb, wide):
    # short and long buffers interleaved, in batches large enough that a long-path wavefront looks after several buffers
    rng = np.random.default_rng(7)
    data = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    seed = -7
    for n in (3, 100, 20000):
        picks = [(int(st), int(m)) for st, m in zip(rng.integers(0, 97, n), rng.choice([0, 5, 16, 100, 240, 241, 1000, 5000, 65536], size=n))]
        got = run_batch(gb, wide, [data[st:st + m] for st, m in picks], seed)
        want = {p: ref(wide, data[p[0]:p[0] + p[1]], seed) for p in set(picks)}
        bad = [(i, p) for i, (p, g) in enumerate(zip(picks, got)) if g != want[p]]
        assert not bad, (n, bad[:10])


def test_negative_length_hashes_as_empty(gb):
    lib, ctx = gb.codec.lib, gb.codec.native.ctx
    so = np.zeros(2, dtype=np.int64)
    sl = np.array([-5, 0], dtype=np.int32)
    out = np.zeros(4, dtype=np.int64)
    d = [lib.achip_device_alloc(ctx, 64) for _ in range(4)]
    assert lib.achip_memcpy_h2d(ctx, d[1], so.ctypes.data, so.nbytes) == 0
    assert lib.achip_memcpy_h2d(ctx, d[2], sl.ctypes.data, sl.nbytes) == 0
    assert lib.achip_xxhash3_128_batch(ctx, d[0], d[1], d[2], ctypes.c_int64(0), d[3], 2) == 0
    assert lib.achip_xxhash3_64_batch(ctx, d[0], d[1], d[2], ctypes.c_int64(0), d[3], 0) == 0  # (no launch)
    assert lib.achip_memcpy_d2h(ctx, out.ctypes.data, d[3], out.nbytes) == 0
    assert lib.achip_ctx_synchronize(ctx) == 0
    for dp in d:
        lib.achip_device_free(ctx, dp)
    assert [int(v) & M64 for v in out] == [0x6001C324468D497F, 0x99AA06D3014798D8] * 2


def test_single_call_host_api_and_python_twins(gb):
    import aircompressor_amd as A
    h = A.XxHash3HipHasher(native_ctx=gb.codec.native)
    data = b"".join(d for _, d, _ in common.corpus_sample()[:3])
    for off, n in ((0, 0), (1, 3), (5, 8), (3, 16), (7, 100), (2, 240), (9, 241), (11, 4096), (13, 70001), (0, len(data))):
        piece = data[off:off + n]
        for seed in (0, -1, 2654435761):
            assert h.hash(data, off, n, seed) & M64 == xxh3_ref.xxh3_64(piece, seed), (off, n, seed)
            lo, hi = h.hash128(data, off, n, seed=seed)
            assert (lo & M64, hi & M64) == xxh3_ref.xxh3_128(piece, seed), (off, n, seed)
            assert isinstance(h.hash128(piece, seed=seed), A.XxHash128)
            # the batch twins give the same values as the single calls
            assert run_batch(gb, False, [piece], seed)[0] == h.hash(piece, seed=seed) & M64
            assert run_batch(gb, True, [piece], seed)[0] == tuple(v & M64 for v in h.hash128(piece, seed=seed))
    assert h.hash(b"") == 0x2D06800538D394C2
    assert h.hash128(b"") == (0x6001C324468D497F, 0x99AA06D3014798D8 - (1 << 64))
    with pytest.raises(IndexError):
        h.hash(b"abc", 2, 5)


def test_argument_checks_with_a_context(gb):
    check_argument_statuses(gb.codec.lib, gb.codec.native.ctx)


@pytest.mark.parametrize("wide", [False, True], ids=["xxh3_64", "xxh3_128"])
def test_full_size_batch(gb, wide):
    """65 536 x 64 KiB buffers (4 GiB hashed) whose offsets point into a handful of distinct corpus blocks: every copy hashes to the
    reference's value"""
    lib, ctx = gb.codec.lib, gb.codec.native.ctx
    blocks = [d for _, d, _ in common.corpus_sample()][:8]
    assert all(len(b) == 65536 for b in blocks)
    n, seed = 65536, 0x9E3779B185EBCA8D
    src = np.frombuffer(b"".join(blocks), dtype=np.uint8)
    so = np.array([65536 * (i % 8) for i in range(n)], dtype=np.int64)
    sl = np.full(n, 65536, dtype=np.int32)
    out = np.zeros(n * (2 if wide else 1), dtype=np.int64)
    d = [lib.achip_device_alloc(ctx, a.nbytes + 64) for a in (src, so, sl, out)]
    assert all(d)
    for dp, a in zip(d[:3], (src, so, sl)):
        assert lib.achip_memcpy_h2d(ctx, dp, a.ctypes.data, a.nbytes) == 0
    fn = lib.achip_xxhash3_128_batch if wide else lib.achip_xxhash3_64_batch
    assert fn(ctx, d[0], d[1], d[2], ctypes.c_int64(seed), d[3], n) == 0
    assert lib.achip_memcpy_d2h(ctx, out.ctypes.data, d[3], out.nbytes) == 0
    assert lib.achip_ctx_synchronize(ctx) == 0
    for dp in d:
        lib.achip_device_free(ctx, dp)
    u = [int(v) & M64 for v in out]
    got = [(u[2 * i], u[2 * i + 1]) for i in range(n)] if wide else u
    want = [ref(wide, b, seed) for b in blocks]
    bad = [i for i, g in enumerate(got) if g != want[i % 8]]
    assert not bad, bad[:10]
