"""GPU tests of the streaming hashers (xxhash_stream.hip) through the C ABI and the Python twins.  The scheme and the plans are in
tests/xxh_stream_cases.py: state i owns a plaintext and cut points, round r updates every state with its r-th piece in one call, and after
every round every state's digest must EQUAL the one-shot reference (tests/xxh3_ref.py; the oracle's xxh64 / xxh32) of the prefix absorbed so
far -- so every test also shows that digest leaves the state alone.  The shapes are the smallest at which each mechanism can break."""
import ctypes
import struct

import numpy as np
import pytest

from tests import common
from tests import xxh_stream_cases as C

pytestmark = pytest.mark.gpu
M64 = C.M64
ALGO = pytest.mark.parametrize("algo", C.ALGOS, ids=C.ALGO_NAMES)


class GpuBackend(C.Backend):
    def __init__(self, lib, ctx):
        self.lib, self.ctx = lib, ctx

    def alloc(self, nbytes):
        return self.lib.achip_device_alloc(self.ctx, nbytes)

    def free(self, p):
        assert self.lib.achip_device_free(self.ctx, p) == 0

    def h2d(self, p, array):
        array = np.ascontiguousarray(array)
        assert self.lib.achip_memcpy_h2d(self.ctx, p, array.ctypes.data, array.nbytes) == 0
        assert self.lib.achip_ctx_synchronize(self.ctx) == 0  # (the host array may go away)

    def d2h(self, array, p):
        assert self.lib.achip_memcpy_d2h(self.ctx, array.ctypes.data, p, array.nbytes) == 0
        assert self.lib.achip_ctx_synchronize(self.ctx) == 0

    def state_size(self, algo):
        return self.lib.achip_hash_state_size(algo)

    def reset(self, algo, states, n, seed):
        assert self.lib.achip_hash_states_reset(self.ctx, algo, states, n, ctypes.c_int64(seed if seed < (1 << 63) else seed - (1 << 64))) == 0

    def update(self, algo, states, src, off, ln, n):
        assert self.lib.achip_hash_states_update(self.ctx, algo, states, src, off, ln, n) == 0

    def digest(self, algo, states, out, n):
        assert self.lib.achip_hash_states_digest(self.ctx, algo, states, out, n) == 0


@pytest.fixture(scope="module")
def gb():
    from tests.gpu_harness import GpuBatch
    return GpuBatch(0)


@pytest.fixture(scope="module")
def be(gb):
    return GpuBackend(gb.codec.lib, gb.codec.native.ctx)


@ALGO
def test_every_total_and_first_cut(be, algo):
    # 1: totals 0..600 cut once at every listed position <= total, five seeds, every plaintext at its own odd offset from a misaligned base
    plan = C.small_plan()
    assert len(plan) == 11879
    for seed in C.SEEDS:
        bad = C.run_plan(be, algo, plan, seed, packed=True, misalign=seed & 7)
        assert not bad, (seed, [(plan[i], r, a) for i, r, a in bad[:10]])


@ALGO
def test_block_boundaries_of_the_stream(be, algo):
    # 2: totals 1024 k + d; pieces that end one before, at and one after a multiple of 64 and of 1024; long pieces that start at 1, 63, 64, 65,
    # 960, 1023, 1024, 1025 of the stream (the partial block at the front of a wavefront's piece)
    plan = C.boundary_plan()
    assert len(plan) == 6354
    bad = C.run_plan(be, algo, plan, 0x9E3779B185EBCA8D)
    assert not bad, [(plan[i], r, a) for i, r, a in bad[:10]]


@ALGO
@pytest.mark.parametrize("sizes", [(1,), (1, 2, 3, 4, 5, 6, 7)], ids=["bytes", "rotation"])
def test_dribble(be, algo, sizes):
    # 3: 700 updates of one byte (of 1..7 bytes in rotation) into one state, a digest after each
    plan = C.dribble_plan(700, sizes)
    assert len(plan[0][2]) == 699
    bad = C.run_plan(be, algo, plan, 7)
    assert not bad, bad[:10]


@ALGO
def test_many_rounds_of_uneven_pieces(be, algo):
    # 4: 2 000 states, totals from UNEVEN_TOTALS, 1..9 random cuts: short and long pieces in the same call, every state digested every round
    plan = C.uneven_plan(2000, 3)
    bad = C.run_plan(be, algo, plan, -7)
    assert not bad, [(plan[i], r, a) for i, r, a in bad[:10]]


@ALGO
def test_uneven_pieces_where_a_wavefront_looks_after_several_states(be, algo):
    # 4, at 20 000 states, digested after the last round only
    plan = C.uneven_plan(20000, 4)
    bad = C.run_plan(be, algo, plan, -7, digest_every_round=False)
    assert not bad, [(plan[i], r, a) for i, r, a in bad[:10]]


@ALGO
def test_seeds_per_sub_range(be, algo):
    # 5: halves of one array reset with different seeds and updated in one call; reset of a used state gives a fresh hasher; XXH32 takes the
    # seed's low 32 bits
    bad, total = C.seeds_per_half(be, algo)
    assert total == 80 and bad == 0


def signed(v, bits=64):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def as_twin(algo, ref):
    """the reference value as the Python twins return it: signed long, signed int, XxHash128 of signed longs"""
    if algo == C.XXH3_128:
        return (signed(ref[0]), signed(ref[1]))
    return signed(ref, 32) if algo == C.XXH32 else signed(ref)


def corpus_bytes():
    return b"".join(d for _, d, _ in common.corpus_sample()[:3])


PIECES = (0, 1, 3, 240, 241, 4096, 70001)


@ALGO
def test_host_hasher_of_the_c_abi(gb, algo):
    # 6: achip_hasher_* over corpus bytes in pieces (0, 1, 3, 240, 241, 4096, 70 001, rest); digest mid-stream and twice; reset; one update larger
    # than the staging chunk (1 MiB)
    lib, ctx = gb.codec.lib, gb.codec.native.ctx
    data = corpus_bytes()
    view = np.frombuffer(data, dtype=np.uint8)
    out = (ctypes.c_int64 * 2)()

    def digest(h):
        assert lib.achip_hasher_digest(h, out) == 0
        u = (int(out[0]) & M64, int(out[1]) & M64)
        return u if algo == C.XXH3_128 else u[0]

    for seed in (0, -1, 2654435761):
        h = lib.achip_hasher_create(ctx, algo, ctypes.c_int64(seed))
        assert h
        pos = 0
        for n in PIECES + (len(data) - sum(PIECES),):
            assert lib.achip_hasher_update(h, view[pos:].ctypes.data if n else None, n) == 0
            pos += n
            want = C.reference_of(algo, data[:pos], seed)
            assert digest(h) == want and digest(h) == want, (seed, pos)
        assert pos == len(data)
        assert lib.achip_hasher_reset(h, ctypes.c_int64(seed + 1)) == 0
        assert digest(h) == C.reference_of(algo, b"", seed + 1)
        big = np.frombuffer((data * 8)[:(1 << 20) + 70001], dtype=np.uint8)
        assert lib.achip_hasher_update(h, big.ctypes.data, big.size) == 0
        assert digest(h) == C.reference_of(algo, big.tobytes(), seed + 1)
        assert lib.achip_hasher_update(h, None, -1) < 0
        assert lib.achip_hasher_destroy(h) == 0


@ALGO
def test_python_streaming_twins(gb, algo):
    # 6: the four streaming objects: pieces, update_le_long / update_le_int, digest twice and mid-stream, reset, context manager, use after close
    import aircompressor_amd as A
    make = [A.XxHash32HipHasher.create, A.XxHash64HipHasher.create, A.XxHash3HipHasher.new_hasher, A.XxHash3HipHasher.new_hasher128][algo]
    data = corpus_bytes()
    for seed in (0, -1, 0x9E3779B185EBCA87):
        with make(seed, native_ctx=gb.codec.native) as h:
            pos = 0
            for n in PIECES + (len(data) - sum(PIECES),):
                assert h.update(data, pos, n) is h
                pos += n
                want = as_twin(algo, C.reference_of(algo, data[:pos], seed))
                assert h.digest() == want and h.digest() == want, (seed, pos)
            if algo == C.XXH3_128:
                assert isinstance(h.digest(), A.XxHash128)
            # after reset(seed) the object equals a fresh one; updateLE equals update of the packed little-endian bytes
            assert h.reset(seed ^ 5) is h
            assert h.digest() == as_twin(algo, C.reference_of(algo, b"", seed ^ 5))
            assert h.update_le_long(-2).update_le_int(0x80000001).update_le_long(0x0102030405060708).update(b"xyz") is h
            packed = struct.pack("<qIq", -2, 0x80000001, 0x0102030405060708) + b"xyz"
            assert h.digest() == as_twin(algo, C.reference_of(algo, packed, seed ^ 5))
            with make(seed ^ 5, native_ctx=gb.codec.native) as fresh:
                assert fresh.update(packed).digest() == h.digest()
            assert h.reset().update(b"abc").digest() == as_twin(algo, C.reference_of(algo, b"abc", 0))  # (the default seed)
            with pytest.raises(IndexError):
                h.update(b"abc", 2, 5)
        with pytest.raises(RuntimeError):
            h.update(b"x")
        with pytest.raises(RuntimeError):
            h.digest()
        with pytest.raises(RuntimeError):
            h.reset()
        h.close()  # (closing twice is fine, as in the reference)
    big = (data * 8)[:(1 << 20) + 70001]  # one update larger than the staging chunk
    with make(3, native_ctx=gb.codec.native) as h:
        assert h.update(big).digest() == as_twin(algo, C.reference_of(algo, big, 3))


def test_hip_hash_states_object(gb):
    import aircompressor_amd as A
    lib, ctx = gb.codec.lib, gb.codec.native.ctx
    be = GpuBackend(lib, ctx)
    data = np.frombuffer(C.data(), dtype=np.uint8)
    n = 5
    src, off, ln, out = be.to_device(data), be.to_device(np.arange(n, dtype=np.int64) * 300), be.to_device(np.array([0, 1, 240, 300, 299], dtype=np.int32)), be.alloc(16 * n)
    for algo in C.ALGOS:
        with A.HipHashStates(algo, n, native_ctx=gb.codec.native) as st:
            assert st.reset(9).update(src, off, ln).update(src, off, ln) is st
            st.reset(10, 1, 2)
            st.update(src, off, ln)
            st.digest(out)
            got = np.zeros(2 * n, dtype=np.int64)
            be.d2h(got, out)
            for i, m in enumerate([0, 1, 240, 300, 299]):
                piece = C.data()[300 * i:300 * i + m]
                want = C.reference_of(algo, piece if i in (1, 2) else piece * 3, 10 if i in (1, 2) else 9)
                g = (int(got[2 * i]) & M64, int(got[2 * i + 1]) & M64) if algo == C.XXH3_128 else int(got[i]) & M64
                assert g == want, (algo, i)
            with pytest.raises(IndexError):
                st.reset(0, 3, 3)
    for p in (src, off, ln, out):
        be.free(p)


def test_argument_checks_with_a_context(gb):
    lib, ctx = gb.codec.lib, gb.codec.native.ctx
    p = lib.achip_device_alloc(ctx, 4096)
    cls = lib.achip_status_class
    want = cls(lib.achip_xxhash64_batch(ctx, p, None, p, 0, p, 1))
    assert want == 3
    for algo in C.ALGOS:
        assert cls(lib.achip_hash_states_reset(ctx, algo, None, 1, 0)) == want
        assert cls(lib.achip_hash_states_update(ctx, algo, None, p, p, p, 1)) == want
        assert cls(lib.achip_hash_states_update(ctx, algo, p, p, None, p, 1)) == want
        assert cls(lib.achip_hash_states_update(ctx, algo, p, p, p, None, 1)) == want
        assert cls(lib.achip_hash_states_digest(ctx, algo, None, p, 1)) == want
        assert cls(lib.achip_hash_states_digest(ctx, algo, p, None, 1)) == want
        assert cls(lib.achip_hash_states_reset(ctx, algo, p, -1, 0)) == want
        # nStates == 0 launches nothing and succeeds, whatever the arrays
        assert lib.achip_hash_states_reset(ctx, algo, None, 0, 0) == 0
        assert lib.achip_hash_states_update(ctx, algo, None, None, None, None, 0) == 0
        assert lib.achip_hash_states_digest(ctx, algo, None, None, 0) == 0
    assert cls(lib.achip_hash_states_reset(ctx, 4, p, 1, 0)) == 3
    assert lib.achip_device_free(ctx, p) == 0


def one_shot_batch(lib, ctx, be, algo, dsrc, n_blocks, size, seed):
    """the one-shot batch kernels on n_blocks buffers of `size` bytes at dsrc -> unsigned ints or (low, high) pairs"""
    off, ln = be.to_device(np.arange(n_blocks, dtype=np.int64) * size), be.to_device(np.full(n_blocks, size, dtype=np.int32))
    out = be.alloc(16 * n_blocks)
    if algo == C.XXH32:
        got = np.zeros(n_blocks, dtype=np.int32)
        assert lib.achip_xxhash32_batch(ctx, dsrc, off, ln, ctypes.c_int32(signed(seed, 32)), out, n_blocks) == 0
    else:
        got = np.zeros(n_blocks * (2 if algo == C.XXH3_128 else 1), dtype=np.int64)
        fn = {C.XXH64: lib.achip_xxhash64_batch, C.XXH3_64: lib.achip_xxhash3_64_batch, C.XXH3_128: lib.achip_xxhash3_128_batch}[algo]
        assert fn(ctx, dsrc, off, ln, ctypes.c_int64(signed(seed)), out, n_blocks) == 0
    be.d2h(got, out)
    for p in (off, ln, out):
        be.free(p)
    if algo == C.XXH32:
        return [int(v) & 0xFFFFFFFF for v in got]
    u = [int(v) & M64 for v in got]
    return [(u[2 * i], u[2 * i + 1]) for i in range(n_blocks)] if algo == C.XXH3_128 else u


@ALGO
def test_equal_to_the_one_shot_kernels_at_size(gb, be, algo):
    # 7: 16 384 states, each fed a 64 KiB corpus block in three unequal pieces (1 000 / 40 000 / rest), offsets into 8 distinct blocks: every
    # state equals the one-shot batch kernel's hash of the whole block, computed in the same process
    lib, ctx = gb.codec.lib, gb.codec.native.ctx
    blocks = [d for _, d, _ in common.corpus_sample()][:8]
    assert len(blocks) == 8 and all(len(b) == 65536 for b in blocks)
    src = np.frombuffer(b"".join(blocks), dtype=np.uint8)
    seed = 0x9E3779B185EBCA8D
    dsrc = be.to_device(src)
    want = one_shot_batch(lib, ctx, be, algo, dsrc, 8, 65536, seed)
    be.free(dsrc)
    assert want[0] == C.reference_of(algo, blocks[0], seed)  # (and the one-shot kernels equal the reference)
    plan = C.three_piece_plan(16384)
    assert plan[9] == (65536, 65536, [1000, 41000])
    bad = C.run_plan(be, algo, plan, seed, digest_every_round=False, src=src, want=lambda i, absorbed: want[i % 8])
    assert not bad, bad[:10]
