"""The LZ4 encoders with the acceleration of Lz4Compressor.create(acceleration) on the GPU (achip_ctx_set_lz4_acceleration; the `_accel` kernels of lz4_compress.hip):
bytes, lengths, statuses and error offsets against the pure-Python model (tests/lz4_accel_ref.py, pinned by tests/golden/lz4_accel_vectors.json), every output decoded
again by the GPU decoders.  Inputs: tests/lz4_accel_cases.py -- the smallest shapes at which the kernels can go wrong, all of a test's blocks in one batch per
(setting, acceleration).  The value applies to LZ4 block and LZ4 frame encodes of its context and to nothing else: a mixed batch shows both."""
import numpy as np
import pytest

from tests import lz4_accel_cases as cases, lz4_accel_ref as ref
from tests.gpu_harness import GpuBatch

pytestmark = pytest.mark.gpu

LZ4_D, LZ4_C, SNAPPY_D, SNAPPY_C = 0, 1, 2, 3
LZ4F_D, LZ4F_C, LZ4H_D, LZ4H_C = 6, 7, 10, 11
BAD_ARGUMENT = -(3 + 16 * 102)  # INVALID_ARGUMENT / ACHIP_D_BAD_ARGUMENT
DEFAULTS = {"lz4.compress.variant": 4, "lz4.compress.mem_waves": 1, "lz4.compress.tier_min_blocks": 5120, "max_src_len_hint": 0}
# serial probes, batch probes, the window encoder a wavefront per block, and the window encoder through the two-tier kernel with one and two memory wavefronts
SETTINGS = {
    "variant 0": {"lz4.compress.variant": 0},
    "variant 1": {"lz4.compress.variant": 1},
    "variant 4": {"lz4.compress.variant": 4},
    "variant 4, tiers, mem_waves 1": {"lz4.compress.variant": 4, "lz4.compress.tier_min_blocks": 1, "lz4.compress.mem_waves": 1},
    "variant 4, tiers, mem_waves 2": {"lz4.compress.variant": 4, "lz4.compress.tier_min_blocks": 1, "lz4.compress.mem_waves": 2},
}


@pytest.fixture(scope="module")
def gpu():
    return GpuBatch()


@pytest.fixture
def g(gpu):
    """the module's context with every setting these tests touch at its default, before and after"""
    def reset():
        for k, v in DEFAULTS.items():
            gpu.set_option(k, v)
        gpu.codec.native.set_lz4_acceleration(1)
    reset()
    yield gpu
    reset()


def configure(g, setting, acceleration):
    for k, v in SETTINGS[setting].items():
        g.set_option(k, v)
    g.codec.native.set_lz4_acceleration(acceleration)
    assert g.codec.native.get_lz4_acceleration() == acceleration


def lz4_bound(g, n):
    return g.codec.lib.achip_lz4_max_compressed_length(n)


def encode_and_check(g, blocks, want, what):
    """one batch through achip_lz4_compress_batch: outputs, lengths (GpuBatch cuts the outputs at outLen), statuses, error offsets; then the GPU decoder on every output"""
    outs, status, err = g.run(LZ4_C, [d for _, d in blocks], [lz4_bound(g, len(d)) for _, d in blocks], unaligned=True)
    assert status == [0] * len(blocks) and err == [0] * len(blocks), what
    for (name, _), c, w in zip(blocks, outs, want):
        assert len(c) == len(w) and c == w, (what, name, len(c), len(w))
    back, status, _ = g.run(LZ4_D, outs, [len(d) for _, d in blocks])
    assert status == [0] * len(blocks), what
    assert all(b == d for b, (_, d) in zip(back, blocks)), what


@pytest.mark.parametrize("acceleration", cases.ACCELERATIONS)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_blocks_equal_the_model(g, setting, acceleration):
    configure(g, setting, acceleration)
    blocks = cases.block_cases()
    encode_and_check(g, blocks, [cases.expected(name, acceleration) for name, _ in blocks], (setting, acceleration))


@pytest.mark.parametrize("acceleration", cases.LIMIT_ACCELERATIONS)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_a_probe_that_steps_past_the_limit_ends_the_block(g, setting, acceleration):
    configure(g, setting, acceleration)
    blocks = cases.limit_cases(acceleration)
    assert len(blocks) == 3 * acceleration + 21
    encode_and_check(g, blocks, [ref.compress(d, acceleration) for _, d in blocks], (setting, acceleration))


@pytest.mark.parametrize("setting", ["variant 0", "variant 1", "variant 4", "variant 4, tiers, mem_waves 1"])
def test_max_src_len_hint(g, setting):
    """the hint promises blocks of at most 64 KiB, one block is longer: the narrow launch alone runs, the long block gets INVALID_ARGUMENT -- at acceleration 4 as at 1"""
    blocks = [b for b in cases.block_cases() if b[0] in ("alice 64 KiB", "text 70000", "zeros 5000")]
    results = {}
    for acceleration in (1, 4):
        configure(g, setting, acceleration)
        g.set_option("max_src_len_hint", 65536)
        outs, status, err = g.run(LZ4_C, [d for _, d in blocks], [lz4_bound(g, len(d)) for _, d in blocks])
        assert status == [0, BAD_ARGUMENT, 0] and err == [0, 0, 0], (setting, acceleration)
        assert outs == [cases.expected("alice 64 KiB", acceleration), b"", cases.expected("zeros 5000", acceleration)], (setting, acceleration)
        results[acceleration] = status
    assert results[1] == results[4]


@pytest.mark.parametrize("acceleration", cases.FRAME_ACCELERATIONS)
def test_frames_equal_the_python_frame_writer(g, acceleration):
    g.codec.native.set_lz4_acceleration(acceleration)
    frames = cases.frame_cases()
    caps = [g.codec.lib.achip_lz4frame_max_compressed_length(len(d)) for _, d in frames]
    outs, status, err = g.run(LZ4F_C, [d for _, d in frames], caps)
    assert status == [0] * len(frames) and err == [0] * len(frames)
    for (name, d), c in zip(frames, outs):
        w = ref.compress_frame(d, acceleration)
        assert len(c) == len(w) and c == w, (name, acceleration, len(c), len(w))
    assert outs[4][7:11] == (65536 | 0x80000000).to_bytes(4, "little")  # (the random block is stored)
    back, status, _ = g.run(LZ4F_D, outs, [len(d) for _, d in frames])
    assert status == [0] * len(frames) and all(b == d for b, (_, d) in zip(back, frames))


def mixed_items(g):
    """[(op, input, capacity)]: LZ4 block, LZ4 frame, Snappy block and Hadoop LZ4 stream encodes of text, and an LZ4 block decode"""
    lib = g.codec.lib
    text = cases.alice()[:30000]
    packed = ref.compress(text, 1)
    return [(LZ4_C, text, lib.achip_lz4_max_compressed_length(len(text))), (LZ4F_C, text, lib.achip_lz4frame_max_compressed_length(len(text))),
            (SNAPPY_C, text, lib.achip_snappy_max_compressed_length(len(text))), (LZ4H_C, text, lib.achip_hadoop_max_compressed_length(0, len(text), 262144)),
            (LZ4_D, packed, len(text)), (LZ4_C, cases.book()[:20000], lib.achip_lz4_max_compressed_length(20000))]


def test_mixed_batches_take_the_value_for_lz4_and_lz4_frame_only(g):
    plain = GpuBatch()  # a second context, at the default: two contexts hold different values side by side
    g.codec.native.set_lz4_acceleration(4)
    assert (g.codec.native.get_lz4_acceleration(), plain.codec.native.get_lz4_acceleration()) == (4, 1)
    items = mixed_items(g)
    ops, blocks, caps = [i[0] for i in items], [i[1] for i in items], [i[2] for i in items]
    text = blocks[0]
    for run in ("run", "run_host"):  # achip_mixed_batch, achip_mixed_batch_host
        fast, st_fast, _ = getattr(g, run)(ops, blocks, caps)
        slow, st_slow, _ = getattr(plain, run)(ops, blocks, caps)
        assert st_fast == [0] * len(items) and st_slow == [0] * len(items), run
        assert fast[0] == ref.compress(text, 4) and fast[1] == ref.compress_frame(text, 4) and fast[5] == ref.compress(blocks[5], 4), run
        assert slow[0] == ref.compress(text, 1) and slow[1] == ref.compress_frame(text, 1) and slow[5] == ref.compress(blocks[5], 1), run
        assert fast[0] != slow[0] and fast[1] != slow[1], run
        assert fast[2:5] == slow[2:5] and fast[4] == text, run  # Snappy, the Hadoop LZ4 writer and the decoder do not know the value
    # achip_batch_host with ACHIP_OP_LZ4_COMPRESS / ACHIP_OP_LZ4FRAME_COMPRESS
    outs, status, _ = g.run_host(LZ4_C, [text, blocks[5]], [caps[0], caps[5]])
    assert status == [0, 0] and outs == [ref.compress(text, 4), ref.compress(blocks[5], 4)]
    outs, status, _ = g.run_host(LZ4F_C, [text], [caps[1]])
    assert status == [0] and outs == [ref.compress_frame(text, 4)]
    # the Hadoop LZ4 writer, one-shot and in window form, writes what it writes at acceleration 1
    assert g.run(LZ4H_C, [text], [caps[3]])[0] == plain.run(LZ4H_C, [text], [caps[3]])[0]
    A = g.A
    w_fast = g.codec.window_host(A.OP_LZ4HADOOP_COMPRESS, A.native.WINDOW_FIRST | A.native.WINDOW_LAST, text, caps[3], compress=True)
    w_slow = plain.codec.window_host(A.OP_LZ4HADOOP_COMPRESS, A.native.WINDOW_FIRST | A.native.WINDOW_LAST, text, caps[3], compress=True)
    assert w_fast == w_slow and w_fast[0] == len(text) and w_fast[4] == 0 and len(w_fast[1]) > 8


def test_multi_batch_host_each_context_its_own_value(g):
    """achip_multi_batch_host over two contexts with different values: every item is encoded at the value of the context whose slice it fell into"""
    plain = GpuBatch()
    g.codec.native.set_lz4_acceleration(8)
    multi = g.A.HipMultiContextCodec(contexts=[g.codec.native, plain.codec.native])
    text = cases.alice()
    blocks = [text[k * 4000:(k + 1) * 4000 + 2000] for k in range(10)]
    src, src_off, src_len = g.pack(blocks, align=1)
    caps = np.array([lz4_bound(g, len(b)) for b in blocks], dtype=np.int32)
    dst_off = np.concatenate([[0], np.cumsum(caps[:-1])]).astype(np.int64)
    dst = np.zeros(int(caps.sum()) + 16, dtype=np.uint8)
    out_len, status, _ = multi.run_host(LZ4_C, src, src_off, src_len, dst, dst_off, caps)
    assert status.tolist() == [0] * len(blocks)
    starts = multi.slice_starts.tolist()
    assert starts[0] == 0 and starts[2] == len(blocks) and 0 < starts[1] < len(blocks)
    for i, b in enumerate(blocks):
        acceleration = 8 if i < starts[1] else 1
        assert dst[dst_off[i]:dst_off[i] + out_len[i]].tobytes() == ref.compress(b, acceleration), (i, acceleration)


def test_setter_refuses_and_keeps_the_value(g):
    A = g.A
    n = g.codec.native
    n.set_lz4_acceleration(7)
    for bad in (0, -1, 65538):
        with pytest.raises(A.IllegalArgumentException) as e:
            n.set_lz4_acceleration(bad)
        assert str(e.value) == "LZ4 acceleration should be in the [1, 65537] range but got %d" % bad
        assert n.get_lz4_acceleration() == 7
    n.set_lz4_acceleration(65537)
    assert n.get_lz4_acceleration() == 65537


def test_python_compressors_take_the_argument(g):
    A = g.A
    text = cases.alice()[:20000]
    for acceleration in (1, 4):
        block = A.Lz4HipCompressor(native_ctx=g.codec.native, acceleration=acceleration)
        frame = A.Lz4FrameHipCompressor(native_ctx=g.codec.native, acceleration=acceleration)  # (the same context: each compressor brings its own value)
        out = np.zeros(block.max_compressed_length(len(text)), dtype=np.uint8)
        assert out[:block.compress_segment(np.frombuffer(text, dtype=np.uint8), out)].tobytes() == ref.compress(text, acceleration)
        out = np.zeros(frame.max_compressed_length(len(text)), dtype=np.uint8)
        assert out[:frame.compress_segment(np.frombuffer(text, dtype=np.uint8), out)].tobytes() == ref.compress_frame(text, acceleration)
    assert A.Lz4HipCompressor(native_ctx=g.codec.native).acceleration == 1
