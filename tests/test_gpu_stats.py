"""achip_ctx_get_stat on the GPU: a statistic kept in the scratch answers for the last launch that took the scratch and is -1 after any other (DESIGN 8b;
achip_stats.h).  Every launch that leaves statistics (the producers) is followed, on the same context, by every other kind of call that takes the scratch
(the interveners): the producer's statistics are valid after it and -1 after the intervener.  And the rule does not over-clear: the producer twice in a row
leaves valid statistics twice.  All batches are 16 items of 1 KiB of text, the smallest that takes every path: lz4.decompress.auto_min_blocks is set to 16, the
option's minimum, so that 16 blocks run auto mode's probes."""
import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

N, ITEM = 16, 1024
ROOM = 4096  # per compressed item: any of the formats' worst case for 1 KiB
OP_LZ4_D, OP_LZ4_C, OP_SNAPPY_D, OP_SNAPPY_C, OP_ZSTD_D, OP_ZSTD_C, OP_LZ4F_D, OP_LZ4F_C, OP_SNF_C, OP_LZ4H_D, OP_LZ4H_C, OP_LZO_D, OP_LZO_C = 0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 16, 17
FIRST_LAST = 1 | 2  # ACHIP_WINDOW_FIRST | ACHIP_WINDOW_LAST


@pytest.fixture(scope="module")
def g():
    from tests.gpu_harness import GpuBatch
    return GpuBatch(0, options={"lz4.decompress.auto_min_blocks": 16})


@pytest.fixture(scope="module")
def plains():
    text = common.corpus_sample()[0][1]  # calgary/book1
    return tuple(text[i * ITEM:(i + 1) * ITEM] for i in range(N))


@pytest.fixture(scope="module")
def streams(g, plains):
    """{compress op: the 16 items compressed by it} -- made once (on a context of their own, so that no test depends on what making them left behind)"""
    from tests.gpu_harness import GpuBatch
    maker = GpuBatch(0)
    out = {}
    for op in (OP_LZ4_C, OP_SNAPPY_C, OP_ZSTD_C, OP_LZ4F_C, OP_LZ4H_C, OP_LZO_C):
        outs, status, _ = maker.run(op, list(plains), [ROOM] * N)
        assert status == [0] * N, (op, status)
        out[op] = tuple(outs)
    return out


def stat(g, name):
    return g.codec.native.get_stat(name)


def decode(g, op, comp, plains, options):
    for k, v in options.items():
        g.set_option(k, v)
    outs, status, _ = g.run(op, list(comp), [ITEM] * N)
    assert status == [0] * N and tuple(outs) == plains, status


# ---- producers: launch -> {statistic kept in the scratch: what it must be right after the launch} (None: any value >= 0; UNSTATED: checked afterwards only) ----
UNSTATED = "unstated"



def lz4_auto(g, streams, plains):
    decode(g, OP_LZ4_D, streams[OP_LZ4_C], plains, {"lz4.decompress.variant": 5})
    choice = stat(g, "decompress.choice")
    assert choice in (0, 3), choice
    # (choice 0: the two passes were launched beside the rings and returned at once, or -- a remembered choice -- not at all: their count is 0 or -1)
    return {"lz4.decompress.mixed_groups": None, "decompress.choice": choice, "decompress.twopass_fallback_blocks": None if choice == 3 else UNSTATED}


def snappy_two_passes(g, streams, plains):
    try:
        decode(g, OP_SNAPPY_D, streams[OP_SNAPPY_C], plains, {"snappy.decompress.variant": 7})
    finally:
        g.set_option("snappy.decompress.variant", 5)
    return {"decompress.twopass_fallback_blocks": None}


def zstd_pipeline(g, streams, plains):
    decode(g, OP_ZSTD_D, streams[OP_ZSTD_C], plains, {"zstd.decompress.variant": 1})
    return {"zstd.decompress.fallback_items": None, "zstd.decompress.fallback_stage1": None, "zstd.decompress.multiblock_items": None, "zstd.decompress.long_items": None}


def zstd_one_kernel(g, streams, plains):
    try:
        decode(g, OP_ZSTD_D, streams[OP_ZSTD_C], plains, {"zstd.decompress.variant": 0})
    finally:
        g.set_option("zstd.decompress.variant", 1)
    return {"zstd.decompress.fallback_items": N}


def lzo(variant):
    def producer(g, streams, plains):
        try:
            decode(g, OP_LZO_D, streams[OP_LZO_C], plains, {"lzo.decompress.variant": variant})
        finally:
            g.set_option("lzo.decompress.variant", 0)
        return {"lzo.decompress.fallback_blocks": 0}
    producer.__name__ = "lzo_variant_%d" % variant
    return producer


PRODUCERS = (lz4_auto, snappy_two_passes, zstd_pipeline, zstd_one_kernel, lzo(1), lzo(2))


# ---- interveners: another call on the same context that takes the scratch; its statuses are 0 ----
def device_arrays(g, blocks, caps):
    """a batch's arrays on the device, as GpuBatch.run makes them"""
    torch = g.torch
    src, src_off, src_len = g.pack(list(blocks))
    caps = np.asarray(caps, dtype=np.int32)
    dst_off = np.cumsum(np.concatenate(([0], (caps[:-1].astype(np.int64) + 15) // 16 * 16)))
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(g.dev)  # noqa: E731
    n = len(blocks)
    d = {"src": to(src), "src_off": to(src_off), "src_len": to(src_len), "dst_off": to(dst_off), "dst_cap": to(caps),
         "dst": torch.zeros(int(dst_off[-1]) + int(caps[-1]) + 64, dtype=torch.uint8, device=g.dev),
         "out_len": torch.full((n,), -7, dtype=torch.int32, device=g.dev), "status": torch.full((n,), -7, dtype=torch.int32, device=g.dev),
         "err": torch.zeros(n, dtype=torch.int64, device=g.dev)}
    torch.cuda.synchronize()
    return d


def lz4_compress(g, streams, plains):
    outs, status, _ = g.run(OP_LZ4_C, list(plains), [ROOM] * N)
    assert status == [0] * N and tuple(outs) == streams[OP_LZ4_C]


def zstd_compress(g, streams, plains):
    outs, status, _ = g.run(OP_ZSTD_C, list(plains), [ROOM] * N)
    assert status == [0] * N and tuple(outs) == streams[OP_ZSTD_C]


def lz4_frame_decode(g, streams, plains):
    outs, status, _ = g.run(OP_LZ4F_D, list(streams[OP_LZ4F_C]), [ITEM] * N)
    assert status == [0] * N and tuple(outs) == plains


def decoded_size_batch(g, streams, plains):
    """(of LZ4 frames: a size query that works in the scratch -- the block codecs' does not, and leaves the statistics alone)"""
    d = device_arrays(g, streams[OP_LZ4F_C], [ITEM] * N)
    size = g.torch.full((N,), -7, dtype=g.torch.int64, device=g.dev)
    g.codec.decoded_sizes(OP_LZ4F_D, d["src"], d["src_off"], d["src_len"], size, d["status"], d["err"], N)
    g.codec.synchronize()
    assert d["status"].cpu().tolist() == [0] * N and size.cpu().tolist() == [ITEM] * N


def plan_outputs(g, streams, plains):
    torch = g.torch
    size = torch.full((N,), ITEM, dtype=torch.int64, device=g.dev)
    status = torch.zeros(N, dtype=torch.int32, device=g.dev)
    dst_off, dst_cap, total = torch.zeros(N, dtype=torch.int64, device=g.dev), torch.zeros(N, dtype=torch.int32, device=g.dev), torch.zeros(2, dtype=torch.int64, device=g.dev)
    torch.cuda.synchronize()
    g.codec.plan_outputs(size, status, N, 16, dst_off, dst_cap, total)
    g.codec.synchronize()
    assert total.cpu().tolist() == [N * ITEM, 0] and dst_off.cpu().tolist() == [i * ITEM for i in range(N)]


def pack_outputs(g, streams, plains):
    torch = g.torch
    comp = streams[OP_LZ4_C]
    d = device_arrays(g, comp, [len(c) for c in comp])
    out_len = d["src_len"]
    status = torch.zeros(N, dtype=torch.int32, device=g.dev)
    packed_off, packed_len, total = torch.zeros(N, dtype=torch.int64, device=g.dev), torch.zeros(N, dtype=torch.int32, device=g.dev), torch.zeros(3, dtype=torch.int64, device=g.dev)
    want = sum(len(c) for c in comp)
    packed = torch.zeros(want + 64, dtype=torch.uint8, device=g.dev)
    torch.cuda.synchronize()
    g.codec.pack_outputs(d["src"], d["src_off"], out_len, status, N, 1, packed, want, packed_off, packed_len, total)
    g.codec.synchronize()
    assert total.cpu().tolist() == [want, 0, 1] and packed[:want].cpu().numpy().tobytes() == b"".join(comp)


def window(g, compress, op, windows, caps):
    torch = g.torch
    d = device_arrays(g, windows, caps)
    flags = torch.full((N,), FIRST_LAST, dtype=torch.int32, device=g.dev)
    stop = torch.full((N,), -7, dtype=torch.int32, device=g.dev)
    consumed, need = torch.zeros(N, dtype=torch.int64, device=g.dev), torch.zeros(N, dtype=torch.int64, device=g.dev)
    torch.cuda.synchronize()
    call = g.codec.window_compress if compress else g.codec.window_decompress
    call(op, flags, d["src"], d["src_off"], d["src_len"], d["dst"], d["dst_off"], d["dst_cap"], d["out_len"], d["status"], d["err"], N, consumed, stop, need)
    g.codec.synchronize()
    assert d["status"].cpu().tolist() == [0] * N and stop.cpu().tolist() == [0] * N  # (ACHIP_STOP_END)
    assert consumed.cpu().tolist() == [len(w) for w in windows]
    return d["out_len"].cpu().tolist()


def lz4_hadoop_window_decode(g, streams, plains):
    assert window(g, False, OP_LZ4H_D, streams[OP_LZ4H_C], [ITEM] * N) == [ITEM] * N


def snappy_framed_window_compress(g, streams, plains):
    assert all(0 < n <= ROOM for n in window(g, True, OP_SNF_C, plains, [ROOM] * N))


INTERVENERS = (lz4_compress, zstd_compress, lz4_frame_decode, decoded_size_batch, plan_outputs, pack_outputs, lz4_hadoop_window_decode, snappy_framed_window_compress)


def check_valid(g, expected):
    for name, want in expected.items():
        got = stat(g, name)
        assert want is UNSTATED or ((got >= 0) if want is None else (got == want)), (name, got, want)


@pytest.mark.parametrize("intervener", INTERVENERS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("producer", PRODUCERS, ids=lambda f: f.__name__)
def test_statistics_end_with_the_next_launch_that_takes_the_scratch(g, streams, plains, producer, intervener):
    """(no intervener is a producer's own op, so this is the full cross product)"""
    expected = producer(g, streams, plains)
    check_valid(g, expected)
    intervener(g, streams, plains)
    left = {name: stat(g, name) for name in expected}
    assert left == {name: -1 for name in expected}, left


@pytest.mark.parametrize("producer", PRODUCERS, ids=lambda f: f.__name__)
def test_the_same_launch_again_leaves_its_statistics_again(g, streams, plains, producer):
    check_valid(g, producer(g, streams, plains))
    check_valid(g, producer(g, streams, plains))
