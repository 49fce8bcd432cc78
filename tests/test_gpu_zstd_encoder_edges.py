"""The catalog of constructed Zstd encoder inputs (tests/zstd_encoder_cases.py: every path of the frame, block, literals and sequences code and of the match
finders, each case proven to reach its edge by tests/test_zstd_encoder_cases.py) through every encoder variant on the GPU: the oracle's bytes for every case,
from sources packed 16-byte aligned and packed back to back; the frames back through the decoder; tight capacities; the stream writer."""
import numpy as np
import pytest

from tests import oracle_lib
from tests import zstd_encoder_cases as ze
from tests.oracle_lib import OracleError

pytestmark = pytest.mark.gpu

VARIANTS = (3, 0, 1, 2)
DEFAULT_VARIANT = 3
_batch = None


def batch():
    """the catalog in a fixed shuffled order, the oracle's frames and capacities: computed once"""
    global _batch
    if _batch is None:
        o = oracle_lib.load()
        cases = ze.cases()
        cases = [cases[i] for i in np.random.default_rng(11).permutation(len(cases))]
        _batch = ([n for n, _, _ in cases], [d for _, d, _ in cases], [o.compress("zstd", d) for _, d, _ in cases], [o.max_compressed_length("zstd", len(d)) for _, d, _ in cases])
    return _batch


def own_batch(options):
    from tests.gpu_harness import GpuBatch
    return GpuBatch(0, options)


@pytest.mark.parametrize("variant", VARIANTS)
def test_catalog_is_bit_exact_with_oracle(variant):
    names, blocks, want, caps = batch()
    g = own_batch({"zstd.compress.variant": variant})
    try:
        for unaligned in (True, False):
            how = "back to back" if unaligned else "aligned"
            outs, status, _ = g.run(5, blocks, caps, unaligned=unaligned)
            failed = [n for n, s in zip(names, status) if s != 0]
            assert not failed, "variant %d, %s: status of %r" % (variant, how, failed[:10])
            differ = [n for n, c, w in zip(names, outs, want) if c != w]
            assert not differ, "variant %d, %s sources: %d cases differ from the oracle: %r" % (variant, how, len(differ), differ[:10])
    finally:
        g.set_option("zstd.compress.variant", DEFAULT_VARIANT)


def test_gpu_decoder_restores_the_catalog_from_the_gpu_frames():
    names, blocks, want, caps = batch()
    g = own_batch({})
    outs, status, _ = g.run(5, blocks, caps, unaligned=True)
    assert all(s == 0 for s in status) and outs == want
    plain, status, _ = g.run(4, outs, [max(len(b), 1) for b in blocks], unaligned=True)
    wrong = [n for n, b, p, s in zip(names, blocks, plain, status) if s != 0 or p != b]
    assert not wrong, "the decoder does not restore %r" % wrong[:10]


LADDER = ("frame/size=6/raw-block",                                   # a raw block
          "literals/rle/64",                                          # RLE literals (two blocks)
          "literals/huffman/1024/streams=4,form=2",                   # four-stream Huffman literals
          "literals/huffman/255/streams=1,form=0",                    # one stream
          "seq-modes/n=40,codes-same-varied-same/ll=rle,of=fse,ml=rle",  # an FSE offsets table: its limit is output + outputSize, as in the Java
          "seq-modes/n=80,codes-varied-varied-varied/ll=fse,of=fse,ml=fse",
          "blocks/last-block-of-6/raw",                               # multi-block
          "sequences/count=130")


def test_capacity_ladder():
    """capacities 0 .. 24, the oracle's length minus {40, 9, 8, 7, 4, 3, 1, 0}, plus 1, and the bound -- back to back, so that an overrun lands in the
    neighbour's output: status and bytes are what the oracle's compress(data, capacity) gives or raises"""
    o = oracle_lib.load()
    by_name = {n: d for n, d, _ in ze.cases()}
    names, blocks, caps = [], [], []
    for name in LADDER:
        data = by_name[name]
        full = len(o.compress("zstd", data))
        for cap in sorted(set(list(range(25)) + [full - k for k in (40, 9, 8, 7, 4, 3, 1, 0) if full - k >= 0] + [full + 1, o.max_compressed_length("zstd", len(data))])):
            names.append("%s at %d" % (name, cap))
            blocks.append(data)
            caps.append(cap)
    outs, status, _ = own_batch({}).run(5, blocks, caps, unaligned=True)
    wrong = []
    for n, b, cap, c, s in zip(names, blocks, caps, outs, status):
        try:
            want, st = o.compress("zstd", b, cap), 0
        except OracleError as e:
            want, st = None, e.status
        if s != st or (st == 0 and c != want):
            wrong.append((n, s, st))
    assert not wrong, "%d of %d differ from the oracle (case, status, the oracle's): %r" % (len(wrong), len(names), wrong[:10])


def test_stream_writer_on_the_emulator_sized_cases():
    """the emulator-sized part of the catalog once through the ZstdOutputStream writer against the oracle's"""
    o = oracle_lib.load()
    cases = ze.emulator_cases()
    blocks = [d for _, d, _ in cases]
    want = [o.zstd_stream_compress(b) for b in blocks]
    outs, status, _ = own_batch({}).run(14, blocks, [o.lib.orc_zstd_stream_max_compressed_length(len(b)) for b in blocks], unaligned=True)
    wrong = [n for (n, _, _), c, s, w in zip(cases, outs, status, want) if s != 0 or c != w]
    assert not wrong, "%d streams differ from the oracle's: %r" % (len(wrong), wrong[:10])
