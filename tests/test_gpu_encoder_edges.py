"""The catalog of constructed encoder inputs (tests/encoder_edge_cases.py: every path of the LZ4 and Snappy window encoders, every numeric edge of the formats,
each case proven to reach its edge by tests/test_encoder_edge_cases.py) through every encoder variant on the GPU: the oracle's bytes for every case, whichever
kernel, tier or wavefront drew it, from sources packed 16-byte aligned and packed back to back."""
import numpy as np
import pytest

from tests import encoder_edge_cases as ec
from tests import oracle_lib

pytestmark = pytest.mark.gpu

OPS = {"lz4": dict(c=1, d=0), "snappy": dict(c=3, d=2)}
# (name, options of the test's own context) -- every option is put back to its default afterwards
CONFIGS = {
    "lz4": [("4, a wavefront per block", {"lz4.compress.variant": 4}),
            ("4, two tiers, one memory wavefront", {"lz4.compress.variant": 4, "lz4.compress.tier_min_blocks": 1, "lz4.compress.mem_waves": 1}),
            ("4, two tiers, two memory wavefronts", {"lz4.compress.variant": 4, "lz4.compress.tier_min_blocks": 1, "lz4.compress.mem_waves": 2}),
            ("1", {"lz4.compress.variant": 1}),
            ("0", {"lz4.compress.variant": 0})],
    "snappy": [("4", {"snappy.compress.variant": 4}),
               ("4, sub-blocks in turn", {"snappy.compress.variant": 4, "snappy.compress.fan": 0}),
               ("2", {"snappy.compress.variant": 2}),
               ("1", {"snappy.compress.variant": 1}),
               ("0", {"snappy.compress.variant": 0})],
}
DEFAULTS = {"lz4.compress.variant": 4, "lz4.compress.tier_min_blocks": 5120, "lz4.compress.mem_waves": 1, "snappy.compress.variant": 4, "snappy.compress.fan": 1}

_batches = {}


def batch(codec):
    """the catalog in a fixed shuffled order (neighbours in a tiers workgroup differ), the oracle's streams and capacities: computed once"""
    if codec not in _batches:
        o = oracle_lib.load()
        cases = ec.cases(codec)
        order = np.random.default_rng(5).permutation(len(cases))
        cases = [cases[i] for i in order]
        _batches[codec] = ([n for n, _, _ in cases], [d for _, d, _ in cases], [o.compress(codec, d) for _, d, _ in cases], [o.max_compressed_length(codec, len(d)) for _, d, _ in cases])
    return _batches[codec]


def own_batch(options):
    from tests.gpu_harness import GpuBatch
    return GpuBatch(0, options)


def restore(g, options):
    for k in options:
        g.set_option(k, DEFAULTS[k])


@pytest.mark.parametrize("codec, config", [(c, k) for c in ("lz4", "snappy") for k in range(5)], ids=lambda v: str(v))
def test_catalog_is_bit_exact_with_oracle(codec, config):
    what, options = CONFIGS[codec][config]
    names, blocks, want, caps = batch(codec)
    g = own_batch(options)
    try:
        for unaligned in (True, False):
            outs, status, _ = g.run(OPS[codec]["c"], blocks, caps, unaligned=unaligned)
            failed = [n for n, s in zip(names, status) if s != 0]
            assert not failed, "%s variant %s, %s: status of %r" % (codec, what, "unaligned" if unaligned else "aligned", failed[:10])
            differ = [n for n, c, w in zip(names, outs, want) if c != w]
            assert not differ, "%s variant %s, %s sources: %d cases differ from the oracle: %r" % (codec, what, "unaligned" if unaligned else "aligned", len(differ), differ[:10])
    finally:
        restore(g, options)


@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_gpu_decoder_restores_the_catalog_from_the_gpu_streams(codec):
    """the default encoder's streams through the decoder of the same codec in its default (auto) mode"""
    names, blocks, want, caps = batch(codec)
    g = own_batch({})
    outs, status, _ = g.run(OPS[codec]["c"], blocks, caps, unaligned=True)
    assert all(s == 0 for s in status) and outs == want
    plain, status, _ = g.run(OPS[codec]["d"], outs, [max(len(b), 1) for b in blocks], unaligned=True)
    wrong = [n for n, b, p, s in zip(names, blocks, plain, status) if s != 0 or p != b]
    assert not wrong, "%s: the decoder does not restore %r" % (codec, wrong[:10])


def test_zstd_encoder_on_both_catalogs():
    """the inputs a match finder trips on, once through Zstd compress (default variant) against the oracle's frames"""
    o = oracle_lib.load()
    names = [n for c in ("lz4", "snappy") for n in batch(c)[0]]
    blocks = [d for c in ("lz4", "snappy") for d in batch(c)[1]]
    caps = [o.max_compressed_length("zstd", len(b)) for b in blocks]
    g = own_batch({})
    outs, status, _ = g.run(5, blocks, caps)
    failed = [n for n, s in zip(names, status) if s != 0]
    assert not failed, "status of %r" % failed[:10]
    differ = [n for n, b, c in zip(names, blocks, outs) if c != o.compress("zstd", b)]
    assert not differ, "%d cases differ from the oracle: %r" % (len(differ), differ[:10])
