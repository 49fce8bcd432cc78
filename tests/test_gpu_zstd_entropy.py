"""GPU parity tests (through the C ABI) for the Zstd decoder's entropy stages on the catalog of tests/zstd_entropy_cases.py: hand-built FSE table descriptions,
Huffman tables and streams, treeless literals and repeat-mode tables across blocks.  The expectation of every case is the oracle's (the Java decoder): status, error
offset and bytes.  On the CPU the same catalog runs under tools/hostemu/check_zstd.py --part entropy."""
import numpy as np
import pytest

from tests import oracle_lib
from tests import zstd_entropy_cases as ze
from tests.oracle_lib import OracleError

pytestmark = pytest.mark.gpu
OP_ZSTD_DECOMPRESS = 4
DEFAULT_SEQ_WAVES = 1   # (the library's defaults, restored by the tests that change them)
DEFAULT_LIT_ITEMS = 13


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


@pytest.fixture(scope="module")
def entropy_cases(o):
    """(cases, expected): expected[pad][i] is the oracle's (status, offset, bytes) for case i at its capacity + pad -- computed once, shared, left unchanged"""
    cases = ze.entropy_catalog()

    def expect(c, cap):
        try:
            return 0, 0, o.decompress("zstd", c.frame, cap)
        except OracleError as e:
            return e.status, e.offset, None
    expected = {pad: [expect(c, c.capacity(pad)) for c in cases] for pad in (0, 64)}
    for pad in (0, 64):
        for c, (est, _, eout) in zip(cases, expected[pad]):
            assert (est != 0) == c.malformed and (c.malformed or eout == c.plain), c.name  # (also tests/test_zstd_entropy_cases.py)
    return cases, expected


def _run(g, cases, expected, pad, order, pipeline):
    """the cases in `order` through g at capacity + pad: status, offset and bytes as the oracle has them; on the pipeline exactly the malformed cases and those that
    leave it by design are handed to the one-kernel decoder (a valid frame that silently leaves the fast path tests nothing)"""
    sub = [cases[i] for i in order]
    outs, status, err = g.run(OP_ZSTD_DECOMPRESS, [c.frame for c in sub], [c.capacity(pad) for c in sub], unaligned=(pad == 0))
    for k, c in enumerate(sub):
        est, eoff, eout = expected[pad][order[k]]
        assert status[k] == est, "%s: gpu status %d oracle %d (gpu offset %d, oracle %d)" % (c.name, status[k], est, err[k], eoff)
        if est == 0:
            assert len(outs[k]) == len(eout) and outs[k] == eout, c.name
        else:
            assert err[k] == eoff, "%s: gpu offset %d oracle %d" % (c.name, err[k], eoff)
    if pipeline:
        stat = g.codec.native.get_stat
        stages = [stat("zstd.decompress.fallback_stage%d" % k) for k in range(1, 7)]
        want = sum(1 for c in cases if c.malformed or c.fallback)
        assert stat("zstd.decompress.fallback_items") == want == sum(stages), stages
        # by stage: what the parse stage (and the multi-block walk, stage 6) refuses; the literal stage (streams that decode short or long); the sequence stage
        # (a stream without its end mark, the sequences of a block whose tables are not there)
        assert stages[3] == 0 and stages[4] == 0, stages
        assert stages[1] == sum(1 for c in cases if c.tags & {"stream-decodes-short", "stream-decodes-long"}) + sum(1 for c in cases if c.name == "huf-four-streams-5"), stages


@pytest.mark.parametrize("lit_items,seq_waves", [(13, DEFAULT_SEQ_WAVES), (16, DEFAULT_SEQ_WAVES), (13, 4), (16, 4), (20, DEFAULT_SEQ_WAVES)],
                         ids=["split-tables", "plain-entries", "split-tables-4-waves", "plain-entries-4-waves", "lengths-by-symbol"])
def test_entropy_catalog_through_the_pipeline(entropy_cases, lit_items, seq_waves):
    """zstd.decompress.lit_items 13 (symbol bytes and length nibbles apart) and 16 (plain u16 entries), zstd.decompress.seq_waves at its default and at 4; the catalog
    twice, in catalog order and in a seeded shuffle (other lanes, slots and neighbours for every case), at exact capacities with unaligned outputs and with 64 bytes of
    slack.  lit_items 20 (lengths by symbol) once more: its table staging wrote the lengths of entries behind a table of fewer than 8 entries."""
    from tests.gpu_harness import GpuBatch
    cases, expected = entropy_cases
    g = GpuBatch(0, options={"zstd.decompress.variant": 1})
    shuffled = [int(i) for i in np.random.default_rng(77).permutation(len(cases))]
    try:
        g.set_option("zstd.decompress.lit_items", lit_items)
        g.set_option("zstd.decompress.seq_waves", seq_waves)
        for pad in (0, 64):
            _run(g, cases, expected, pad, list(range(len(cases))), True)
            _run(g, cases, expected, pad, shuffled, True)
    finally:
        g.set_option("zstd.decompress.lit_items", DEFAULT_LIT_ITEMS)
        g.set_option("zstd.decompress.seq_waves", DEFAULT_SEQ_WAVES)


def test_entropy_catalog_through_the_one_kernel_decoder_and_the_size_query(entropy_cases):
    """zstd.decompress.variant 0: the decoder everything irregular falls back to, on every case; and the decoded-size query on the valid ones"""
    from tests.gpu_harness import GpuBatch
    from tests.test_gpu_decoded_size import size_on_gpu
    cases, expected = entropy_cases
    g = GpuBatch(0, options={"zstd.decompress.variant": 0})
    for pad in (0, 64):
        _run(g, cases, expected, pad, list(range(len(cases))), False)
    valid = [c for c in cases if not c.malformed]
    size, status, err, _ = size_on_gpu(g, OP_ZSTD_DECOMPRESS, [c.frame for c in valid])
    wrong = [(c.name, int(s), int(z), len(c.plain)) for c, s, z in zip(valid, status, size) if s != 0 or z != len(c.plain)]
    assert not wrong, wrong[:8]
    assert (err == 0).all()
