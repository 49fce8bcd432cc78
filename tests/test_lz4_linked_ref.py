"""The model of the LZ4 frame reader with linked blocks (tests/lz4_linked_ref.py) against the oracle, and the catalog (tests/lz4_linked_cases.py) against the model:
where the Java reader has an answer the model gives the same one, so what the model adds is the one rule of linked blocks; every case of the catalog holds the edge
its label names and decodes to what its builder wrote -- or fails where the label says."""
import pytest

from tests import lz4_frame_vectors, lz4_linked_cases as cat, lz4_linked_ref as ref, oracle_lib


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


def oracle_answer(o, data, cap):
    try:
        return ref.Result(0, 0, o.decompress("lz4frame", data, cap))
    except oracle_lib.OracleError as e:
        return ref.Result(e.status, e.offset, b"")


def test_xxh32_is_the_oracles(o):
    for n in (0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 100, 1000):
        data = bytes((7 * k + n) & 0xFF for k in range(n))
        assert ref.xxh32(data) == o.xxh32(data)


def test_the_model_without_the_setting_is_the_java_reader_on_its_own_vectors(o):
    count = 0
    for name, frame, cap, plain, _ in lz4_frame_vectors.cases(o):
        want = oracle_answer(o, frame, cap)
        assert ref.decompress(frame, cap) == want, name
        if plain is not None:
            assert want.out == plain, name
        count += 1
    assert count >= 30  # (all of them: nothing is filtered above)


def test_the_setting_changes_nothing_for_frames_of_independent_blocks(o):
    """every vector but the one linked frame, and every independent-block case of the catalog: model off == model on == oracle"""
    items = [(name, frame, cap) for name, frame, cap, _, _ in lz4_frame_vectors.cases(o) if name != "linked blocks"]
    items += [(c.name, c.data, c.cap) for c in cat.cases() if not c.linked]
    assert sum(1 for c in cat.cases() if not c.linked) >= 2
    for name, data, cap in items:
        want = oracle_answer(o, data, cap)
        assert ref.decompress(data, cap, False) == want, name
        assert ref.decompress(data, cap, True) == want, name


def test_the_vectors_linked_frame_decodes_with_the_setting(o):
    """(its one block holds no match that reaches out of it: the content an independent frame would give)"""
    frame = lz4_frame_vectors.build(o, 0)
    assert ref.decompress(frame, len(lz4_frame_vectors.CONTENT), True) == ref.Result(0, 0, lz4_frame_vectors.CONTENT)


def test_every_damaged_vector_fails_alike_under_a_cleared_independence_bit(o):
    """the checks around the rule keep their order, detail and offset: the vectors of an independent frame, rebuilt as linked ones, give the model with the setting
    what the oracle gives for the independent original (the header checksum differs by the bit, so the frames are rebuilt, not patched)"""
    n = len(lz4_frame_vectors.CONTENT)
    ind = lz4_frame_vectors.FLG_BLOCK_INDEPENDENCE
    for extra, kw in ((lz4_frame_vectors.FLG_CONTENT_CHECKSUM, {"content_checksum": 5}), (lz4_frame_vectors.FLG_BLOCK_CHECKSUM, {"block_checksum": 5}),
                      (lz4_frame_vectors.FLG_CONTENT_SIZE, {"content_size": n + 1}), (lz4_frame_vectors.FLG_DICTIONARY_ID, {}), (lz4_frame_vectors.FLG_RESERVED_MASK, {}),
                      (0, {"bd": 0x10}), (0, {"bd": 0x71}), (0, {}), (0, {"stored": True})):
        independent, linked = lz4_frame_vectors.build(o, ind | extra, **kw), lz4_frame_vectors.build(o, extra, **kw)
        for cap in (n, n - 1):
            for cut in (0, 2, 4, 10):
                a, b = independent[:len(independent) - cut], linked[:len(linked) - cut]
                assert ref.decompress(b, cap, True) == oracle_answer(o, a, cap), (extra, kw, cap, cut)


def test_every_case_holds_the_edge_its_label_names():
    for c in cat.cases():
        assert c.label and c.claims, c.name
        assert cat.claim_failures(c) == [], c.name


def test_every_linked_case_gives_what_its_builder_wrote_or_fails_where_its_label_says():
    linked = [c for c in cat.cases() if c.linked]
    assert len(linked) >= 40
    for c in linked:
        got = ref.decompress(c.data, c.cap, True)
        if c.plain is not None:
            assert got == ref.Result(0, 0, c.plain), c.name
        else:
            assert c.status != 0 and (got.status, got.offset, got.out) == (c.status, c.offset, b""), (c.name, got.status, got.offset)
        off = ref.decompress(c.data, c.cap, False)
        assert (off.status, off.offset) == (ref.malformed(ref.D_LINKED_BLOCKS), cat.linked_descriptor(c)), c.name


def test_the_greedy_encoder_keeps_the_end_of_block_rules():
    """the last five bytes of a block are literals, no match starts in its last twelve -- and a linked encoding is smaller than an independent one"""
    plain = cat.text(40000, seed=3)
    sizes = {}
    for linked in (True, False):
        f = ref.frame(ref.greedy_blocks(plain, 9000, linked), linked=linked, size_id=4)
        assert f.plain == plain
        for block in ref.walk(f.data)[0].blocks:
            assert block.tail >= 5
            assert all(q.pos <= block.size - 12 and q.pos + q.ml <= block.size - 5 for q in block.seqs)
        sizes[linked] = len(f.data)
    assert sizes[True] < sizes[False]
