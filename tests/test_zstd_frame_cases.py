"""Checks on the hand-built Zstd frames of tests/zstd_frame_cases.py themselves (no GPU): the writer against the oracle's decoder, the catalog's
malformed frames refused by it, and every edge the catalog promises present -- counted from the generator's own records."""
import pytest

from tests import common, oracle_lib, zstd_frame_cases as zc
from tests.oracle_lib import OracleError


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


def test_the_writers_smallest_frame_and_checksum(o):
    frame, plain = zc.build_frame(b"A", [(1, 3, 1)], checksum=False, last_literals=0)
    assert frame == bytes.fromhex("28b52ffd20044500000841015401020004") and plain == b"AAAA"
    assert o.decompress("zstd", frame, 4) == b"AAAA"
    for data in (b"", b"a", b"abcd" * 7, bytes(range(256)) * 5 + b"xyz", common.corpus_sample()[0][1][:4099]):
        assert zc.xxh64(data) == o.xxh64(data) & ((1 << 64) - 1), len(data)
    frame, plain = zc.build_frame(b"hello, ", [(7, 14, 7)], checksum=True, last_literals=0)
    assert o.decompress("zstd", frame, 21) == b"hello, " * 3 == plain


def test_the_oracle_decodes_every_valid_frame_to_the_python_plaintext_and_refuses_every_malformed_one(o):
    cases = zc.catalog()
    assert 100 <= len(cases) <= 400 and sum(len(c.plain) for c in cases if c.plain) < 8 << 20
    for c in cases:
        for pad in (0, 64):
            cap = c.capacity(pad)
            if c.malformed:
                with pytest.raises(OracleError):
                    o.decompress("zstd", c.frame, cap)
            else:
                assert o.decompress("zstd", c.frame, cap) == c.plain, c.name
        assert zc.sequence_count(c.frame) == c.nseq, c.name


def test_every_edge_value_occurs(o):
    K = zc.kernel_constants()
    assert (K["GS"], K["IN_RING"], K["OUT_RING"]) == (4, 128, 256) and K["CHUNK"] == 64 and K["LDS_REACH"] == 176 and K["WIN"] == 4096
    cases = zc.catalog()
    valid = set().union(*[c.tags for c in cases if not c.malformed])
    missing = [t for t in zc.required_tags(K) if t not in valid]
    assert not missing, missing
    bad = set().union(*[c.tags for c in cases if c.malformed])
    assert not [t for t in zc.MALFORMED_KINDS if t not in bad]
    assert all(c.stage == 4 for c in cases if c.malformed)
    assert {c.checksum for c in cases if not c.malformed} == {True, False} and {c.checksum for c in cases if c.malformed} == {True, False}
    # both sides of the execute stage's per-item rule among the small frames (the large tiles are made of them)
    small = [c for c in cases if c.cap <= 4096]
    assert sum(1 for c in small if zc.is_long(c.cap, c.nseq, K)) >= 20 and sum(1 for c in small if not zc.is_long(c.cap, c.nseq, K)) >= 20


def test_every_header_form_occurs(o):
    """every literals block type x size format and every form of the sequence count, counted by the module's own reader over the frames the decode tests
    run: the catalog's valid frames, the size query's clean items, and the encoder's frames for the forms only an encoder can write"""
    from tests import decoded_size_cases
    frames = [c.frame for c in zc.catalog() if not c.malformed] + [comp for _, comp, _ in decoded_size_cases.clean_items(o, "zstd", big=False)]
    frames += [o.compress("zstd", p) for _, p in zc.form_plains()]
    seen = {}
    for f in frames:
        for form in zc.header_forms(f):
            seen[form] = seen.get(form, 0) + 1
    print(sorted(seen.items()))
    assert len(zc.HEADER_FORMS) == 19 and not [form for form in zc.HEADER_FORMS if seen.get(form, 0) == 0]
    # the hand frames bring the forms no encoder here writes: RLE literals, the 255 form
    hand = {form for c in zc.catalog() if not c.malformed for form in zc.header_forms(c.frame)}
    assert hand >= {("literals", "rle", k) for k in range(4)} | {("literals", "raw", k) for k in range(4)} | {("count", n) for n in ("one byte", "two bytes", "255")}


def test_sequence_counts_of_encoder_frames(o):
    """sequence_count() on the encoders' frames: Huffman and raw literal headers of every form; the oracle's encoder is the Java encoder restated"""
    text = b"".join(d for _, d, _ in common.corpus_sample()[:3])
    plains = zc.encoder_plains(text, common.synthetic_blocks(21, 1, 131072)[0])
    cases = zc.encoder_cases(plains, [("oracle", lambda b: o.compress("zstd", b))])
    assert len(cases) == 12 and all(c.nseq > 0 for c in cases)
    # (a text frame has a sequence every 10 .. 15 bytes or so: short; what is counted must be of that order)
    for c in cases:
        if c.name.startswith("oracle-text") and len(c.plain) >= 1000:
            assert len(c.plain) / 40 < c.nseq < len(c.plain) / 4, (c.name, c.nseq)
