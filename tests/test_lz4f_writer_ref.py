"""The pure-Python LZ4 frame writer of tests/lz4f_writer_ref.py held to the oracle, and the catalog of tests/lz4f_writer_cases.py held to its labels (CPU only).
At the Java writer's settings the model's bytes are the oracle's frame writer's; at every setting the oracle's frame reader -- Lz4FrameCompression.decompress
restated, which verifies the header checksum, every block checksum, the content checksum and the content size -- reads every model frame back to the plaintext,
and so does the linked-frame model's reader."""
import struct

import pytest

from tests import lz4_linked_ref, lz4f_writer_cases as cases, lz4f_writer_ref as ref, oracle_lib
from tests.lz4_linked_ref import xxh32


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


def test_at_the_java_writers_settings_the_model_is_the_oracle(o):
    seen = 0
    for c in cases.catalog():
        assert ref.compress(c.data, *ref.DEFAULT) == o.compress("lz4frame", c.data), c.name
        seen += 1
    assert seen == len(cases.catalog()) > 200


def test_every_model_frame_reads_back_through_the_oracle_and_the_linked_model(o):
    for c in cases.catalog():
        frame = cases.expected(c.name)
        assert len(frame) <= cases.bound(c), c.name
        assert o.decompress("lz4frame", frame, len(c.data)) == c.data, c.name
        back = lz4_linked_ref.decompress(frame, len(c.data))
        assert (back.status, back.out) == (0, c.data), c.name


def test_the_oracle_reader_does_verify_what_the_model_writes(o):
    """a damaged block checksum, content checksum or content size of a model frame is refused: the read-back above is a check of those fields"""
    c = next(c for c in cases.catalog() if c.settings == (65536, 1, 1, 1) and "two blocks" in c.labels and "compressed" in c.labels)
    frame = cases.expected(c.name)
    p = ref.parse(frame)
    first = p.blocks[0]
    for at in (first.at + 4 + len(first.data), len(frame) - 1, 6):  # the first block's checksum, the content checksum, the content size
        damaged = bytearray(frame)
        damaged[at] ^= 0x01
        with pytest.raises(oracle_lib.OracleError):
            o.decompress("lz4frame", bytes(damaged), len(c.data) + 2)


def test_every_case_holds_what_its_labels_say():
    seen = set()
    for c in cases.catalog():
        block_size, bc, cc, cs = c.settings
        p = ref.parse(cases.expected(c.name))
        assert p.block_size == block_size and p.flg == 0x60 | bc << 4 | cs << 3 | cc << 2, c.name
        stored = [b.stored for b in p.blocks]
        sizes = [min(block_size, len(c.data) - k * block_size) for k in range(len(p.blocks))]
        assert sum(sizes) == len(c.data) and all(s > 0 for s in sizes), c.name
        facts = {
            "empty": len(c.data) == 0 and p.blocks == [],
            "two blocks": len(p.blocks) >= 2,
            "block checksum": bool(p.blocks) and all(b.checksum == xxh32(b.data) for b in p.blocks),
            "content checksum": p.content_checksum == xxh32(c.data) and cc == 1,
            "content size": p.content_size == len(c.data) and cs == 1,
            "stored": any(stored),
            "compressed": any(not s for s in stored),
            "stored between compressed": any(not a and b and not c2 for a, b, c2 in zip(stored, stored[1:], stored[2:])),
            "compressed between stored": any(a and not b and c2 for a, b, c2 in zip(stored, stored[1:], stored[2:])),
            "all stored": len(stored) >= 2 and all(stored),
            "wide table": any(z > 65536 for z in sizes),
        }
        for k, b in enumerate(p.blocks):  # a stored block is the plaintext, and is there because the encoder's bytes were no fewer
            if b.stored:
                assert b.data == c.data[k * block_size:k * block_size + sizes[k]], c.name
                assert len(ref.encode_block(b.data)) >= len(b.data), c.name
        if not bc:
            assert all(b.checksum is None for b in p.blocks), c.name
        for label in c.labels:
            assert facts[label], (c.name, label)
        for label, holds in facts.items():  # ... and a case is labelled with everything it holds
            assert holds == (label in c.labels), (c.name, label, holds)
        seen |= c.labels
    assert seen == set(cases.REQUIRED_LABELS)


def test_the_catalog_has_every_shape_the_issue_names():
    by = cases.by_settings()
    assert [s for s in by if s[0] == 65536] == [(65536,) + f for f in cases.FLAG_SETS] and len(cases.FLAG_SETS) == 8
    for flags in cases.FLAG_SETS:
        lengths = {(c.name.split(" ")[0], len(c.data)) for c in by[(65536,) + flags]}
        for kind in ("zeros", "text", "random"):
            assert {n for k, n in lengths if k == kind} == set(cases.LENGTHS_64K)
    for block_size in cases.LARGE_BLOCK_SIZES:
        for flags in ((0, 0, 0), (1, 1, 1)):
            assert [len(c.data) for c in by[(block_size,) + flags]] == [block_size - 1, block_size, block_size + 1]
    assert cases.MISALIGNMENTS == (0, 1, 2, 3)


def test_the_bound_is_the_worst_case_places():
    assert ref.max_compressed_length(0, *ref.DEFAULT) == 11
    assert ref.max_compressed_length(65537, 65536, 1, 1, 1) == 15 + (8 + 65536 + 257 + 16) + (8 + 1 + 16) + 8
    assert ref.header(5, 4194304, 0, 0, 0) == struct.pack("<I", ref.MAGIC) + bytes([0x60, 0x70, 0x73])


def test_acceleration_above_one_takes_the_accelerated_block_encoder():
    d = cases.data("text", 70000, 5)
    slow, fast = ref.compress(d, 65536, 1, 0, 0), ref.compress(d, 65536, 1, 0, 0, acceleration=7)
    assert slow != fast
    assert lz4_linked_ref.decompress(fast, len(d)).out == d
