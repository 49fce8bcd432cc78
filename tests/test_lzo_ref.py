"""The pure-Python LZO1X model (tests/lzo_ref.py) -- what every LZO kernel is checked against -- pinned from outside: liblzo2's recorded streams
(tests/golden/lzo_vectors.json, written by tools/record_lzo_vectors.py) decode to the recorded plaintexts, the model's compress output has the recorded length and
hash (and liblzo2 restored the plaintext from it when the file was recorded), and the catalog (tests/lzo_cases.py) says what its labels say."""
import hashlib
import json
import os

import pytest

from tests import lzo_cases as cases, lzo_ref as ref
from tests.conftest import reference_available

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lzo_vectors.json")


@pytest.fixture(scope="module")
def vectors():
    return json.load(open(GOLDEN))["vectors"]


def sha(b):
    return hashlib.sha256(b).hexdigest()[:16]  # (the file keeps 64 bits of every hash)


def test_model_decodes_every_recorded_liblzo2_stream(vectors):
    decoded = 0
    kinds = set()
    for label, e in vectors.items():
        for level in ("lzo1x_1", "lzo1x_999"):
            s = e.get(level, {}).get("hex")  # (not a stream of its own: {"same_as": "lzo1x_1"}, or beyond 8 KiB its length and hash)
            if s is None:
                continue
            stream = bytes.fromhex(s)
            plain = ref.decompress(stream, e["input_length"])
            assert len(plain) == e["input_length"] and sha(plain) == e["input_sha256"], (label, level)
            assert ref.decoded_size(stream) == e["input_length"]
            last = 0
            for c in ref.commands(stream):  # the two commands the Java encoder never emits, by the literals of the command before
                if c is not None and c[0] == 2 and 1 <= last <= 3 and c[1] <= 1024:
                    kinds.add((level, "2 bytes within 1 KiB behind 1..3 literals"))
                if c is not None and c[0] == 3 and last >= 4 and 2049 <= c[1] <= 3072:
                    kinds.add((level, "3 bytes at 2049..3072 behind 4 or more literals"))
                last = 0 if c is None else c[2]
            decoded += 1
    assert decoded >= 60  # (a level-999 stream equal to the level-1 stream is kept once)
    assert ("lzo1x_999", "2 bytes within 1 KiB behind 1..3 literals") in kinds
    assert ("lzo1x_999", "3 bytes at 2049..3072 behind 4 or more literals") in kinds


def test_model_compress_matches_the_recorded_hashes(vectors):
    inputs = dict(cases.vector_inputs())
    assert set(inputs) == set(vectors)
    for label, data in inputs.items():
        e = vectors[label]
        assert (len(data), sha(data)) == (e["input_length"], e["input_sha256"]), label  # (the catalog still builds the recorded plaintext)
        out = ref.compress(data)
        assert (len(out), sha(out)) == (e["model"]["length"], e["model"]["sha256"]), label
        assert (len(out), sha(out)) == (e["java"]["length"], e["java"]["sha256"]), label  # the reference's own encoder, transliterated (tools/record_lzo_vectors.py)
        assert e["model"]["liblzo2_restores"], label
        assert len(out) <= ref.max_compressed_length(len(data))


def test_round_trip_and_labels_of_every_encode_case():
    for label, data, predicate in cases.encode_cases():
        out = ref.compress(data)
        assert ref.decompress(out, len(data)) == data, label
        assert ref.decoded_size(out) == len(data), label
        if predicate is not None:
            assert predicate(ref.commands(out)), label  # the plaintext still provokes the emit path its label names
        if data:
            with pytest.raises(ref.Malformed):
                ref.decompress(out, len(data) - 1)
            with pytest.raises(ref.IllegalArgument):
                ref.compress(data, ref.max_compressed_length(len(data)) - 1)
    with pytest.raises(ref.IllegalArgument):
        ref.compress(b"", 15)  # the bound is checked before "nothing compresses to nothing"
    assert ref.compress(b"", 16) == b""


def test_decode_catalog_labels():
    valid = malformed = 0
    for case in cases.decode_cases():
        label, stream, capacity = case
        for cap, verdict in cases.runs(case):
            if capacity is None:  # a valid stream, with exact and with generous room
                assert verdict[0] == "ok" and len(verdict[1]) == ref.decoded_size(stream), label
                valid += 1
            else:
                assert verdict[0] == "malformed" and 0 <= verdict[1] <= len(stream), (label, verdict[0])
                malformed += 1
    assert valid >= 100 and malformed >= 60


def test_model_decodes_as_the_transliterated_java_decoder():
    """the reference's LzoRawDecompressor, transliterated and run over the decode catalog when the vectors were recorded: plaintext or offset per case"""
    recorded = json.load(open(GOLDEN))["java_decode"]
    seen = 0
    for case in cases.decode_cases() + [cases.long_run_case()]:
        for cap, verdict in cases.runs(case):
            theirs = recorded["%s @ %d" % (case[0], cap)]
            ours = "ok %d %s" % (len(verdict[1]), sha(verdict[1])) if verdict[0] == "ok" else "malformed %d" % verdict[1]
            assert theirs == ours, case[0]
            seen += 1
    assert seen == len(recorded) >= 190


@pytest.mark.parametrize("label, stream, offset", [
    ("nothing behind a first command 17", b"\x11", 1),
    ("first command 16", b"\x10", 1),
    ("a trailer cut in two", b"\x15abcd\x21\x04", 6),
    ("a match before the start", b"\x15abcd\x40\x01\x11\x00\x00", 7),
    ("literals past the input", b"\x04abcdef", 1),
])
def test_malformed_offsets_by_hand(label, stream, offset):
    """offsets worked out from the Java text by hand, not taken from the model"""
    with pytest.raises(ref.Malformed) as e:
        ref.decompress(stream, 100)
    assert e.value.offset == offset, label


def test_decoded_size_agrees_with_decompress():
    for case in cases.decode_cases() + [cases.long_run_case()]:
        label, stream, _ = case
        try:
            n = ref.decoded_size(stream)
        except ref.Malformed as e:
            with pytest.raises(ref.Malformed) as e2:
                ref.decompress(stream, ref.INT_MAX)
            assert e2.value.offset == e.offset, label
            continue
        assert len(ref.decompress(stream, n)) == n, label


def test_bounds_and_table_sizes():
    assert [ref.max_compressed_length(n) for n in (0, 1, 254, 255, 65536)] == [16, 17, 270, 272, 65809]
    assert ref.max_compressed_length(-1) == 15 and ref.max_compressed_length(-255) == -240
    assert [ref.compute_table_size(n) for n in (13, 16, 17, 2048, 2049, 1 << 20)] == [16, 16, 32, 2048, 4096, 4096]


@pytest.mark.reference
def test_liblzo2_cross_decode_live():
    """the recording, done again where the reference's checkout is: liblzo2 restores every plaintext from the model's stream, the model from liblzo2's"""
    if not reference_available():
        pytest.skip("needs the reference checkout")
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import record_lzo_vectors as rec
    lzo = rec.Liblzo2()
    assert lzo.version == "2030"
    for label, data in cases.vector_inputs():
        if not data:
            continue
        assert lzo.decompress(ref.compress(data), len(data)) == data, label
        recorded = json.load(open(GOLDEN))["vectors"][label]
        for level in (1, 999):
            stream = lzo.compress(data, level)
            assert ref.decompress(stream, len(data)) == data, (label, level)
            e = recorded["lzo1x_%d" % level]  # the recorded stream, or -- beyond 8 KiB -- its length and hash
            e = recorded[e["same_as"]] if "same_as" in e else e
            assert (e["hex"] == stream.hex()) if "hex" in e else ((e["length"], e["sha256"]) == (len(stream), sha(stream))), (label, level)
    agreed = 0
    for case in cases.decode_cases():  # the assembler's valid streams: where liblzo2 takes a stream (it is stricter than the Java decoder about a block's first command), it decodes the same bytes
        label, stream, capacity = case
        if capacity is None and stream:
            n = ref.decoded_size(stream)
            theirs = lzo.decompress(stream, n)
            assert theirs is None or theirs == ref.decompress(stream, n), label
            agreed += theirs is not None
    assert agreed >= 50
