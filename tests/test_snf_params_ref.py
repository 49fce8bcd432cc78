"""The pure-Python SnappyFramedOutputStream with its five-argument constructor (tests/snf_params_ref.py), the reference of the tests at parameters the oracle's
one-shot writer does not have: at the defaults its bytes ARE the oracle's writer's, for every case and however the input is handed over; its reader returns the
input for every parameter set; no data chunk holds more plaintext than the block size; without checksums every CRC field is 0; at the constructed ratios the first
chunk is kept, and stored at the double below; its outputs are the recorded ones (tests/golden/snf_params_vectors.json)."""
import importlib.util
import json
import os

import pytest

from tests import common, oracle_lib, snf_params_cases as cases, snf_params_ref as ref


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("record_snf_params_vectors", os.path.join(os.path.dirname(common.HERE), "tools", "record_snf_params_vectors.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def every_input():
    seen = {}
    for block_size in cases.BLOCK_SIZES:
        for name, data in cases.inputs(block_size):
            seen["%s (catalog of %d)" % (name, block_size)] = data
    for name, _, data, _, _ in cases.edge_pairs():
        seen[name] = data
    return seen


def test_model_is_the_oracle_at_the_defaults(o):
    inputs = every_input()
    assert len(inputs) > 100
    for name, data in inputs.items():
        want = o.compress("snappyframed", data)
        assert ref.compress(data, *ref.DEFAULT_PARAMS) == want, name
        assert ref.max_compressed_length(len(data)) == o.max_compressed_length("snappyframed", len(data)), name
    # write() in pieces takes the buffer's ways (:116-141): the bytes do not depend on how the input arrives
    data = cases.data("text", 200000, 99)
    want = o.compress("snappyframed", data)
    for pieces in ((1,), (65535, 1, 1), (65536,), (70000, 70000), (10, 65526, 65536, 3), tuple([9973] * 20)):
        assert ref.compress(data, *ref.DEFAULT_PARAMS, pieces=pieces) == want, pieces
    assert ref.compress(data, True, 4096, 0.85, pieces=(1, 4095, 4097, 10000)) == ref.compress(data, True, 4096, 0.85)


def test_reader_returns_the_input_and_chunks_hold_at_most_a_block():
    for params in cases.parameter_sets():
        checksums, block_size, ratio = params
        for name, data in cases.inputs(block_size):
            stream = cases.expected(params, name)
            plain_lengths = []
            assert ref.decompress(stream, verify_checksums=checksums, plain_lengths=plain_lengths) == data, (params, name)
            assert ref.decompress(stream, verify_checksums=False) == data, (params, name)
            assert all(0 < n <= block_size for n in plain_lengths) and len(plain_lengths) == (len(data) + block_size - 1) // block_size, (params, name)
            assert plain_lengths[:-1] == [block_size] * (len(plain_lengths) - 1), (params, name)
            assert len(stream) <= ref.max_compressed_length(len(data), block_size), (params, name)
            chunks = ref.chunks(stream)
            if not checksums:
                assert all(crc == 0 for _, _, crc, _ in chunks), (params, name)
            if ratio == ref.SMALLEST_RATIO:
                assert all(flag == ref.UNCOMPRESSED_DATA_FLAG for _, flag, _, _ in chunks), (params, name)


def test_a_checksum_free_stream_does_not_verify():
    data = cases.data("text", 5000)
    stream = ref.compress(data, False, 4096, 0.85)
    with pytest.raises(ref.ChecksumError) as e:
        ref.decompress(stream)
    assert e.value.position == 10
    assert ref.decompress(stream, verify_checksums=False) == data


def test_constructed_ratios_sit_on_the_edge():
    pairs = cases.edge_pairs()
    assert len(pairs) >= 3
    for name, block_size, data, kept, raw in pairs:
        assert 0 < raw < kept <= 1.0, name
        for ratio, want_kept in ((kept, True), (raw, False)):
            trace = []
            stream = ref.compress(data, True, block_size, ratio, trace=trace)
            length, compressed, was_kept = trace[0]
            assert was_kept == want_kept and float(compressed) / float(length) == kept, (name, ratio)
            assert ref.chunks(stream)[0][1] == (ref.COMPRESSED_DATA_FLAG if want_kept else ref.UNCOMPRESSED_DATA_FLAG), (name, ratio)
            assert ref.decompress(stream) == data, (name, ratio)


def test_arguments_are_checked_in_the_constructors_order():
    for ratio, text in ((0.0, "0.0"), (-1.0, "-1.0"), (1.5, "1.5"), (float("nan"), "NaN")):
        with pytest.raises(ValueError) as e:
            ref.compress(b"abc", True, 0, ratio)  # (the block size is bad too: the ratio is refused first)
        assert str(e.value) == "minCompressionRatio %s must be between (0,1.0]." % text
    for block_size in (0, -1, 65537):
        with pytest.raises(ValueError) as e:
            ref.compress(b"abc", True, block_size, 0.85)
        assert str(e.value) == "blockSize must be in (0, 65536]"


def test_model_matches_the_recorded_vectors(recorder):
    vectors = recorder.load(os.path.join(common.GOLDEN, "snf_params_vectors.json"))
    assert vectors == json.loads(json.dumps(recorder.vectors()))
    assert sorted(vectors["catalog"]) == sorted(cases.params_name(p) for p in cases.parameter_sets())
    assert sorted(vectors["edge_pairs"]) == sorted(p[0] for p in cases.edge_pairs())
