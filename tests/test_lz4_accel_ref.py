"""The pure-Python LZ4 encoder with acceleration (tests/lz4_accel_ref.py), the reference of the GPU tests at accelerations the oracle does not have: at
acceleration 1 it IS the oracle's encoder, byte for byte; at every acceleration its output decodes back through the oracle and stays inside the bound; its outputs
are the recorded ones (tests/golden/lz4_accel_vectors.json); the closed forms of the probe schedule the kernels compute per lane are the loop's running sums; its
frame writer is the oracle's at acceleration 1."""
import hashlib
import json
import os

import pytest

from tests import common, encoder_edge_cases, lz4_accel_cases as cases, lz4_accel_ref as ref, oracle_lib


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


@pytest.fixture(scope="module")
def vectors():
    return json.load(open(os.path.join(common.GOLDEN, "lz4_accel_vectors.json")))


def test_model_is_the_oracle_at_acceleration_1(o):
    text = cases.alice() + cases.book()
    inputs = [(name, data) for name, data, _ in encoder_edge_cases.cases("lz4")]
    inputs += [("text of %d bytes" % n, text[:n]) for n in (0, 1, 12, 13, 14, 64, 4096, 65536, 65537)]
    inputs += [(name, data) for name, data in cases.block_cases()]
    assert len(inputs) > 60
    for name, data in inputs:
        assert ref.compress(data, 1) == o.compress("lz4", data), name


def test_model_output_decodes_and_stays_inside_the_bound(o):
    for name, data in cases.block_cases():
        for a in cases.ACCELERATIONS:
            c = cases.expected(name, a)
            assert len(c) <= ref.max_compressed_length(len(data)) == o.max_compressed_length("lz4", len(data)), (name, a)
            assert o.decompress("lz4", c, len(data)) == data, (name, a)


def test_model_matches_the_recorded_vectors(vectors):
    assert sorted(vectors["block"]) == sorted(n for n, _ in cases.block_cases()) and sorted(vectors["frame"]) == sorted(n for n, _ in cases.frame_cases())
    for kind, inputs, fn, accelerations in (("block", cases.block_cases(), ref.compress, cases.ACCELERATIONS), ("frame", cases.frame_cases(), ref.compress_frame, cases.FRAME_ACCELERATIONS)):
        for name, data in inputs:
            assert sorted(vectors[kind][name], key=int) == [str(a) for a in accelerations]
            for a in accelerations:
                e = vectors[kind][name][str(a)]
                assert (len(data), hashlib.sha256(data).hexdigest()) == (e["input_length"], e["input_sha256"]), (kind, name, "the input changed")
                out = fn(data, a)
                assert (len(out), hashlib.sha256(out).hexdigest()) == (e["length"], e["sha256"]), (kind, name, a)


def test_the_parameter_shows_on_text_and_not_on_noise(vectors):
    # the sizes the issue quotes for the first 64 KiB of alice29.txt; random bytes and zeros give the same bytes at every acceleration
    sizes = [vectors["block"]["alice 64 KiB"][str(a)]["length"] for a in (1, 2, 4, 8, 16, 64)]
    assert sizes == [40284, 42538, 46968, 53264, 59277, 64910]
    for name in ("random 8 KiB", "zeros 5000"):
        assert len({vectors["block"][name][str(a)]["sha256"] for a in cases.ACCELERATIONS}) == 1


def test_closed_forms_of_the_probe_schedule():
    for a in (1, 2, 3, 7, 64, 65537):
        # the loop itself: step and findMatchAttempts as Lz4RawCompressor.java:113-125 moves them
        attempts, step, offset = a << ref.SKIP_TRIGGER, 1, 0
        for m in range(700):
            assert ref.scan_offset(m, a) == offset, (a, m)
            assert ref.scan_advance(m, a) == step, (a, m)
            offset += step
            step = attempts >> ref.SKIP_TRIGGER
            attempts += 1
            # the form the kernels use (lz4_compress_body.h): the schedule of acceleration 1 plus a - 1 per advance from the second probe on
            assert ref.scan_offset(m, a) == (0 if m == 0 else ref.scan_offset(m, 1) + (m - 1) * (a - 1))
        # the window encoder's pattern: the probes among the first 64 positions of a search
        assert ref.probe_pattern(a) == sum(1 << ref.scan_offset(m, a) for m in range(64) if ref.scan_offset(m, a) < 64)


def test_acceleration_range():
    for bad in (0, -1, 65538):
        with pytest.raises(ValueError, match=r"LZ4 acceleration should be in the \[1, 65537\] range but got %d" % bad):
            ref.compress(b"x" * 20, bad)
    assert ref.compress(b"x" * 20, 65537)


def test_frame_writer_is_the_oracle_at_acceleration_1(o):
    for name, data in cases.frame_cases():
        assert ref.compress_frame(data, 1) == o.compress("lz4frame", data), name
        for a in cases.FRAME_ACCELERATIONS:
            f = ref.compress_frame(data, a)
            assert o.decompress("lz4frame", f, len(data)) == data, (name, a)
