#!/usr/bin/env python3
"""Writes tests/golden/lz4_accel_vectors.json: length and SHA-256 of what the pure-Python LZ4 encoder with acceleration (tests/lz4_accel_ref.py) makes of every
input of tests/lz4_accel_cases.py at every acceleration the tests use -- blocks, and frames at the frame test's accelerations.  The file pins the model: the GPU
tests take their expected bytes from it, so a change to the model that changes an output has to show here (tests/test_lz4_accel_ref.py compares).
Run after a deliberate change to the model or the cases:   python tools/record_lz4_accel_vectors.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import lz4_accel_cases as cases, lz4_accel_ref as ref  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "lz4_accel_vectors.json")


def entry(data, out):
    return {"input_length": len(data), "input_sha256": hashlib.sha256(data).hexdigest(), "length": len(out), "sha256": hashlib.sha256(out).hexdigest()}


def vectors():
    blocks = {name: {str(a): entry(data, ref.compress(data, a)) for a in cases.ACCELERATIONS} for name, data in cases.block_cases()}
    frames = {name: {str(a): entry(data, ref.compress_frame(data, a)) for a in cases.FRAME_ACCELERATIONS} for name, data in cases.frame_cases()}
    return {"block": blocks, "frame": frames}


if __name__ == "__main__":
    with open(PATH, "w") as f:
        json.dump(vectors(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s" % PATH)
