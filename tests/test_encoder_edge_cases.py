"""The catalog of constructed encoder inputs (tests/encoder_edge_cases.py), held to what it claims, without a GPU:
every case reaches the edge it is named for (the oracle's stream of it, parsed, has the sequences the case expects), and over the catalog the LZ4 and Snappy
window encoders take every one of their paths (a counting build of the kernel source on the emulator) and write the oracle's bytes."""
import json
import os
import subprocess
import sys

import pytest

from tests import encoder_edge_cases as ec
from tests import common
from tests import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


def test_filler_has_no_repeated_4_gram():
    pool = ec._filler_pool()
    assert len({pool[i:i + 4] for i in range(len(pool) - 3)}) == len(pool) - 3 and 0 not in pool


def test_catalog_is_deterministic_and_small():
    for codec in ("lz4", "snappy"):
        cases = ec.cases(codec)
        assert 200 <= len(cases) <= 700 and sum(len(d) for _, d, _ in cases) <= 4 << 20
        assert len({name for name, _, _ in cases}) == len(cases)
        assert sum(len(d) > 65536 for _, d, _ in cases) <= 40 and sum(len(d) <= 4096 for _, d, _ in cases) >= 0.9 * len(cases)
    r = subprocess.run([sys.executable, "-c", "import hashlib; from tests import encoder_edge_cases as ec; print(hashlib.sha256(b''.join(d for c in ('lz4', 'snappy') for _, d, _ in ec.cases(c))).hexdigest())"],
                       capture_output=True, text=True, cwd=ROOT, check=True)
    import hashlib
    assert r.stdout.strip() == hashlib.sha256(b"".join(d for c in ("lz4", "snappy") for _, d, _ in ec.cases(c))).hexdigest()


@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_every_case_reaches_its_edge(o, codec):
    """2a: by the oracle alone.  A case whose property fails is a broken case: the case is repaired, the property stays."""
    broken = []
    for name, data, expect in ec.cases(codec):
        stream = o.compress(codec, data)
        if len(data):
            assert o.decompress(codec, stream, len(data)) == data, name
        why = ec.check(codec, data, stream, expect)
        if why:
            broken.append((name, why))
    assert not broken, "%d cases miss their edge: %r" % (len(broken), broken[:5])


def test_the_parsers_read_hand_made_streams():
    assert ec.lz4_parse(bytes([0x11, 97, 1, 0, 0x50, 1, 2, 3, 4, 5])) == [(1, 1, 5), (5, 0, 0)]
    assert ec.lz4_parse(bytes([0xFF, 0]) + bytes(15) + bytes([7, 0, 255, 4]) + bytes([0x00])) == [(15, 7, 15 + 255 + 4 + 4), (0, 0, 0)]
    assert ec.snappy_parse(bytes([20, 0 << 2, 97, 1 | (7 << 2) | (7 << 5), 0xFF, 2 | (7 << 2), 1, 0])) == (20, [("L", 1), ("C1", 2047, 11), ("C2", 1, 8)])
    assert ec.snappy_parse(bytes([0x80, 1, 60 << 2, 60]) + bytes(61)) == (128, [("L", 61)])
    assert ec.check("lz4", bytes(20), bytes([0x1A, 0, 1, 0, 0x50, 0, 0, 0, 0, 0]), {"has": [[(1, 1, None)]], "last": 5, "count": 1, "max_offset": 1, "none": [(None, 2, None)]}) == []
    assert ec.check("lz4", bytes(20), bytes([0x1A, 0, 1, 0, 0x50, 0, 0, 0, 0, 0]), {"last": 6, "max_offset": 0}) != []


# (Nothing is exempt for its size: the entries beyond 20 000 bytes that raise a counter of their own -- the catch-up of 64 and 65 bytes, the wide table, the
# sub-block boundary -- are filler and runs, which the emulator finishes in a fraction of a second; see encoder_edge_cases.emulator_cases.)
# Counters that no input raises: said here with the argument instead of asserted.
UNREACHABLE = {
    ("lz4", 30): "the window's catch-up has at most input - anchor bytes of room, anchor >= base and input <= base + 63: its loop ends in its first trip of 64 lanes "
                 "(the most a window's catch-up reaches, 60 and 61 bytes, are catalog entries; 64 and more are found by the batch-probe step: counter 34)",
    ("snappy", 52): "a copy takes the scalar way when the registers cannot measure it -- the candidate's 16 bytes were not loaded (then okB is false), or the copy starts in "
                    "the last four lanes or within 12 bytes of the block's end (then a0 + 8 bytes are not in the window: okA is false) -- so the scalar way always counts from memory",
}
VARIANTS = [("lz4", 4), ("lz4", 4 | 16), ("lz4", 4 | 48), ("snappy", 4)]


def test_every_encoder_path_is_reached():
    """2b: the catalog entries the emulator takes (all but 64 KiB and more of mixed data) through the window encoders (variant 4; LZ4 also as a wavefront per block and with two memory-tier wavefronts)
    built with -DACHIP_HOST_STATS: the oracle's bytes for every entry, and every counter raised by some entry -- LZ4's 20 .. 26 without exception."""
    jobs = common.emulator_checks(["enc_stats"], {v: ("enc_paths.py", v[0], "catalog", "--json", "--option", str(v[1])) for v in VARIANTS}, merge=False)  # (side by side)
    import enc_paths
    for (codec, option), job in jobs.items():
        out, err = job.stdout, job.stderr
        assert job.returncode == 0, err
        results = json.loads(out.strip().splitlines()[-1])
        assert len(results) == len(ec.emulator_cases(codec)) > 200
        differ = [name for name, ok, _ in results if not ok]
        assert not differ, "%s variant %d differs from the oracle on %r" % (codec, option, differ[:10])
        for k, what in enc_paths.COUNTERS[codec].items():
            first = next((name for name, _, c in results if c[str(k)]), None)
            total = sum(c[str(k)] for _, _, c in results)
            print("%-6s option %2d  %2d %-46s %7d  first: %s" % (codec, option, k, what, total, first))
            if (codec, k) in UNREACHABLE:
                assert not (codec == "lz4" and 20 <= k <= 26)
                assert total == 0, "counter %d (%s) is reached after all, by %r: assert it" % (k, what, first)
            else:
                assert total > 0, "no catalog entry reaches counter %d of %s: %s" % (k, codec, what)
