"""Checks on the entropy-stage catalog of tests/zstd_entropy_cases.py itself (no GPU): the edges it promises, recounted from the frames' bytes by the reader at the
end of that module; the oracle's verdict (the Java decoder: the project's contract) and libzstd's on every case; the states of every named table visited; sizes."""
import os
import subprocess

import pytest

from tests import oracle_lib, zstd_entropy_cases as ze, zstd_frame_cases as zc
from tests.oracle_lib import OracleError


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


@pytest.fixture(scope="module")
def cases():
    return ze.entropy_catalog()


def test_the_table_model_rebuilds_the_predefined_tables_and_the_writer_round_trips(cases):
    # RFC 8878 appendix A: rows of the three predefined decoding tables (symbol, number of bits, baseline)
    ll, of, ml = (ze.fse_decode_table(*ze.PREDEFINED[k]) for k in range(3))
    assert ll[0] == (0, 4, 0) and ll[1] == (0, 4, 16) and ll[2] == (1, 5, 32) and ll[22] == (0, 4, 32) and ll[60] == (35, 6, 0) and ll[63] == (32, 6, 0)
    assert of[0] == (0, 5, 0) and of[1] == (6, 4, 0) and of[2] == (9, 5, 0) and of[27] == (28, 5, 0) and of[31] == (24, 5, 0)
    assert ml[0] == (0, 6, 0) and ml[1] == (1, 4, 0) and ml[2] == (2, 5, 32) and ml[57] == (52, 6, 0) and ml[63] == (46, 6, 0)
    # every description the catalog writes reads back as the counts it was written from
    assert len(ze.TABLES) >= 150
    for key, (kind, norm, log) in ze.TABLES.items():
        raw, _ = ze.fse_description(norm, log)
        d = ze.read_fse_description(raw + bytes(8), 0, 255 if kind == "W" else ze.MAX_SYMBOL[kind])
        assert d is not None and d["log"] == log and d["norm"] == list(norm) and d["bytes"] == len(raw), key
    # the block executor here and the execute-stage catalog's agree
    out = bytearray()
    assert ze.execute_block(out, [1, 4, 8], b"abcdefgh", [(3, 5, 5), (2, 4, 1), (1, 3, 2)])
    assert bytes(out) == zc.execute(b"abcdefgh", [(3, 5, 2), (2, 4, -1), (1, 3, -2)])[0]


def test_the_oracle_on_every_case(o, cases):
    """The expected status, offset and bytes of every case are the oracle's.  The Python model (RFC 8878) must agree with it on every case it calls valid; where it
    calls a case valid that the Java decoder refuses, the case says so (`differs`, tag java-differs) and expects the refusal."""
    for c in cases:
        for pad in (0, 64):
            cap = c.capacity(pad)
            if c.malformed:
                with pytest.raises(OracleError):
                    o.decompress("zstd", c.frame, cap)
            else:
                assert o.decompress("zstd", c.frame, cap) == c.plain == c.model_plain, c.name
        if "java-differs" in c.tags:
            assert c.malformed and c.model_plain is not None and c.differs and c.name in ze.KNOWN_DIFFERENCES, c.name
    assert all(c.differs for c in cases if c.name in ze.KNOWN_DIFFERENCES) and {c.name for c in cases if c.differs} == set(ze.KNOWN_DIFFERENCES)


def test_libzstd_on_every_valid_case(cases):
    """libzstd (pyarrow's) must agree on every valid case it accepts, and may refuse only cases that say so"""
    pa = pytest.importorskip("pyarrow")
    codec = pa.Codec("zstd")
    for c in cases:
        if c.malformed:
            continue
        try:
            got = codec.decompress(c.frame, decompressed_size=max(c.cap, 1)).to_pybytes()
        except Exception:
            assert c.differs and "libzstd" in c.differs, c.name
            continue
        assert got == c.plain, c.name
        assert not c.differs, c.name  # (a note that no longer holds)


def test_every_edge_occurs(cases):
    found = {}
    for c in cases:
        if not c.malformed:
            for t in ze.scan_item(c.frame):
                found[t] = found.get(t, 0) + 1
    missing = [t for t in ze.required_scan_tags() if t not in found]
    assert not missing, missing
    own = {}
    for c in cases:
        if not c.malformed:
            for t in c.tags:
                own[t] = own.get(t, 0) + 1
    missing = [t for t in ze.required_case_tags() if t not in own]
    assert not missing, missing
    bad = set().union(*(c.tags for c in cases if c.malformed))
    missing = [t for t in ze.REQUIRED_MALFORMED if t not in bad]
    assert not missing, missing
    for kind in ("LL", "OF", "ML"):
        assert sum(1 for c in cases if "random-table" in c.tags and "table=" + kind in c.tags) >= 40, kind
        for t in ze.MALFORMED_TABLES:
            assert any(c.malformed and t in c.tags and "table=" + kind in c.tags for c in cases), (kind, t)
    # the cases that leave the pipeline by design: Huffman log 12, more than one frame in an item, four streams with overlapping segments -- and nothing else
    assert sorted(c.name for c in cases if c.fallback) == ["huf-four-streams-1-overlap", "huf-four-streams-2-overlap", "huf-four-streams-5-overlap", "huf-log-12", "two-frames"]


def test_every_state_of_every_named_table_is_visited(cases):
    cov = ze.state_coverage(cases)
    named = {k: v for k, v in cov.items() if k.split("/")[0] in ("LL", "OF", "ML")}
    assert len(named) >= 30
    for key, (visited, usable, total) in named.items():
        assert visited == usable, (key, visited, usable, total)
    # tables with symbols no small frame can use (offset codes above 18) are there, and their other states are all visited
    assert sum(1 for v, u, t in named.values() if u < t) >= 3
    for family in ("random/LL", "random/OF", "random/ML"):
        v = sum(x[0] for k, x in cov.items() if k.startswith(family))
        u = sum(x[1] for k, x in cov.items() if k.startswith(family))
        assert v >= 0.8 * u, (family, v, u)


def test_frames_are_small_and_generated(cases):
    assert 300 <= len(cases) <= 600
    assert max(len(c.frame) for c in cases) <= 100000 and sum(len(c.frame) for c in cases) <= 1 << 20
    assert max(c.cap for c in cases) <= 420000 and sum(c.cap for c in cases if not c.malformed) <= 24 << 20
    assert len({c.name for c in cases}) == len(cases)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tracked = subprocess.run(["git", "ls-files", "tests/golden"], cwd=root, capture_output=True, text=True)
    if tracked.returncode == 0:
        assert not [f for f in tracked.stdout.split() if "entropy" in f]
