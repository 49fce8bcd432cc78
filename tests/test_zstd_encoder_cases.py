"""The catalog of constructed Zstd encoder inputs (tests/zstd_encoder_cases.py), held to what it claims, without a GPU: every case reaches the edge it is
named for (the oracle's frame of it, read back by describe(), has the blocks, literals and sequences the case expects, and its sequences rebuild the plaintext),
describe() reads hand-made frames and refuses corrupted ones, and over emulator_cases() the encoder takes every one of its paths (a counting build of the
kernel source on the emulator, every variant) and writes the oracle's bytes."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

from tests import common
from tests import oracle_lib
from tests import zstd_encoder_cases as ze
from tests import zstd_frame_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


def _digest():
    return hashlib.sha256(b"".join(n.encode() + d for n, d, _ in ze.cases())).hexdigest()


def test_catalog_is_deterministic_and_within_its_size():
    cases = ze.cases()
    sizes = [len(d) for _, d, _ in cases]
    assert 150 <= len(cases) <= 500 and sum(sizes) <= 12 << 20
    assert len({name for name, _, _ in cases}) == len(cases)
    assert sum(n > 131072 for n in sizes) <= 24 and sum(n > 1 << 20 for n in sizes) <= 2
    assert sum(n <= 16384 for n in sizes) >= 0.8 * len(cases)
    r = subprocess.run([sys.executable, "-c", "from tests import test_zstd_encoder_cases as t; print(t._digest())"], capture_output=True, text=True, cwd=ROOT, check=True)
    assert r.stdout.strip() == _digest()
    emu = ze.emulator_cases()
    assert sum(len(d) > 131072 for _, d, _ in emu) >= 2  # (multi-block ones)


def test_every_case_reaches_its_edge(o):
    """by the oracle alone.  A case whose property fails is a broken case: the case is repaired, the property stays."""
    broken = []
    for name, data, expect in ze.cases():
        frame = o.compress("zstd", data)
        assert o.decompress("zstd", frame, max(len(data), 1)) == data, name
        why = ze.check(data, frame, expect)
        if why:
            broken.append((name, why))
    assert not broken, "%d cases miss their edge: %r" % (len(broken), broken[:5])


def test_describe_reads_hand_made_frames():
    # the three table kinds, a sequence of each asserted literally.  RLE tables: zc.build_frame
    frame, plain = zc.build_frame(b"abcdefghij" * 3, [(9, 5, -2), (9, 5, -3), (9, 5, -3)], last_literals=3)
    d = ze.describe(frame)
    b, = d["blocks"]
    assert d["content_size"] == len(plain) == 45 and d["single_segment"] and not d["checksum"]
    assert b["modes"] == ("rle", "rle", "rle") and b["sequences"] == [(9, 2, 5), (9, 3, 5), (9, 3, 5)] and b["offsets"] == [4, 8, 1] and b["last_literals"] == 3
    assert b["literals"]["kind"] == "raw" and b["literals"]["regenerated"] == 30 and b["count_form"] == "one byte"
    assert ze.check(plain, frame, {"exact": {0: [(9, 2, 5), (9, 3, 5), (9, 3, 5)]}, "rep": [(2, True), (3, True)], "types": ["compressed"]}) == []
    assert ze.check(plain, frame, {"count": 2}) != [] and ze.check(plain[:-1] + b"!", frame, {}) == [] and ze.check(plain[:9] + b"!" + plain[10:], frame, {}) != []
    # predefined tables: the block 01 (raw literal "A"), one sequence, modes 0; the states are 6 + 5 + 6 bits behind the end mark, LL first.
    # LL state 2 is code 1 of the predefined table (literal length 1), OF state 0 is code 0 (value 1: the repeat offset 1), ML state 1 is code 1 (length 4)
    bits = (1 << 17) | (2 << 11) | (0 << 6) | 1  # end mark, LL state, OF state, ML state -- no extra bits
    block = bytes([1 << 3, 65, 1, 0]) + bits.to_bytes(3, "little")
    frame = b"\x28\xb5\x2f\xfd" + bytes([0x20, 5]) + ((len(block) << 3) | 5).to_bytes(3, "little") + block
    table = ze.fse_decode_table(*ze.LL_DEFAULT)
    assert table[2][0] == 1 and ze.fse_decode_table(*ze.OF_DEFAULT)[0][0] == 0 and ze.fse_decode_table(*ze.ML_DEFAULT)[1][0] == 1
    b, = ze.describe(frame)["blocks"]
    assert b["modes"] == ("predefined",) * 3 and b["sequences"] == [(1, 1, 4)] and b["offsets"] == [1]
    assert ze.check(b"AAAAA", frame, {"exact": {0: [(1, 1, 4)]}}) == []
    # an FSE table for the offsets: accuracy log 5, codes 0 and 2 with 16 of 32 states each (its description written by _write_description below)
    counts = [16, 0, 16]
    desc = _write_description(counts, 5)
    assert ze.read_fse_description(desc, 0, len(desc), 8, 31)[:2] == (counts, 5)
    states = ze.fse_decode_table(counts, 5)
    s2 = next(i for i, (sym, _, _) in enumerate(states) if sym == 2)
    bits = (1 << (6 + 5 + 6 + 2)) | (2 << 13) | (s2 << 8) | (1 << 2) | 1  # end mark, LL state 2, OF state, ML state 1, two extra offset bits: value 4 + 1
    block = bytes([2 << 3, 65, 66, 1, 0x20]) + desc + bits.to_bytes(3, "little")
    frame = b"\x28\xb5\x2f\xfd" + bytes([0x20, 6]) + ((len(block) << 3) | 5).to_bytes(3, "little") + block
    b, = ze.describe(frame)["blocks"]
    assert b["modes"] == ("predefined", "fse", "predefined") and b["sequences"] == [(1, 5, 4)] and b["offsets"] == [2] and b["tables"]["of"]["counts"] == counts
    assert ze.check(b"ABBBBB", frame, {}) != [] and ze.check(b"AAAAAB", frame, {}) != []  # (offset 2 behind one literal: before the start)
    # corrupted frames are refused
    good, plain = zc.build_frame(b"abcdefghij" * 3, [(9, 5, -2), (9, 5, -3), (9, 5, -3)], last_literals=3, checksum=True)
    assert ze.describe(good)["checksum"]
    for bad in (good[:-1], good + b"\0", b"\x29" + good[1:], good[:5] + bytes([good[5] + 1]) + good[6:], good[:-5] + b"\0" + good[-4:],
                good[:4] + bytes([good[4] | 8]) + good[5:], good[:6] + bytes([good[6] | 6]) + good[7:]):
        with pytest.raises(ze.Malformed):
            ze.describe(bad)


def _write_description(counts, log):
    """an FSE table description from its counts (RFC 8878 4.1.1), for the reader's test"""
    acc, n = log - 5, 4
    remaining, i = 1 << log, 0
    while remaining > 0:
        c = counts[i]
        bits = (remaining + 1).bit_length()
        lower, threshold = (1 << (bits - 1)) - 1, (1 << bits) - 1 - (remaining + 1)
        v = c + 1
        if v < threshold:
            acc |= v << n
            n += bits - 1
        else:
            acc |= (v + threshold if v > lower else v) << n
            n += bits
        remaining -= abs(c)
        i += 1
        if c == 0:
            run = 0
            while counts[i + run] == 0:
                run += 1
            i += run
            while run >= 3:
                acc |= 3 << n
                n += 2
                run -= 3
            acc |= run << n
            n += 2
    return acc.to_bytes((n + 7) // 8, "little")


# Counters that no input raises: said here with the argument, and asserted to stay zero.
UNREACHABLE = {
    65: "RLE literals come behind `literalsSize <= 63 -> raw`: at 64 and more literals the header has two or three bytes",
    105: "offset codes are highest_bit(offset + 3) with offset < the window of 2^20: at most 20, predefined offsets are always allowed",
}
# Reachable in principle, not reached by any input built so far (what was tried: profiles/zstd_encoder_edges.md).  These two names and no others.
NOT_REACHED = {
    118: "the three-byte sequence count needs 32 512 sequences in a block of 131 072 bytes: at most four bytes a sequence",
    112: "fse_normalize_counts2",
}
VARIANTS = (3, 0, 1, 2)
# the match-finder counters that belong to one family of variants: the window finder (3) and the position-by-position one (0, 1, 2; 1 probes serially)
WINDOW_FINDER = set(range(0, 17))
BATCH_PROBE, SERIAL_PROBE = {17, 19}, {18}
# the three-byte RLE literals header and the FSE table logs at their maximum: only ze.EMULATOR_MANY_SEQUENCES get there, under the default variant and variant 1
MANY_SEQUENCES_ONLY = {67, 108}


def test_every_encoder_path_is_reached():
    """emulator_cases(v) through the four variants of a -DACHIP_HOST_STATS build, side by side: the oracle's bytes for every entry, and every counter raised by
    some entry under the default variant -- the match finder's under the variant they belong to, the others under every variant but for the two that only
    the cases of thousands of sequences raise (left out under variants 0 and 2)."""
    jobs = common.emulator_checks(["enc_stats"], {v: ("enc_paths.py", "zstd", "catalog", "--json", "--option", str(v)) for v in VARIANTS}, merge=False)  # (side by side)
    import enc_paths
    names = enc_paths.COUNTERS["zstd"]
    assert set(UNREACHABLE) | set(NOT_REACHED) <= set(names) and set(NOT_REACHED) <= {112, 118}
    for v, job in jobs.items():
        out, err = job.stdout, job.stderr
        assert job.returncode == 0, err
        results = json.loads(out.strip().splitlines()[-1])
        assert len(results) == len(ze.emulator_cases(v)) > 120
        differ = [name for name, ok, _ in results if not ok]
        assert not differ, "variant %d differs from the oracle on %r" % (v, differ[:10])
        for k, what in names.items():
            first = next((name for name, _, c in results if c[str(k)]), None)
            total = sum(c[str(k)] for _, _, c in results)
            print("variant %d  %3d %-52s %7d  first: %s" % (v, k, what, total, first))
            if k in UNREACHABLE or k in NOT_REACHED:
                assert total == 0, "counter %d (%s) is reached after all, by %r: assert it" % (k, what, first)
            elif k in WINDOW_FINDER:
                assert (total > 0) == (v == 3), "variant %d, counter %d (%s): %d" % (v, k, what, total)
            elif k in SERIAL_PROBE:
                assert total > 0 or v not in (0, 1, 2), "variant %d never probes a single position" % v
                assert v != 1 or sum(c["17"] for _, _, c in results) == 0, "variant 1 took a batch probe"
            elif k in BATCH_PROBE:
                assert (total > 0) == (v != 1), "variant %d, counter %d (%s): %d" % (v, k, what, total)
            elif k in MANY_SEQUENCES_ONLY and v in (0, 2):
                assert total == 0  # (raised only by the cases of thousands of sequences, which these two variants leave out: emulator_cases(v))
            else:
                assert total > 0, "no catalog entry reaches counter %d under variant %d: %s" % (k, v, what)
