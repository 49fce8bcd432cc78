"""The catalog of constructed decoder streams (tests/decoder_edge_cases.py), held to what it claims, without a GPU: it is deterministic and small, the
oracle decodes every valid case to the builder's own plaintext and refuses every malformed one (as the reference's decoders do, where oracle/_ref/libref.so
is there), every label of every ring configuration is reached by a targeted case and by a grammar case, and the configuration table is the one the two launch
tables hold.  The emulator run of the catalog is a job of tests/test_host_logic.py::test_lane_private_decoder_kernels_on_the_cpu
(tools/hostemu/check_v3.py --part edges)."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import pytest

from tests import decoder_edge_cases as dc
from tests import oracle_lib
from tests.oracle_lib import OracleError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODECS = ("lz4", "snappy")
ALL = [(codec, config) for codec in CODECS for config in dc.CONFIGS[codec]]

DIGEST = ("import hashlib; from tests import decoder_edge_cases as dc; h = hashlib.sha256()\n"
          "for codec in ('lz4', 'snappy'):\n"
          "    for config in dc.CONFIGS[codec]:\n"
          "        for c in dc.cases(codec, config): h.update(c.plain + c.stream)\n"
          "        for m in dc.malformed(codec, config): h.update(m[2])\n"
          "print(h.hexdigest())")


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


def test_builders_write_hand_checked_streams():
    assert dc.lz4_stream([], 3) == (dc._filler(0, 3), bytes([0x30]) + dc._filler(0, 3))
    f = dc._filler(0, 14)
    assert dc.lz4_stream([(2, 6, 1)], 12) == (f[:2] + f[1:2] * 6 + f[2:14], bytes([0x22]) + f[:2] + bytes([1, 0, 0xC0]) + f[2:14])
    plain, s = dc.lz4_stream([(15, 19, 3), (270, 274, 300)], 12)
    assert s[:2] == bytes([0xFF, 0]) and s[17:21] == bytes([3, 0, 0]) + bytes([0xFF]) and s[21:24] == bytes([0xFF, 0]) + plain[34:35] and len(plain) == 15 + 19 + 270 + 274 + 12
    assert plain[15:34] == (plain[12:15] * 7)[:19] and plain[304:578] == plain[4:278]
    f = dc._filler(0, 61)
    plain, s = dc.snappy_stream([(61, 70, 5, {"cut": 60, "copy": [2, 4]})])
    assert s == dc.varint(131) + bytes([60 << 2, 60]) + f + bytes([2 | (59 << 2), 5, 0]) + bytes([3 | (9 << 2), 5, 0, 0, 0]) and plain == f + (f[56:] * 14)
    assert dc.snappy_pieces(140, 9, {}) == [(64, 2), (64, 2), (12, 2)] and dc.snappy_pieces(11, 2047, {"copy": 1}) == [(11, 1)] and dc.snappy_pieces(8, 70000, {"copy": 1}) == [(8, 4)]
    assert dc.snappy_stream([(3, 0, 0, {"lit": 4})])[1] == bytes([3, 63 << 2, 2, 0, 0, 0]) + f[:3]
    pool = dc._filler(0, 1 << 19)
    assert 0 not in pool and len({pool[i:i + 4] for i in range(0, 1 << 16)}) > 65500  # filler: a wrong source byte shows


def test_catalog_is_deterministic_and_within_its_sizes():
    h = hashlib.sha256()
    for codec, config in ALL:
        cfg = dc.CONFIGS[codec][config]
        cases = dc.cases(codec, config)
        assert len({c.name for c in cases}) == len(cases)
        assert sum(len(c.plain) for c in cases) <= 4 << 20, (codec, config)
        for c in cases:
            far = any(s[2] >= 65535 for s in c.seqs)
            limit = 262144 if far and config != dc.LATENCY else dc.size_limit(cfg)
            assert len(c.plain) <= limit, (codec, config, c.name, len(c.plain))
            h.update(c.plain + c.stream)
        assert sum(c.kind == "targeted" for c in cases) >= 200 and sum(c.kind == "grammar" for c in cases) >= 6
        for m in dc.malformed(codec, config):
            h.update(m[2])
    r = subprocess.run([sys.executable, "-c", DIGEST], capture_output=True, text=True, cwd=ROOT, check=True)
    assert r.stdout.strip() == h.hexdigest()


def test_configs_derive_chunk_and_reach():
    for codec in CODECS:
        for cfg in dc.CONFIGS[codec].values():
            assert cfg.CHUNK == 16 * cfg.GS * cfg.GPL and cfg.LDS_REACH == cfg.OUT_RING - cfg.CHUNK - 16
            assert cfg.IN_RING >= 2 * cfg.CHUNK and cfg.OUT_RING >= 4 * cfg.CHUNK  # (achip_rings.h's static_asserts)


def launch_table(source, function, launcher, latency_kernel):
    """{(lanes, ring class): (GS, GPL, IN_RING, OUT_RING, PHASED)} read from the text of a ring decoder's launch function"""
    src = open(os.path.join(ROOT, "aircompressor_amd", "csrc", source)).read()
    body = src[src.index("hipError_t %s(" % function):]
    body = body[:body.index("\n}\n")]

    def row(args):
        a = [int(x) for x in args.split(",")]
        gs, in_ring, out_ring, gpl, phased = a + [1, 0][len(a) - 3:]  # template <GS, IN_RING, OUT_RING, GPL = 1, PHASED = 0>
        return (gs, gpl, in_ring, out_ring, phased)
    rows = {}
    lat = re.search(r"%s<(\d+), (\d+)>" % latency_kernel, body)
    kernel = src[src.index("void %s(" % latency_kernel):]
    rings = re.search(r"(?:Rings|snappy_buffer_decode)<(\d+), IN_RING, OUT_RING, (\d+)[,>]", kernel)  # the lanes and granules per lane of the latency kernel's rings
    rows[(4, 3)] = (int(rings.group(1)), int(rings.group(2)), int(lat.group(1)), int(lat.group(2)), 0)
    outer = None
    for line in body.splitlines():
        line = line.split("//")[0]
        m = re.match(r"\s*(?:case (\d+)|default):(.*)", line)
        if not m:
            continue
        label = int(m.group(1)) if m.group(1) else None
        launches = re.findall(r"%s<([\d, ]+)>" % launcher, m.group(2))
        if len(launches) == 2:    # return ringClass ? <class 1> : <class 0>   (default: 16 lanes)
            lanes = label if label is not None else 16
            rows[(lanes, 1)], rows[(lanes, 0)] = row(launches[0]), row(launches[1])
            outer = None
        elif len(launches) == 1:  # inside the 4-lane switch over the ring class (default: class 0)
            rows[(outer, label if label is not None else 0)] = row(launches[0])
        else:
            outer = label
    return rows


@pytest.mark.parametrize("codec, source, function, launcher, kernel", [
    ("lz4", "lz4_decompress_v2.hip", "launch_lz4_decompress_rings", "lz4d2_launch", "lz4_decompress_latency_kernel"),
    ("snappy", "snappy_decompress_v2.hip", "launch_snappy_decompress_rings", "snd2_launch", "snappy_decompress_latency_kernel")])
def test_configs_equal_the_launch_tables(codec, source, function, launcher, kernel):
    """a ring size or lane count that changes in a launch table without the catalog following fails here (the text of the C++ launch functions, nothing compiled)"""
    table = launch_table(source, function, launcher, kernel)
    ours = {k: (c.GS, c.GPL, c.IN_RING, c.OUT_RING, c.phased) for k, c in dc.CONFIGS[codec].items()}
    assert table == ours, {k: (table.get(k), ours.get(k)) for k in set(table) | set(ours) if table.get(k) != ours.get(k)}
    assert len(table) == 16


class _Ref:
    """the reference's own decoders (oracle/_ref/libref.so, as tests/test_ref_pin.py loads it)"""

    def __init__(self):
        from tests import test_ref_pin
        if os.path.isdir(test_ref_pin.REFERENCE):
            subprocess.run(["make", "-s", "-C", test_ref_pin.REF_DIR], check=True)
        self.ref = test_ref_pin.Ref(ctypes.CDLL(test_ref_pin.LIB)) if os.path.exists(test_ref_pin.LIB) else None


@pytest.fixture(scope="module")
def ref():
    return _Ref().ref


@pytest.mark.parametrize("codec, config", ALL, ids=lambda v: str(v).replace(" ", ""))
def test_oracle_decodes_every_valid_case_and_refuses_every_malformed_one(o, codec, config):
    for c in dc.cases(codec, config):
        for cap in (len(c.plain), len(c.plain) + 9):
            assert o.decompress(codec, c.stream, cap) == c.plain, (c.name, cap)
    for name, condition, stream, cap in dc.malformed(codec, config):
        with pytest.raises(OracleError):
            o.decompress(codec, stream, cap)


@pytest.mark.parametrize("codec", CODECS)
def test_reference_decoders_agree_on_the_catalog(o, ref, codec):
    """the transliterated reference decoder: the same plaintext, and on the malformed cases the same kind of failure at the same offset"""
    if ref is None:
        pytest.skip("oracle/_ref/libref.so absent and the reference is not here to build it from")
    for config in ((4, 0), (16, 0), (64, 1), dc.LATENCY):
        for c in dc.cases(codec, config):
            r, out, _, msg = ref.decompress(codec, c.stream, len(c.plain))
            assert r == len(c.plain) and out == c.plain, (config, c.name, r, msg)
        for name, condition, stream, cap in dc.malformed(codec, config):
            with pytest.raises(OracleError) as e:
                o.decompress(codec, stream, cap)
            r, _, off, msg = ref.decompress(codec, stream, cap)
            if e.value.cls == 2:
                assert r == -2, (config, name, r, msg)
            else:
                assert r == -1 and off == e.value.offset, (config, name, r, off, msg, str(e.value))


@pytest.mark.parametrize("codec", CODECS)
def test_every_label_is_reached_by_a_targeted_case_and_by_a_grammar_case(codec):
    cells = unreachable = 0
    for config in dc.CONFIGS[codec]:
        names = dc.label_names(codec, config)
        assert len(set(names)) == len(names)
        reached = {"targeted": set(), "grammar": set()}
        for c in dc.cases(codec, config):
            got = dc.labels(c, codec, config)
            assert got <= set(names), (config, c.name, got - set(names))
            reached[c.kind] |= got
        excused = {label for (cc, cf, label) in dc.UNREACHABLE if cc == codec and cf == config}
        assert excused <= set(names)
        cells += len(names)
        unreachable += len(excused)
        for kind in ("targeted", "grammar"):
            missing = [n for n in names if n not in reached[kind] and n not in excused]
            assert not missing, "%s %r: no %s case reaches %r" % (codec, config, kind, missing)
        assert not (excused & (reached["targeted"] | reached["grammar"])), "declared unreachable and reached: assert it instead"
    assert all(len(why) > 40 for why in dc.UNREACHABLE.values())
    assert unreachable * 20 <= cells, (unreachable, cells)


def test_labels_of_hand_made_cases():
    cfg = dc.CONFIGS["lz4"][(16, 0)]  # CHUNK 256, OUT_RING 1024, LDS_REACH 752
    case = lambda seqs, tail=13: dc.Case("x", "targeted", seqs, tail, None, None)
    got = dc.labels(case([(1040, 256 + 17, 256 + 3), (0, 65, 752)]), "lz4", (16, 0))
    assert {"off:REACH+0", "band-after:dwords-head0", "ml:4GS+1/plain", "lit:0", "op%16=0", "wrap:src"} <= got and "band-after:small" not in got
    got = dc.labels(case([(1024 + 255, 4, 9), (0, 64, 769)]), "lz4", (16, 0))
    assert {"band-after:small", "off:REACH+17", "ml:4/plain", "ml:4GS/plain", "op%CHUNK=CHUNK-1", "off:9"} <= got
    got = dc.labels(case([(2040, 20, 1024)]), "lz4", (16, 0))
    assert "wrap:both" in got and "off:RING+0" in got and "ml:4/plain" not in got
    # the first sequence is 1 + 1 + 251 + 2 = 255 bytes: the second token at 255, its two length bytes at 256 and 257 -- with input base 15 they lie on both sides of 272 - 15
    assert "lz4:lit-chain-straddles-refill" not in dc.labels(case([(251, 4, 1), (270, 4, 1)]), "lz4", (16, 0))
    assert "lz4:lit-chain-straddles-refill" in dc.labels(case([(250, 4, 1), (270, 4, 1)]), "lz4", (16, 0))  # token at 254, length bytes at 255 | 256
    assert dc._last_move(dc.CONFIGS["lz4"][(4, 0)], 100, 3, 4) == ("dwords", 1) and dc._last_move(cfg, 100, 300, 64) == ("small", 0) and dc._last_move(cfg, 100, 30, 64) == ("other", 0)


def test_gpu_batches_put_every_case_at_the_four_base_pairs(o):
    """the batch layout and the containers of tests/test_gpu_decoder_edges.py, built here without a GPU: the filler blocks leave every case at the (input base,
    output base) pair of its run (asserted while the batch is built), every filler decodes, and the oracle reads each container back to the builders' plaintext"""
    from tests import test_gpu_decoder_edges as ge
    for codec in CODECS:
        for shift in dc.SHIFTS:
            streams, caps, want, names = ge.batch(codec, (4, 0), shift)
            assert len(streams) == 2 * (2 * len(dc.cases(codec, (4, 0))) + len(dc.malformed(codec, (4, 0))))
            for f, cap, (_, _, plain) in list(zip(streams, caps, want))[0:64:2]:
                assert o.decompress(codec, f, cap) == plain
        assert sorted(n for n in ge.batch(codec, (4, 0), (0, 0))[3]) == sorted(n for n in ge.batch(codec, (4, 0), (8, 5))[3])
    for container in ge.CONTAINERS:
        groups, streams, plains = ge.container_inputs(container)
        assert len(groups) > 80 and all(len(p) <= 262144 for p in plains)
