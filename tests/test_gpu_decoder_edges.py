"""The catalog of constructed decoder streams (tests/decoder_edge_cases.py: one named edge of one ring instantiation per stream, each proven against the oracle
and labelled by tests/test_decoder_edge_cases.py, each run under the emulator with guard bands by tools/hostemu/check_v3.py --part edges) through every
decoder on the GPU: every ring configuration on the cases built for its own ring sizes, the two-pass decoders and auto mode on the 4-lane cases, and the ring
bodies inside the four containers.  Sources and outputs are packed back to back; a small block in front of every case puts it at each of the four
(input base, output base) pairs in turn.  Nothing here can fault a kernel that the emulator run passes: the malformed streams are refused by bounds checks."""
import struct

import numpy as np
import pytest

from tests import decoder_edge_cases as dc
from tests import oracle_lib
from tests.oracle_lib import OracleError
from tests.test_gpu_lz4_snappy import CODECS, DECODERS, configure

pytestmark = pytest.mark.gpu

_expected = {}


def own_batch(options=None):
    from tests.gpu_harness import GpuBatch
    return GpuBatch(0, options or {})


def restore(g, codec):
    """the test's own context back at its defaults (the lanes per block of LZ4 excepted: its default, "by the batch size", is no value the option takes --
    as in tests/test_gpu_lz4_snappy.py it goes back to 16; the context is this test's alone)"""
    configure(g, codec, DECODERS[0])
    if codec == "snappy":
        g.set_option(CODECS[codec]["group_opt"], 0)
    g.set_option(CODECS[codec]["variant_opt"], 5)
    g.set_option("%s.decompress.parse" % codec, 0)
    g.set_option("decompress.latency_max_blocks", 256)
    g.set_option("lz4.decompress.auto_min_blocks", 4096)


def filler(codec, src_residue, dst_residue):
    """a literal-only block whose stream length and capacity are src_residue and dst_residue mod 16: (stream, capacity, plaintext)"""
    for n in range(1, 40):
        plain, stream = dc.build(codec, [], n, strict=False)
        if len(stream) % 16 == src_residue:
            return stream, n + (dst_residue - n) % 16, plain
    raise AssertionError((codec, src_residue))


def batch(codec, config, shift):
    """The catalog of a configuration as one batch for GpuBatch.run(unaligned=True): the cases in a fixed shuffled order (the lane groups of a wavefront hold
    different cases), every valid one at its exact capacity and at capacity + 9, every malformed one at its own capacity; in front of each a filler block that
    leaves it at (input base, output base) == shift.  Returns (streams, capacities, expectations, names), an expectation being (status, offset, plaintext)."""
    o = oracle_lib.load()
    key = (codec, config)
    if key not in _expected:
        valid, damaged = dc.cases(codec, config), dc.malformed(codec, config)
        items = [(c.name, c.kind, c.stream, len(c.plain) + pad, (0, 0, c.plain)) for c in valid for pad in (0, 9)]
        for name, _, stream, cap in damaged:
            with pytest.raises(OracleError) as e:
                o.decompress(codec, stream, cap)
            items.append((name, "malformed", stream, cap, (e.value.status, e.value.offset, None)))
        order = np.random.default_rng(7).permutation(len(items))
        _expected[key] = [items[i] for i in order]
    streams, caps, want, names = [], [], [], []
    src = dst = 0
    for name, kind, stream, cap, expect in _expected[key]:
        f, fcap, fplain = filler(codec, (shift[0] - src) % 16, (shift[1] - dst) % 16)
        streams += [f, stream]
        caps += [fcap, cap]
        want += [(0, 0, fplain), expect]
        names += ["filler", "%s (%s)" % (name, kind)]
        src += len(f)
        dst += fcap
        # what GpuBatch.run(unaligned=True) makes of it: offsets are running sums of the stream lengths and of the capacities, from 16-byte aligned buffers
        assert (src % 16, dst % 16) == tuple(shift), (name, src, dst)
        src += len(stream)
        dst += cap
    return streams, caps, want, names


def check(g, op, codec, config, shift, what):
    streams, caps, want, names = batch(codec, config, shift)
    src_off = g.pack(streams, align=1)[1]
    assert all(int(src_off[i]) % 16 == shift[0] for i in range(1, len(streams), 2))
    outs, status, err = g.run(op, streams, caps, unaligned=True)
    wrong = []
    for i, (est, eoff, plain) in enumerate(want):
        ok = status[i] == est and (err[i] == eoff if est != 0 else (len(outs[i]) == len(plain) and outs[i] == plain))
        if not ok:
            wrong.append("%s: status %d offset %d length %d, expected status %d offset %d length %s" % (names[i], status[i], err[i], len(outs[i]), est, eoff, len(plain) if plain is not None else None))
    assert not wrong, "%s %s, bases %r: %d of %d blocks differ: %s" % (codec, what, shift, len(wrong), len(want), wrong[:8])


@pytest.mark.parametrize("codec", ["lz4", "snappy"])
@pytest.mark.parametrize("cfg", DECODERS, ids=lambda c: "variant%d-lanes%d-ring%d" % c)
def test_ring_decoder_on_its_own_edges(codec, cfg):
    """one ring configuration (lanes per block, ring class; (1, 4, 3): the latency class) on the catalog built from its CHUNK, LDS_REACH and ring sizes, at the
    four (input base, output base) pairs: status 0, the exact length and the builder's plaintext for every valid case at both capacities, the oracle's status
    and offset for every malformed one, nothing written outside a block's capacity"""
    g = own_batch()
    try:
        configure(g, codec, cfg)
        for shift in dc.SHIFTS:
            check(g, CODECS[codec]["d"], codec, (cfg[1], cfg[2]), shift, "rings %r" % (cfg,))
    finally:
        restore(g, codec)


@pytest.mark.parametrize("codec", ["lz4", "snappy"])
@pytest.mark.parametrize("parse", [1, 2], ids=["lane-per-block-parse", "wavefront-per-block-parse"])
def test_two_pass_decoders_on_the_4_lane_catalog(codec, parse):
    """variant 7 with either parser: the two passes decode the catalog themselves.  A record holds offsets up to 65 535: a Snappy copy from farther back -- the
    catalog has one such case, at two capacities -- makes the parser hand its block to the ring decoder by design (snappy_decompress_v5.hip), and those blocks
    are the only ones counted in decompress.twopass_fallback_blocks"""
    handed_over = 2 * sum(any(s[2] > 0xFFFF for s in c.seqs) for c in dc.cases(codec, (4, 0)))
    assert handed_over == (2 if codec == "snappy" else 0)
    g = own_batch()
    try:
        configure(g, codec, (7, 4, 0))
        g.set_option("%s.decompress.parse" % codec, parse)
        for shift in dc.SHIFTS:
            check(g, CODECS[codec]["d"], codec, (4, 0), shift, "two passes, parser %d" % parse)
            assert g.codec.native.get_stat("decompress.twopass_fallback_blocks") == handed_over
    finally:
        restore(g, codec)


@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_auto_mode_on_the_4_lane_catalog(codec):
    """the default variant with its probes switched on for a batch of this size (decode_probes.hip reads these streams' heads): whichever decoder the device
    picks returns the bytes"""
    g = own_batch()
    try:
        g.set_option(CODECS[codec]["variant_opt"], 5)
        g.set_option("lz4.decompress.auto_min_blocks", 16)  # (one threshold for both codecs)
        for shift in dc.SHIFTS:
            check(g, CODECS[codec]["d"], codec, (4, 0), shift, "auto mode")
    finally:
        restore(g, codec)


# ---- the ring bodies inside the containers: the 64-lane configurations' targeted valid cases, several blocks to a frame / stream, so that a block starts
# wherever the one before it ended: the readers set the rings up anew for each block, on whatever output base the last one left, next to bytes already written ----

FRAMED_HEADER = bytes([0xff, 0x06, 0x00, 0x00, 0x73, 0x4e, 0x61, 0x50, 0x70, 0x59])
PER_CONTAINER = 5


def container_groups(codec, limit):
    out = []
    for config in ((64, 0), (64, 1)):
        cases = [c for c in dc.cases(codec, config) if c.kind == "targeted" and 0 < len(c.plain) <= limit]
        out += [cases[i:i + PER_CONTAINER] for i in range(0, len(cases), PER_CONTAINER)]
    return out


def lz4_frame(o, cases):
    """a frame of independent 64 KiB blocks, no content size, no checksums but the header's"""
    desc = bytes([(1 << 6) | (1 << 5), 4 << 4])
    out = struct.pack("<I", 0x184D2204) + desc + bytes([(o.xxh32(desc) >> 8) & 0xFF])
    for c in cases:
        out += struct.pack("<I", len(c.stream)) + c.stream
    return out + struct.pack("<I", 0)


def hadoop_stream(o, cases):
    return b"".join(struct.pack(">i", len(c.plain)) + struct.pack(">i", len(c.stream)) + c.stream for c in cases)


def framed_stream(o, cases):
    return FRAMED_HEADER + b"".join(bytes([0]) + struct.pack("<I", len(c.stream) + 4)[:3] + struct.pack("<I", o.crc32c(c.plain, masked=True)) + c.stream for c in cases)


CONTAINERS = {
    "lz4-frame": ("lz4", 6, lz4_frame, "lz4frame.decompress.variant", 2, lambda o, s, cap: o.decompress("lz4frame", s, cap)),
    "hadoop-lz4": ("lz4", 10, hadoop_stream, "hadoop.decompress.variant", 3, lambda o, s, cap: o.hadoop_decompress("lz4", s, cap, 262144)),
    "hadoop-snappy": ("snappy", 12, hadoop_stream, "hadoop.decompress.variant", 3, lambda o, s, cap: o.hadoop_decompress("snappy", s, cap, 262144)),
    "x-snappy-framed": ("snappy", 8, framed_stream, "snappyframed.decompress.variant", 3, lambda o, s, cap: o.decompress("snappyframed", s, cap)),
}


def container_inputs(container):
    """(groups of cases, the container around each group, its plaintext): the oracle's decode of the container is the builders' plaintext"""
    o = oracle_lib.load()
    codec, op, wrap, option, default, decode = CONTAINERS[container]
    groups = container_groups(codec, 65536)  # (64 KiB: the LZ4 frame's block size and the framed format's chunk size, below the Hadoop buffer size)
    streams = [wrap(o, group) for group in groups]
    plains = [b"".join(c.plain for c in group) for group in groups]
    for s, p in zip(streams, plains):
        assert decode(o, s, len(p)) == p
    return groups, streams, plains


@pytest.mark.parametrize("variant", ["default", "wavefront-per-frame"])
@pytest.mark.parametrize("container", list(CONTAINERS))
def test_ring_bodies_inside_the_containers(container, variant):
    codec, op, wrap, option, default, decode = CONTAINERS[container]
    groups, streams, plains = container_inputs(container)
    g = own_batch()
    try:
        g.set_option(option, default if variant == "default" else 0)
        g.set_option("hadoop.buffer_size", 262144)
        for pad, unaligned in ((0, True), (9, True), (0, False)):
            outs, status, err = g.run(op, streams, [len(p) + pad for p in plains], unaligned=unaligned)
            wrong = ["%s .. %s: status %d offset %d" % (group[0].name, group[-1].name, s, e) for group, out, p, s, e in zip(groups, outs, plains, status, err) if s != 0 or out != p]
            assert not wrong, "%s, %s reader, capacity + %d: %d of %d differ: %s" % (container, variant, pad, len(wrong), len(groups), wrong[:8])
    finally:
        g.set_option(option, default)
