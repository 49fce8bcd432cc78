"""Windows over the chunked containers (achip_window_*): the case streams, a unit splitter that reads headers only, the model of a window call built from the
oracle's one-shot functions, and the checks over them -- shared by the emulator (tools/hostemu/check_window.py) and the GPU (tests/test_gpu_window.py).  Nothing here
calls the code under test: a check takes a `run(fmt, compress, buffer_size, windows, flags, caps) -> [result dict]` from its caller.

A result dict: consumed, out (the destination's first outLen bytes), stop, need, status, err.
"""
import struct

import numpy as np

from tests import oracle_lib

FORMATS = ("snappyframed", "lz4hadoop", "snappyhadoop")
DECOMPRESS_OP = {"snappyframed": 8, "lz4hadoop": 10, "snappyhadoop": 12}
COMPRESS_OP = {"snappyframed": 9, "lz4hadoop": 11, "snappyhadoop": 13}
FIRST, LAST = 1, 2
END, NEED_INPUT, NEED_ROOM, FAILED = 0, 1, 2, 3
MAGIC = b"\xff\x06\x00\x00sNaPpY"
FRAMED_BLOCK = 65536
BUFFER_SIZES = (64, 256)
# statuses that say "the destination is too small" in the one-shot readers: a window call says NEED_ROOM instead
D_SNF_OUTPUT_TOO_SMALL, D_HDP_NOT_CONSUMED = 96, 108
SNF_STREAM_DETAILS = range(88, 98)  # their offsets are positions in the stream (a block codec's are its own)


def codec_of(fmt):
    return "lz4" if fmt == "lz4hadoop" else "snappy"


def hadoop_block(codec, buffer_size):
    """Lz4HadoopOutputStream / SnappyHadoopOutputStream: plaintext bytes per block"""
    return buffer_size - (max(int(buffer_size * 0.01), 10) if codec == "lz4" else buffer_size // 6 + 32)


class Case:
    def __init__(self, fmt, name, stream, buffer_size=0, writer_shaped=False):
        self.fmt, self.name, self.stream, self.buffer_size, self.writer_shaped = fmt, name, bytes(stream), buffer_size, writer_shaped

    def __repr__(self):
        return "%s/%s%s" % (self.fmt, self.name, "@%d" % self.buffer_size if self.buffer_size else "")


class Model:
    """one-shot results and block lengths from the oracle, remembered"""

    def __init__(self, o):
        self.o = o
        self.shots = {}
        self.lengths = {}

    def one_shot(self, fmt, data, cap, buffer_size, magic=False):
        """-> (status, offset, plaintext); magic: an x-snappy-framed piece from inside a stream -- the reader gets the stream identifier in front of it and
        its stream offsets are counted from the piece"""
        key = (fmt, bytes(data), cap, buffer_size, magic)
        if key not in self.shots:
            try:
                if fmt == "snappyframed":
                    r = (0, 0, self.o.decompress("snappyframed", (MAGIC if magic else b"") + bytes(data), cap))
                else:
                    r = (0, 0, self.o.hadoop_decompress(codec_of(fmt), data, cap, buffer_size))
            except oracle_lib.OracleError as e:
                off = e.offset - 10 if magic and e.detail in SNF_STREAM_DETAILS else e.offset
                r = (e.status, off, b"")
            self.shots[key] = r
        return self.shots[key]

    def block_length(self, codec, chunk):
        """what a chunk decodes to, or None if the block decoder refuses it"""
        key = (codec, bytes(chunk))
        if key not in self.lengths:
            try:
                self.lengths[key] = len(self.o.decompress(codec, chunk, 1 << 16))
            except oracle_lib.OracleError:
                self.lengths[key] = None
        return self.lengths[key]


class Unit:
    def __init__(self, start, end, whole, declared=0, need=0):
        self.start, self.end, self.whole, self.declared, self.need = start, end, whole, declared, need


def be32(b, p):
    return struct.unpack(">i", b[p:p + 4])[0]


def snappy_preamble(data):
    """-> the announced length, or None"""
    v = 0
    for i in range(5):
        if i >= len(data):
            return None
        v |= (data[i] & 0x7F) << (7 * i)
        if not data[i] & 0x80:
            return v if v < 1 << 31 else None
    return None


def hadoop_units(model, codec, w):
    """The units of a Hadoop window, from its length words (and, per chunk, what it decodes to: the reader's next step depends on it).  The last unit may be not
    whole.  An end-of-stream marker (a length word of -1; for LZ4 any negative chunk length; for Snappy an empty chunk) leaves its unit not whole: the one-shot reader
    reads once more behind it, so what it says depends on everything up to the end of the stream."""
    units, p = [], 0
    while p < len(w):
        if len(w) - p < 4:
            units.append(Unit(p, len(w), False))
            break
        u = be32(w, p)
        if u == 0:
            units.append(Unit(p, p + 4, True))
            p += 4
            continue
        if u == -1:
            units.append(Unit(p, len(w), False))
            break
        q, left, unit = p + 4, u, None
        while unit is None:
            if len(w) - q < 4:
                unit = Unit(p, len(w), False, u)
                break
            clen = be32(w, q)
            q += 4
            if clen == -1 or (clen < 0 and codec == "lz4"):
                unit = Unit(p, len(w), False, u)
            elif clen < 0:
                unit = Unit(p, q, True, u)  # (the Snappy reader refuses it)
            elif clen > len(w) - q:
                unit = Unit(p, len(w), False, u, need=q + clen - p)
            else:
                produced = model.block_length(codec, w[q:q + clen])
                q += clen
                if codec == "snappy" and produced == 0:
                    unit = Unit(p, len(w), False, u)  # (an empty chunk ends the Snappy reader's stream)
                elif produced is None or (codec == "snappy" and (produced > left or snappy_preamble(w[q - clen:q]) != produced)):
                    unit = Unit(p, q, True, u)  # (the reader fails here)
                else:
                    left -= produced
                    if left == 0:
                        unit = Unit(p, q, True, u)
        units.append(unit)
        if not unit.whole:
            break
        p = unit.end
    return units


def framed_units(w, first):
    units, p = [], 0
    if first:
        if len(w) < 10:
            return [Unit(0, len(w), False, need=10)]
        units.append(Unit(0, 10, True))
        p = 10
    while p < len(w):
        if len(w) - p < 4:
            units.append(Unit(p, len(w), False))
            break
        flag, length = w[p], w[p + 1] | w[p + 2] << 8 | w[p + 3] << 16
        if length > len(w) - p - 4:
            units.append(Unit(p, len(w), False, need=4 + length))
            break
        declared = 0
        if flag == 0 and length >= 5:
            declared = snappy_preamble(w[p + 8:p + 4 + length]) or 0
        elif flag == 1 and length >= 5:
            declared = length - 4
        units.append(Unit(p, p + 4 + length, True, declared))
        p += 4 + length
    return units


def split(model, case_fmt, w, first):
    return framed_units(w, first) if case_fmt == "snappyframed" else hadoop_units(model, codec_of(case_fmt), w)


def is_room_status(status):
    return oracle_lib.status_detail(status) in (D_SNF_OUTPUT_TOO_SMALL, D_HDP_NOT_CONSUMED)


def expect(model, fmt, buffer_size, w, flags, cap):
    """what achip_window_decompress_batch owes for window `w`: the leading whole units that fit and that the one-shot reader accepts"""
    first, last = bool(flags & FIRST), bool(flags & LAST)
    out, consumed = b"", 0

    def result(stop, need=0, status=0, err=0):
        return {"consumed": consumed, "out": out, "stop": stop, "need": need, "status": status, "err": err if status else 0}

    for unit in split(model, fmt, w, first):
        room = cap - len(out)
        magic = fmt == "snappyframed" and not (first and unit.start == 0)
        if not unit.whole and last:  # the stream ends inside this unit: the one-shot reader's verdict on everything that is left
            status, off, piece = model.one_shot(fmt, w[unit.start:], room, buffer_size, magic)
            if status == 0:
                out, consumed = out + piece, len(w)
                return result(END)
            if is_room_status(status) and unit.declared > room:
                return result(NEED_ROOM, unit.declared)
            return result(FAILED, 0, status, unit.start + off)
        if not unit.whole:
            return result(NEED_INPUT, unit.need)
        if unit.declared > room:
            return result(NEED_ROOM, unit.declared)
        status, off, piece = model.one_shot(fmt, w[unit.start:unit.end], room, buffer_size, magic)
        if status != 0:
            return result(FAILED, 0, status, unit.start + off)
        out, consumed = out + piece, unit.end
    return result(END)


def mismatch(want, got):
    """-> the names of the fields that differ"""
    return [k for k in ("consumed", "stop", "need", "status", "err", "out") if want[k] != got[k]]


# ---- the case streams -------------------------------------------------------------------------------------------------------------------------------------------
def _text(n, seed=0):
    rng = np.random.default_rng(seed)
    words = [b"window", b"stream", b"block", b"chunk", b"hadoop", b"snappy", b"lz4", b"unit", b" ", b" ", b"the", b"a"]
    out = b""
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))]
    return out[:n]


def be(v):
    return struct.pack(">i", v)


def hadoop_blocks(o, codec, plain, block):
    """[(plaintext length, codec block)] of a writer-shaped stream"""
    return [(len(plain[i:i + block]), o.compress(codec, plain[i:i + block])) for i in range(0, len(plain), block)]


def hadoop_cases(o):
    cases = []
    for codec in ("lz4", "snappy"):
        fmt = codec + "hadoop"
        for buf in BUFFER_SIZES:
            block = hadoop_block(codec, buf)
            for units in (0, 1, 3, 12) if buf == 64 else (4,):
                plain = _text(block * units - (5 if units > 1 else 0), units + buf)
                cases.append(Case(fmt, "writer %d" % units, o.hadoop_compress(codec, plain, buf), buf, True))
                assert len(hadoop_blocks(o, codec, plain, block)) == units
        buf = 64
        block = hadoop_block(codec, buf)
        plain = _text(block * 4 - 3, 7)
        blocks = hadoop_blocks(o, codec, plain, block)
        whole = lambda bl: b"".join(be(n) + be(len(c)) + c for n, c in bl)
        cases.append(Case(fmt, "zero words", be(0) + whole(blocks[:1]) + be(0) + be(0) + whole(blocks[1:3]) + be(0), buf))
        # a block in two chunks: one length word in front of the chunks of two writer blocks
        two = be(blocks[1][0] + blocks[2][0]) + b"".join(be(len(c)) + c for _, c in blocks[1:3])
        cases.append(Case(fmt, "two chunks", whole(blocks[:1]) + two + whole(blocks[3:]), buf))
        if codec == "lz4":  # a chunk that produces less than its block declares: the reader asks for another chunk
            short = be(blocks[1][0] + 9) + be(len(blocks[1][1])) + blocks[1][1]
            cases.append(Case(fmt, "chunk short of its block", whole(blocks[:1]) + short + whole(blocks[2:]), buf))
        negative = be(blocks[1][0]) + be(-7)
        cases.append(Case(fmt, "negative chunk length", whole(blocks[:1]) + negative + whole(blocks[2:]), buf))
        cases.append(Case(fmt, "end marker", whole(blocks[:2]) + be(-1) + whole(blocks[2:]), buf))
        stream = whole(blocks)
        starts = [0]
        for n, c in blocks:
            starts.append(starts[-1] + 8 + len(c))
        for name, k in (("first", 0), ("middle", 2), ("last", len(blocks) - 1)):
            at = starts[k] + 8 + len(blocks[k][1]) // 2
            damaged = bytearray(stream)
            damaged[at] ^= 0xFF
            damaged[at + 1] ^= 0x5A
            cases.append(Case(fmt, "damaged %s unit" % name, damaged, buf))
    return cases


def framed_chunk(o, flag, body, plain=None):
    """a chunk: flag, 24-bit length, then (data chunks) the masked CRC-32C of the plaintext and the body"""
    payload = (struct.pack("<I", o.crc32c(plain, masked=True)) if plain is not None else b"") + body
    return bytes([flag]) + struct.pack("<I", len(payload))[:3] + payload


def framed_cases(o):
    parts = [_text(n, 40 + n) for n in (200, 1, 90, 333, 64)]
    noise = np.random.default_rng(9).integers(0, 256, 120, dtype=np.uint8).tobytes()
    compressed = [framed_chunk(o, 0, o.compress("snappy", p), p) for p in parts]
    raw = framed_chunk(o, 1, noise, noise)
    skippable = framed_chunk(o, 0x80, b"padding....")
    empty_skip = framed_chunk(o, 0xFE, b"")
    cases = [
        Case("snappyframed", "identifier only", MAGIC, writer_shaped=True),
        Case("snappyframed", "compressed", MAGIC + b"".join(compressed[:3]), writer_shaped=True),
        Case("snappyframed", "compressed and raw", MAGIC + compressed[0] + raw + compressed[1] + raw + b"".join(compressed[2:]), writer_shaped=True),
        Case("snappyframed", "skippable", MAGIC + skippable + compressed[0] + empty_skip + raw + skippable, writer_shaped=True),
        Case("snappyframed", "second identifier", MAGIC + compressed[0] + MAGIC + compressed[1] + raw, writer_shaped=True),
        Case("snappyframed", "twelve chunks", MAGIC + b"".join((compressed + [raw]) * 2), writer_shaped=True),
        Case("snappyframed", "unskippable", MAGIC + compressed[0] + framed_chunk(o, 0x02, b"what") + compressed[1]),
        Case("snappyframed", "shorter than 5", MAGIC + compressed[2] + bytes([0, 4, 0, 0]) + b"abcd" + compressed[1]),
        Case("snappyframed", "identifier of 5", MAGIC + compressed[2] + b"\xff\x05\x00\x00sNaPp" + compressed[1]),
        Case("snappyframed", "bad identifier", b"\xff\x06\x00\x00sNaPpX" + compressed[0]),
    ]
    wrong = bytearray(compressed[1])
    wrong[4] ^= 1
    cases.append(Case("snappyframed", "wrong crc", MAGIC + compressed[0] + bytes(wrong) + compressed[2]))
    wrong = bytearray(raw)
    wrong[30] ^= 1
    cases.append(Case("snappyframed", "wrong crc, raw", MAGIC + bytes(wrong) + compressed[2]))
    for name, k in (("first", 0), ("middle", 1), ("last", 2)):
        chunks = [compressed[0], compressed[3], compressed[2]]
        bad = bytearray(chunks[k])
        bad[8 + 2 + (len(bad) - 10) // 2] ^= 0xFF  # (behind header, CRC and preamble)
        chunks[k] = bytes(bad)
        cases.append(Case("snappyframed", "damaged %s chunk" % name, MAGIC + b"".join(chunks)))
    return cases


def all_cases(o):
    return hadoop_cases(o) + framed_cases(o)


# ---- check 1: every cut ----------------------------------------------------------------------------------------------------------------------------------------
def cuts(model, case, quick):
    """[(a, b, flags, cap)]: a at every unit boundary of the stream, b at every byte position behind it (quick: up to two units on, and the end), with and
    without LAST where b is the end, and three rooms: ample, exactly the first unit's plaintext, one byte less"""
    s = case.stream
    bounds = [u.start for u in split(model, case.fmt, s, True) if u.start == 0 or case.fmt != "snappyframed" or u.start >= 10]
    ample = len(model.one_shot(case.fmt, s, 1 << 16, case.buffer_size)[2]) + 4096
    out = []
    for i, a in enumerate(bounds):
        flag = FIRST if a == 0 else 0
        horizon = bounds[i + 2] if quick and i + 2 < len(bounds) else len(s)
        ends = list(range(a, horizon + 1)) + ([len(s)] if horizon < len(s) else [])
        here = split(model, case.fmt, s[a:], bool(flag))
        exact = next((u.declared for u in here if u.declared > 0), 0)
        for b in ends:
            for cap in sorted({ample, exact, max(exact - 1, 0)}):
                out.append((a, b, flag, cap))
                if b == len(s):
                    out.append((a, b, flag | LAST, cap))
    return out


def check_every_cut(run, o, cases, quick=False):
    """-> (windows checked, [description of a wrong one])"""
    model = Model(o)
    wrong, total = [], 0
    groups = {}
    for c in cases:
        groups.setdefault((c.fmt, c.buffer_size), []).append(c)
    for (fmt, buf), group in groups.items():
        items = [(c, a, b, flags, cap) for c in group for a, b, flags, cap in cuts(model, c, quick)]
        got = run(fmt, False, buf, [c.stream[a:b] for c, a, b, _, _ in items], [f for _, _, _, f, _ in items], [cap for _, _, _, _, cap in items])
        total += len(items)
        for (c, a, b, flags, cap), g in zip(items, got):
            want = expect(model, fmt, buf, c.stream[a:b], flags, cap)
            bad = mismatch(want, g)
            if bad:
                wrong.append("%r [%d:%d] flags %d cap %d: %s differ; want %s, got %s" % (c, a, b, flags, cap, bad, _brief(want), _brief(g)))
    return total, wrong


def _brief(r):
    return {k: (len(v) if k == "out" else v) for k, v in r.items()}


# ---- check 2: drive to the end ---------------------------------------------------------------------------------------------------------------------------------
def lockstep(run, fmt, compress, buffer_size, loops):
    """Runs generator loops side by side: each yields (window, flags, cap), is sent the result and returns its value at the end; one call of `run` per round over
    every loop still going.  -> the loops' values"""
    values = [None] * len(loops)
    asks = {}
    for i, g in enumerate(loops):
        try:
            asks[i] = next(g)
        except StopIteration as e:
            values[i] = e.value
    rounds = 0
    while asks:
        rounds += 1
        assert rounds < 4000, "no progress"
        order = sorted(asks)
        got = run(fmt, compress, buffer_size, [asks[i][0] for i in order], [asks[i][1] for i in order], [asks[i][2] for i in order])
        for i, r in zip(order, got):
            try:
                asks[i] = loops[i].send(r)
            except StopIteration as e:
                values[i] = e.value
                del asks[i]
    return values


def drive(stream, window_size, room):
    """The standard loop over one stream: call, advance by consumed, refill, grow to need.  -> (plaintext, status, where the last call began, its room)"""
    pos, held, cap, first = 0, window_size, room, True
    plain = b""
    while True:
        w = stream[pos:pos + held]
        last = pos + len(w) == len(stream)
        r = yield w, (FIRST if first else 0) | (LAST if last else 0), cap
        plain += r["out"]
        if r["stop"] == FAILED or (r["stop"] == END and last):
            return plain, r["status"], pos, cap
        pos += r["consumed"]
        first = first and r["consumed"] == 0
        if r["stop"] == END:
            held = window_size
        elif r["stop"] == NEED_INPUT:
            assert not last, "NEED_INPUT under LAST"
            held = max(held + window_size, r["need"]) if r["consumed"] == 0 else window_size
        else:
            assert r["stop"] == NEED_ROOM
            if r["out"] or r["consumed"]:
                cap = room
            else:
                assert r["need"] > cap, "NEED_ROOM without a need"
                cap = r["need"]


def check_drive(run, o, cases):
    """every case, window sizes of 1 unit, 3 units and 4096 bytes, rooms of 1 unit and 64 KiB: the delivered bytes are the one-shot plaintext -- or, for a damaged
    stream, the plaintext in front of the damage -- and the final status is the one-shot reader's: for the whole stream, or (what a reader says about a damaged chunk
    may depend on the room it is given) for what was left of the stream with the room that was left.  The streams of one format advance side by side."""
    model = Model(o)
    wrong, total = [], 0
    groups = {}
    for c in cases:
        groups.setdefault((c.fmt, c.buffer_size), []).append(c)
    for (fmt, buf), group in groups.items():
        loops, what = [], []
        for c in group:
            units = split(model, c.fmt, c.stream, True)
            spans = [u.end - u.start for u in units]
            one_unit = max([u.declared for u in units] + [1])
            for window_size in (max(spans[:1] + [1]), max(sum(spans[:3]), 1), 4096):
                for room in (one_unit, 65536):
                    loops.append(drive(c.stream, window_size, room))
                    what.append((c, window_size, room))
        for (c, window_size, room), (plain, status, pos, left) in zip(what, lockstep(run, fmt, False, buf, loops)):
            want = expect(model, fmt, buf, c.stream, FIRST | LAST, 1 << 17)
            total += 1
            there = model.one_shot(fmt, c.stream[pos:], left, buf, fmt == "snappyframed" and pos > 0)[0]
            if plain != want["out"] or status not in (want["status"], there):
                wrong.append("%r window %d room %d: %d bytes status %d, want %d bytes status %d" % (c, window_size, room, len(plain), status, len(want["out"]), want["status"]))
    return total, wrong


# ---- check 3: writers ------------------------------------------------------------------------------------------------------------------------------------------
def writer_plaintexts(fmt, buffer_size):
    block = FRAMED_BLOCK if fmt == "snappyframed" else hadoop_block(codec_of(fmt), buffer_size)
    sizes = (0, 1, block - 1, block, block + 1, (3 if fmt == "snappyframed" else 5) * block + (9 if fmt == "snappyframed" else 7))
    return block, [_text(n, 100 + i) for i, n in enumerate(sizes)]


def one_shot_compress(o, fmt, plain, buffer_size):
    return o.compress("snappyframed", plain) if fmt == "snappyframed" else o.hadoop_compress(codec_of(fmt), plain, buffer_size)


def worst_case(o, fmt, n, buffer_size):
    """the room a block of n plaintext bytes wants"""
    return 8 + n if fmt == "snappyframed" else o.hadoop_max_compressed_length(codec_of(fmt), n, buffer_size)


def write_stream(plain, cut, room, block):
    """A writer that is handed plain[:cut], then the rest, and holds what a call did not take; -> its output"""
    out, held, first = b"", b"", True
    for closing, piece in ((False, plain[:cut]), (True, plain[cut:])):
        held += piece
        while True:
            r = yield held, (FIRST if first else 0) | (LAST if closing else 0), room
            assert r["status"] == 0 and r["stop"] != FAILED, r
            out += r["out"]
            first = first and not r["out"]
            held = held[r["consumed"]:]
            if r["stop"] == END:
                break
            if r["stop"] == NEED_INPUT:
                assert not closing and len(held) < block and r["need"] == block, (closing, len(held), r["need"])
                break
            assert r["stop"] == NEED_ROOM and (r["out"] or r["consumed"]), "room for one block, and no block taken"
    assert not held
    return out


def same_blocks(o, fmt, buffer_size, got, want):
    """for an emulator that does not run the block encoders as the device does: the two streams are cut into the same blocks (what the window plan decides)"""
    model = Model(o)
    return [u.declared for u in split(model, fmt, got, True)] == [u.declared for u in split(model, fmt, want, True)]


def check_writers(run, o, quick=False, formats=FORMATS, same=None):
    """plaintexts of 0, 1, block - 1, block, block + 1 and several blocks and a bit; each handed over in two pieces cut at 40 fixed positions, with ample room and
    with room for exactly one block: the outputs, one behind the other, are the one-shot writer's stream.  The writers of one format advance side by side."""
    wrong, total = [], 0
    for fmt in formats:
        for buf in (BUFFER_SIZES if fmt != "snappyframed" else (0,)):
            block, plains = writer_plaintexts(fmt, buf)
            loops, what = [], []
            for plain in plains:
                positions = sorted({int(p) for p in np.linspace(0, len(plain), 38)} | {min(block, len(plain)), max(len(plain) - 1, 0)})[:40]
                if quick:
                    positions = positions[::8]
                for room in (worst_case(o, fmt, len(plain), buf) * 2 + 64, worst_case(o, fmt, block, buf) + (10 if fmt == "snappyframed" else 0)):
                    for cut in positions:
                        loops.append(write_stream(plain, cut, room, block))
                        what.append((plain, cut, room))
            for (plain, cut, room), got in zip(what, lockstep(run, fmt, True, buf or 262144, loops)):
                total += 1
                want = one_shot_compress(o, fmt, plain, buf)
                if got != want and not (same is not None and same(o, fmt, buf, got, want)):
                    wrong.append("%s buffer %d, %d bytes cut at %d, room %d: %d bytes differ from the one-shot writer's" % (fmt, buf, len(plain), cut, room, len(got)))
    return total, wrong
