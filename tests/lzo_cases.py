"""A labelled catalog of LZO1X streams and plaintexts at the edges of the grammar (M/lzo/LzoRawDecompressor.java, M/lzo/LzoRawCompressor.java), for the
model's own tests, the CPU emulator's check and the GPU tests.

Decode side: streams assembled command by command (Assembler: lit(n), m(length, offset, trailing), end()) -- valid ones and malformed ones.  A case is
(label, stream, capacity): capacity None = "whatever the stream decodes to" (the tests run such a case with exact and with generous room); the expected
outcome of every case comes FROM THE MODEL (expected()).
Encode side: plaintexts built so that the Java encoder takes a given emit path; what the encoder is expected to emit is a predicate over the commands of
the model's output (tests/test_lzo_ref.py asserts it: a plaintext that stopped provoking its path would fail there, not pass silently)."""
import random

from tests import lzo_ref

GENEROUS = 96  # bytes of room beyond the plaintext in the "generous" runs


def _bytes(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


class Assembler:
    """LZO1X commands, one call each; the literal bytes are pseudo-random (seeded per stream)"""

    def __init__(self, seed=1):
        self.out = bytearray()
        self.rng = random.Random(seed)

    def _literals(self, n):
        self.out += _bytes(self.rng, n)

    def first(self, n):
        """the first-command form: one byte 17 + n, then n literals (0 <= n <= 238)"""
        assert 0 <= n <= 238
        self.out.append(17 + n)
        self._literals(n)
        return self

    def lit(self, n):
        """0b0000_LLLL: a run of n >= 4 literals (only behind a command without trailing literals, or as a block's first command)"""
        assert n >= 4
        v = n - 3
        if v <= 15:
            self.out.append(v)
        else:
            self.out.append(0)
            v -= 15
            while v > 255:
                self.out.append(0)
                v -= 255
            self.out.append(v)
        self._literals(n)
        return self

    def _extended(self, command, bits, v):
        limit = (1 << bits) - 1
        if v <= limit:
            self.out.append(command | v)
        else:
            self.out.append(command)
            v -= limit
            while v > 255:
                self.out.append(0)
                v -= 255
            self.out.append(v)

    def m(self, length, offset, trailing=0, kind=None):
        """a match of `length` bytes at `offset`, then `trailing` (0..3) literals.  kind: 'm2' 0b0000_DDLL behind 1..3 literals (2 bytes, offset 1..1024),
        'm3' the same byte behind 4 or more literals (3 bytes, offset 2049..3072), 's' 0bMMMD_DDLL (3..8 bytes, offset 1..2048), 'near' 0b001M_MMMM (offset
        1..16384), 'far' 0b0001_HMMM (offset 16385..49151); None: by offset and length as the Java encoder chooses"""
        assert 0 <= trailing <= 3
        if kind is None:
            kind = "s" if (3 <= length <= 8 and offset <= 2048) else ("near" if offset <= 16384 else "far")
        if kind == "m2":
            assert length == 2 and 1 <= offset <= 1024
            d = offset - 1
            self.out += bytes([((d & 3) << 2) | trailing, d >> 2])
        elif kind == "m3":
            assert length == 3 and 2049 <= offset <= 3072
            d = offset - 2049
            self.out += bytes([((d & 3) << 2) | trailing, d >> 2])
        elif kind == "s":
            assert 3 <= length <= 8 and 1 <= offset <= 2048
            d = offset - 1
            self.out += bytes([((length - 1) << 5) | ((d & 7) << 2) | trailing, d >> 3])
        elif kind == "near":
            assert length >= 3 and 1 <= offset <= 16384
            self._extended(0x20, 5, length - 2)
            t = ((offset - 1) << 2) | trailing
            self.out += bytes([t & 0xFF, t >> 8])
        else:
            assert kind == "far" and length >= 3 and 16385 <= offset <= 49151
            d = offset - 16384
            self._extended(0x10 | ((d >> 14) << 3), 3, length - 2)
            t = ((d & 0x3FFF) << 2) | trailing
            self.out += bytes([t & 0xFF, t >> 8])
        self._literals(trailing)
        return self

    def end(self, low_bits=0):
        """the end marker: 0b0001_0001 and a trailer whose offset field is zero (its two low bits are not looked at)"""
        self.out += bytes([0x11, low_bits & 3, 0])
        return self

    def raw(self, data):
        self.out += bytes(data)
        return self

    def bytes(self):
        return bytes(self.out)


def expected(stream, capacity):
    """the model's verdict: ('ok', plaintext) or ('malformed', offset)"""
    try:
        return ("ok", lzo_ref.decompress(stream, capacity))
    except lzo_ref.Malformed as e:
        return ("malformed", e.offset)


def _valid_cases():
    cases = []

    def add(label, asm):
        cases.append((label, asm.bytes(), None))

    # every command class at both ends of its offset range, with 0..3 literals behind it
    for t in range(4):
        add("m2 offsets 1 and 1024, trailing %d" % t, Assembler(10 + t).lit(1100).m(3, 7, 1).m(2, 1, 2, "m2").m(2, 1024, t, "m2").end())
        add("m3 offsets 2049 and 3072, trailing %d" % t, Assembler(20 + t).lit(3100).m(3, 2049, 0, "m3").lit(9).m(3, 3072, t, "m3").end())
        add("short offsets 1 and 2048, lengths 3 and 8, trailing %d" % t, Assembler(30 + t).lit(2100).m(3, 1, 0, "s").m(8, 2048, t, "s").m(8, 1, t, "s").m(3, 2048, 0, "s").end())
        add("near offsets 1 and 16384, trailing %d" % t, Assembler(40 + t).lit(16500).m(5, 1, t, "near").m(40, 16384, t, "near").end())
        add("far offsets 16385 32767 32768 49151, trailing %d" % t,
            Assembler(50 + t).lit(49200).m(5, 16385, t, "far").m(6, 32767, t, "far").m(7, 32768, t, "far").m(40, 49151, t, "far").end())
    # every length-extension edge
    for n in (4, 18, 19, 273, 274, 528):
        add("literal run %d" % n, Assembler(60 + n).lit(n).m(4, 2, 0).lit(n).end())
    add("trailing literal run 3", Assembler(70).lit(8).m(4, 2, 3).m(2, 5, 3, "m2").end())
    for n in (33, 34, 288, 289):
        add("near match length %d" % n, Assembler(80 + n).lit(40).m(n, 37, 1, "near").m(n, 1, 0, "near").end())
    for n in (9, 10, 264, 265):
        add("far match length %d" % n, Assembler(90 + n).lit(17000).m(n, 16385, 2, "far").m(n, 16500, 0, "far").end())
    # the three meanings of a 0b0000_xxxx byte: behind no literals a run, behind 1..3 a 2-byte match, behind 4 or more a 3-byte match
    add("0b0000_xxxx by the previous literal count", Assembler(100).lit(2060).m(3, 2050, 0, "m3").lit(4).m(3, 2049, 2, "m3").m(2, 3, 0, "m2").lit(5).end())
    # first commands
    for c in (17, 18, 20, 21, 255):
        a = Assembler(110 + c).first(c - 17)
        if c == 17:
            a.lit(6)
        elif c - 17 <= 3:
            a.m(2, 1, 0, "m2")
        else:
            a.m(3, 2, 1, "s")
        add("first command %d" % c, a.end())
    # overlapping matches
    for off in range(1, 16):
        a = Assembler(130 + off).lit(20)
        for length in (15, 16, 17, 32, 33):
            a.m(length, off, length & 3, "near")
        add("overlapping matches at offset %d" % off, a.end())
    # the executor's window
    a = Assembler(150).lit(4200)
    for off in (4095, 4096, 4097):
        a.m(20, off, 1, "near").m(70, off, 0, "near")
    add("offsets 4095 4096 4097", a.end())
    add("offset 49151, long match", Assembler(151).lit(49151).m(600, 49151, 0, "far").end())
    # concatenated blocks
    two = Assembler(160).lit(30).m(9, 11, 2).end().first(5).m(4, 20, 0).end(3)
    add("two blocks in one item", two)
    add("three blocks in one item", Assembler(161).raw(two.bytes()).lit(300).m(50, 300, 1).end())
    # more than 504 records (the arena's chunk link): 700 short commands
    a = Assembler(170).lit(12)
    for k in range(700):
        a.m(3 + k % 6, 1 + k % 11, 1 + k % 3)
    add("700 commands", a.end())
    return cases


def long_run_case():
    """one item whose match-length extension runs past 16383 bytes (the record's skip field): ~4 MiB at offset 1"""
    return ("4 MiB run at offset 1", Assembler(180).lit(4).m(4200000, 1, 0, "near").lit(7).end().bytes(), None)


def _malformed_cases():
    cases = []
    # each command class cut at every byte
    whole = {
        "literal run": (Assembler(200), lambda a: a.lit(600)),
        "first command": (Assembler(201), lambda a: a.first(9)),
        "m2": (Assembler(202).lit(8).m(3, 2, 1), lambda a: a.m(2, 3, 2, "m2")),
        "m3": (Assembler(203).lit(2100), lambda a: a.m(3, 2049, 1, "m3")),
        "short": (Assembler(204).lit(8), lambda a: a.m(5, 3, 3, "s")),
        "near": (Assembler(205).lit(8), lambda a: a.m(700, 3, 2, "near")),
        "far": (Assembler(206).lit(17000), lambda a: a.m(700, 16400, 1, "far")),
        "end marker": (Assembler(207).lit(8), lambda a: a.end()),
    }
    for name, (asm, add) in whole.items():
        head = len(asm.out)
        add(asm)
        full = asm.bytes()
        start = 1 if name in ("literal run", "first command") else head  # (cut at 0, these two are the empty item: valid)
        for cut in range(start, len(full)):
            if name in ("literal run", "first command") and 8 < cut < len(full) - 2:
                continue  # (the middle of the literals: the same check as their ends)
            cases.append(("%s cut at byte %d" % (name, cut - head), full[:cut], 1 << 20))
    # a match reaching before the start of the output
    cases.append(("match before the start of the output", Assembler(210).lit(10).m(4, 11, 0).end().bytes(), 1 << 20))
    cases.append(("m2 before the start of the output", Assembler(211).first(1).m(2, 2, 0, "m2").end().bytes(), 1 << 20))
    # capacity one byte short
    s = Assembler(212).lit(10).m(30, 4, 0).end().bytes()
    cases.append(("capacity one short for a match", s, 39))
    s = Assembler(213).lit(10).m(30, 4, 0).lit(12).end().bytes()
    cases.append(("capacity one short for a literal run", s, 51))
    s = Assembler(214).lit(10).m(30, 4, 3).end().bytes()
    cases.append(("capacity one short for trailing literals", s, 42))
    cases.append(("capacity zero", Assembler(215).lit(10).end().bytes(), 0))
    # literals reaching past the input
    cases.append(("literals past the input", Assembler(216).lit(10).bytes()[:-1] + b"", 1 << 20))
    cases.append(("trailing literals past the input", Assembler(217).lit(10).m(5, 2, 3).bytes()[:-1], 1 << 20))
    # no end marker, bytes behind the last end marker
    cases.append(("no end marker", Assembler(218).lit(10).m(5, 2, 0).bytes(), 1 << 20))
    good = Assembler(219).lit(10).m(5, 2, 0).end().bytes()
    for tail in (b"\x00", b"\x11", b"\x11\x00", b"\x05abc", b"\x40"):
        cases.append(("bytes behind the last end marker %s" % tail.hex(), good + tail, 1 << 20))
    # first commands 16 and 17 followed by nothing
    cases.append(("first command 16", b"\x10", 1 << 20))
    cases.append(("first command 16 and more", b"\x10\x00\x00\x11\x00\x00", 1 << 20))
    cases.append(("first command 17", b"\x11", 1 << 20))
    # a length extension that ends with the input
    cases.append(("extension to the end of the input", Assembler(220).lit(8).bytes() + b"\x20\x00\x00\x00", 1 << 20))
    return cases


_DECODE = None


def decode_cases():
    """[(label, stream, capacity or None)] -- valid and malformed, without the ~4 MiB long-run item (long_run_case())"""
    global _DECODE
    if _DECODE is None:
        _DECODE = [("empty item", b"", None)] + _valid_cases() + _malformed_cases()
    return _DECODE


def runs(case):
    """the (capacity, expected) pairs a case is run with: exact and generous room where the case names none"""
    label, stream, capacity = case
    if capacity is not None:
        return [(capacity, expected(stream, capacity))]
    n = lzo_ref.decoded_size(stream)
    return [(n, expected(stream, n)), (n + GENEROUS, expected(stream, n + GENEROUS))]


# ---- encode side ----
def _planted(seed, distance, length, gap=0):
    """incompressible bytes with ONE repetition planted: `length` bytes that stood `distance` bytes earlier -- and a 40-byte repetition that ends 12 + gap bytes in
    front of it, so that the search has just restarted and probes every position there.  Both sources lie in the block's first 64 bytes, whose positions all
    enter the hash table; whether their entries survive until the search reaches the copies depends on the bytes in between (the table has 4 096 entries):
    planted() looks for a seed with which they do."""
    rng = random.Random(seed)
    base = bytearray(_bytes(rng, distance + 48))
    base[-(52 + gap):-(12 + gap)] = base[4:44]
    return bytes(base) + bytes(base[48:48 + length]) + _bytes(rng, 24)


def planted(predicate, distance, length, gap=0):
    for seed in range(400):
        data = _planted(seed * 7919 + distance + length, distance, length, gap)
        if predicate(lzo_ref.commands(lzo_ref.compress(data))):
            return data
    raise AssertionError("no seed plants a match of %d at %d" % (length, distance))


def _has(match_length=None, offset=None, literals=None):
    def check(cmds):
        for c in cmds:
            if c is None:
                continue
            if (match_length is None or c[0] == match_length) and (offset is None or c[1] == offset) and (literals is None or c[2] == literals):
                return True
        return False
    return check


def _none_at(offset):
    return lambda cmds: all(c is None or c[1] != offset for c in cmds)


_ENCODE = None


def encode_cases():
    """[(label, plaintext, predicate over lzo_ref.commands(compress(plaintext)) or None)]"""
    global _ENCODE
    if _ENCODE is not None:
        return _ENCODE
    rng = random.Random(4242)
    cases = []
    for n in list(range(0, 14)) + [237, 238, 239, 240]:
        cases.append(("incompressible, %d bytes (one literal run)" % n, _bytes(rng, n), None))
    for n in (237, 238, 239):  # the first literal in front of a match: the one-byte form ends at 237
        head = _bytes(rng, n)
        cases.append(("first literal of %d before a match" % n, head + head[:40] + _bytes(rng, 16), _has(offset=n, literals=None)))
    # 0..3 literals before a match: the count goes into the previous command's trailer
    unit = _bytes(rng, 24)
    for k in range(4):
        data = _bytes(rng, 30) + unit + _bytes(rng, 9) + unit + _bytes(rng, k) + unit[:20] + _bytes(rng, 20)
        cases.append(("%d literals between two matches" % k, data, _has(literals=k) if k else None))
    cases.append(("matches back to back", (unit + b"Q") * 3 + unit * 4 + _bytes(rng, 20), None))
    # the short command's edges
    for distance in (2048, 2049):
        for length in (8, 9):
            cases.append(("match of %d at offset %d" % (length, distance), planted(_has(length, distance), distance, length), _has(length, distance)))
    # the offset classes
    for distance in (16384, 16385, 32767, 32768, 49151):
        cases.append(("offset %d" % distance, planted(_has(offset=distance), distance, 300), _has(offset=distance)))
    cases.append(("a candidate at 49152 is refused", _planted(5, 49152, 300), _none_at(49152)))
    # match lengths at the 510 / 255 extension edges: 0b001M_MMMM (31 in the command) and 0b0001_HMMM (7)
    for length in (33, 34, 288, 289, 543, 544, 798, 799):
        distance = max(300, length + 64)
        cases.append(("near match of %d" % length, planted(_has(length, distance), distance, length), _has(length, distance)))
    for length in (9, 10, 264, 265, 519, 520, 774, 775):
        cases.append(("far match of %d" % length, planted(_has(length, 20000), 20000, length), _has(length, 20000)))
    cases.append(("a run of one byte", b"\x07" * 5000 + _bytes(rng, 13), _has(offset=1)))
    # incompressible data through the skip schedule; table sizes 16 (up to 16 bytes) and 4096 (from 2049 bytes)
    cases.append(("incompressible 9000 bytes", _bytes(rng, 9000), None))
    for n in (13, 16, 17, 2048, 2049):
        cases.append(("two-letter text of %d bytes" % n, bytes(rng.choice(b"ab") for _ in range(n)), None))
    words = [_bytes(rng, rng.randrange(2, 9)) for _ in range(60)]
    cases.append(("text-like 30000 bytes", b" ".join(rng.choice(words) for _ in range(6000))[:30000], None))
    _ENCODE = cases
    return cases


def vector_inputs():
    """[(label, plaintext)]: the encode catalog, and small text-like plaintexts whose liblzo2 streams stay below the recording tool's hex limit
    (tools/record_lzo_vectors.py -> tests/golden/lzo_vectors.json)"""
    rng = random.Random(777)
    words = [_bytes(rng, rng.randrange(1, 7)) for _ in range(30)]
    text = b" ".join(rng.choice(words) for _ in range(5000))
    extra = [("text-like %d bytes" % n, text[k:k + n]) for k, n in ((0, 500), (100, 3000))]
    extra += [("three-letter text %d bytes" % n, bytes(rng.choice(b"xyz") for _ in range(n))) for n in (64, 1000)]
    extra.append(("3-byte repeats at 2049..3072", far_triples()))
    return [(label, data) for label, data, _ in encode_cases()] + extra


def far_triples():
    """3 000 incompressible bytes with twenty 3-byte repeats planted 2049 .. 3072 bytes behind their source, 15 fresh bytes between them: what liblzo2's level
    999 encodes with the 3-byte command at 2049 .. 3072 behind four or more literals -- a command the Java encoder never emits"""
    rng = random.Random(0)
    base = bytearray(_bytes(rng, 3000))
    for k in range(20):
        p = 2600 + k * 18
        src = p - rng.randrange(2049, min(p, 3072))
        base[p:p + 3] = base[src:src + 3]
    return bytes(base)
