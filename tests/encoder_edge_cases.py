"""Constructed inputs for the LZ4 and Snappy block ENCODERS: a catalog built at the edges of lz4_compress_mw.h / snappy_compress_mw.h (and of the
batch-probe and serial encoders behind them), the way tests/zstd_frame_cases.py is built at the decoders' edges.

lz4_cases() / snappy_cases() -> [(name, data, expect)].  `expect` says what the ORACLE's stream of `data` must look like (check()), so that a case
provably reaches the edge it is named for: tests/test_encoder_edge_cases.py holds every case to it, runs the catalog through a counting build of the
emulator (every path of the window encoders must be taken), tools/hostemu/check_enc.py --part edges through every variant on the emulator and
tests/test_gpu_encoder_edges.py through every variant on the GPU.  Pure Python + numpy, deterministic, no file read.

The inputs are made of three things: FILLER (bytes without a repeated 4-gram: no encoder finds a match in it), SECOND OCCURRENCES (a stretch of the
input once more at a chosen distance, a different byte guaranteed on either side) and plain runs / periods.  What the Java loops do with them:

LZ4 (Lz4RawCompressor.java): position 0 is inserted, the search probes 1, 2, ... 66 and then advances by 2 for 64 probes, by 3 for 64, ...; a probe at p
needs p + step <= n - 12; a hit is extended backwards down to the anchor / the candidate's position 0 (catch-up) and forwards up to n - 5; behind a match
ending at e, e - 2 is inserted and e probed at once (a hit there is a sequence without literals); the hash is over FIVE bytes, the comparison over four:
a match of exactly 4 bytes needs a fifth byte with the same hash (alike_byte).
Snappy (SnappyRawCompressor.java): per 64 KiB sub-block; position 0 is neither inserted nor probed (but an empty table slot IS position 0), the search
probes 1 .. 33, then every second position for 32 probes, every third, ...; a probe at p needs p + step <= n - 15; no catch-up: the literal before a
copy is as long as the probe schedule says; behind a copy ending at e, e - 1 is inserted and e looked up (a hit: a copy without literal); a copy runs up
to the end of the sub-block."""
import numpy as np

# ---------------------------------------------------------------- the parsers (a few dozen lines each) ----------------------------------------------------------------


def lz4_parse(c):
    """LZ4 block -> [(literal_length, offset, match_length)], the last entry (literal_length, 0, 0): the block's last literals"""
    c = bytes(c)
    i, out = 0, []
    while True:
        tok = c[i]
        i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = c[i]
                i += 1
                lit += b
                if b != 255:
                    break
        i += lit
        assert i <= len(c), "literals beyond the end of the block"
        if i == len(c):
            assert tok & 15 == 0, "the last token has a match length"
            out.append((lit, 0, 0))
            return out
        off = c[i] | (c[i + 1] << 8)
        i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = c[i]
                i += 1
                ml += b
                if b != 255:
                    break
        assert off != 0, "offset 0"
        out.append((lit, off, ml + 4))


def snappy_parse(c):
    """raw Snappy stream -> (uncompressed length, [("L", n) | ("C1", offset, n) | ("C2", offset, n) | ("C4", offset, n)])"""
    c = bytes(c)
    i = total = shift = 0
    while True:
        b = c[i]
        i += 1
        total |= (b & 0x7F) << shift
        shift += 7
        if b < 0x80:
            break
    out = []
    while i < len(c):
        tag = c[i]
        i += 1
        kind = tag & 3
        if kind == 0:
            n = tag >> 2
            if n >= 60:
                nb = n - 59
                n = int.from_bytes(c[i:i + nb], "little")
                i += nb
            out.append(("L", n + 1))
            i += n + 1
        elif kind == 1:
            out.append(("C1", ((tag >> 5) << 8) | c[i], ((tag >> 2) & 7) + 4))
            i += 1
        else:
            nb = 2 if kind == 2 else 4
            out.append(("C2" if kind == 2 else "C4", int.from_bytes(c[i:i + nb], "little"), (tag >> 2) + 1))
            i += nb
    assert i == len(c), "an element runs beyond the end of the stream"
    return total, out


def _fits(item, pattern):
    return len(item) == len(pattern) and all(p is None or p == v for v, p in zip(item, pattern))


def _has_run(items, run):
    return any(all(_fits(items[k + j], p) for j, p in enumerate(run)) for k in range(len(items) - len(run) + 1))


def check(codec, data, stream, expect):
    """-> the list of what `stream` (the oracle's compressed `data`) lacks of `expect`; [] is a case that reaches its edge.  Keys of `expect` (patterns are the
    parsers' tuples, None for "any"):  exact: the whole parse;  has: [run, ...], each run a list of patterns that must appear next to each other;
    none: [pattern, ...] that must not appear;  last: the last literal length (LZ4) / the last element (Snappy);  count / min_count: the number of matches /
    copy elements;  max_offset.  Whatever `expect` says, the parse must add up to len(data), a Snappy copy must stay inside its 64 KiB sub-block."""
    if codec == "lz4":
        return check_parse(codec, data, lz4_parse(stream), expect)
    total, items = snappy_parse(stream)
    return ["the stream says %d bytes, the input has %d" % (total, len(data))] * (total != len(data)) + check_parse(codec, data, items, expect)


def check_parse(codec, data, items, expect):
    """check() on a parse"""
    bad = []
    if codec == "lz4":
        body, last = items[:-1], items[-1][0]
        offsets = [s[1] for s in body]
        if sum(s[0] + s[2] for s in items) != len(data):
            bad.append("the parse adds up to %d of %d bytes" % (sum(s[0] + s[2] for s in items), len(data)))
        n_copies = len(body)
    else:
        offsets = [e[1] for e in items if e[0] != "L"]
        pos = 0
        for e in items:
            n = e[-1]
            if e[0] != "L" and (e[1] > pos % 65536 or e[1] == 0):
                bad.append("a copy at %d reaches %d back: across the start of its sub-block" % (pos, e[1]))
            if pos // 65536 != (pos + n - 1) // 65536:
                bad.append("an element at %d of %d bytes crosses a 64 KiB boundary" % (pos, n))
            pos += n
        if pos != len(data):
            bad.append("the elements add up to %d bytes, the input has %d" % (pos, len(data)))
        last = items[-1] if items else None
        n_copies = len(offsets)
    for key, want in expect.items():
        if key == "exact":
            if list(items) != list(want):
                bad.append("parse %r, expected %r" % (items[:12], list(want)[:12]))
        elif key == "has":
            bad += ["no %r in %r" % (run, items[:12]) for run in want if not _has_run(items, run)]
        elif key == "none":
            bad += ["%r in the parse" % (p,) for p in want if _has_run(items, [p])]
        elif key == "last":
            if last != want:
                bad.append("last %r, expected %r" % (last, want))
        elif key == "count":
            if n_copies != want:
                bad.append("%d matches, expected %d" % (n_copies, want))
        elif key == "min_count":
            if n_copies < want:
                bad.append("%d matches, expected at least %d" % (n_copies, want))
        elif key == "max_offset":
            if offsets and max(offsets) > want:
                bad.append("offset %d beyond %d" % (max(offsets), want))
        else:
            raise KeyError(key)
    return bad


# ---------------------------------------------------------------- the three helpers ----------------------------------------------------------------

_POOL_SIZE = 400000
_pool = None


def _filler_pool():
    """bytes 1..255 without a repeated 4-gram (checked with a set: np.unique over every 4-gram); fillers are slices of it"""
    global _pool
    if _pool is None:
        rng = np.random.default_rng(20260919)
        p = rng.integers(1, 256, _POOL_SIZE, dtype=np.uint8)
        while True:
            a = p.astype(np.uint32)
            grams = a[:-3] | (a[1:-2] << 8) | (a[2:-1] << 16) | (a[3:] << 24)
            order = np.argsort(grams, kind="stable")
            dup = order[1:][grams[order][1:] == grams[order][:-1]]  # every occurrence of a 4-gram but its first
            if dup.size == 0:
                break
            p[dup + 1] = rng.integers(1, 256, dup.size, dtype=np.uint8)
        assert len(set(grams.tolist())) == _POOL_SIZE - 3
        _pool = p.tobytes()
    return _pool


class _Retry(Exception):
    """this salt's bytes collide with what the case needs (a byte that must differ does not): the next salt"""


class _B:
    """a case under construction: filler, second occurrences, runs"""

    def __init__(self, salt=0):
        self.d = bytearray()
        self.cur = 31 + 1009 * salt
        self.ban = None  # the value the next byte must not have (the byte behind a second occurrence differs from the byte behind the first)

    def __len__(self):
        return len(self.d)

    def _push(self, bs):
        if len(bs):
            if self.ban is not None and bs[0] == self.ban:
                raise _Retry()
            self.ban = None
            self.d += bs
        return self

    def fill(self, n, before=None):
        """n bytes of filler; before = p: a second occurrence of position p follows, the filler's last byte differs from the byte before p"""
        pool = _filler_pool()
        not_last = self.d[before - 1] if before else None
        if n == 0:
            if not_last is not None and self.d and self.d[-1] == not_last:
                raise _Retry()
            return self
        while pool[self.cur] == self.ban or pool[self.cur + n - 1] == not_last:
            self.cur += 1
        assert self.cur + n <= _POOL_SIZE
        self.ban = None
        self.d += pool[self.cur:self.cur + n]
        self.cur += n
        return self

    def again(self, src, n):
        """the n bytes at src once more (they may overlap what is being written); whatever comes next differs from the byte behind the first occurrence"""
        if self.ban is not None and self.d[src] == self.ban:
            raise _Retry()
        for i in range(n):
            self.d.append(self.d[src + i])
        self.ban = self.d[src + n]
        return self

    def run(self, n, value=0):
        return self._push(bytes([value]) * n)

    def byte(self, value):
        return self._push(bytes([value]))

    def period(self, p, n):
        """n bytes of period p (p bytes of filler over and over)"""
        at = len(self.d)
        self.fill(min(p, n))
        if n > p:
            self.again(at, n - p)
        return self


def lz4_table_mask(n):
    size = 0 if n <= 1 else 1 << (n - 1).bit_length()
    return min(max(size, 16), 4096) - 1


def lz4_hash(five, mask):
    return ((int.from_bytes(bytes(five[:5]), "little") * 889523592379) >> 28) & mask


def alike_byte(four, other, mask):
    """a byte b != other with lz4_hash(four + b) == lz4_hash(four + other): what lets the LZ4 encoders find a match of exactly 4 bytes"""
    if mask is None:  # (a first pass that only measures the case)
        return other % 255 + 1
    want = lz4_hash(bytes(four) + bytes([other]), mask)
    for b in range(1, 256):
        if b != other and lz4_hash(bytes(four) + bytes([b]), mask) == want:
            return b
    raise _Retry()


def _again4(b, src, n, mask):
    """again(), and behind a 4-byte occurrence the byte that keeps the 5-byte hash"""
    b.again(src, n)
    if n == 4:
        b.byte(alike_byte(b.d[src:src + 4], b.d[src + 4], mask))


def lz4_model(d):
    """The parse of Lz4RawCompressor.java, restated in plain Python: what _build holds a short case to before it is handed out (a case whose table slot was
    taken by a filler position, or whose neighbouring bytes happen to agree, is rebuilt from other filler).  The oracle is the judge of the catalog
    (tests/test_encoder_edge_cases.py); this only keeps the catalog from depending on luck."""
    n = len(d)
    if n < 13:
        return [(n, 0, 0)]
    mask, table, out = lz4_table_mask(n), {}, []
    mfl, limit, anchor = n - 12, n - 5, 0
    table[lz4_hash(d[0:5], mask)] = 0
    pos = 1
    while True:
        nxt, attempts, step = pos, 64, 1
        while True:
            pos = nxt
            nxt += step
            step = attempts >> 6
            attempts += 1
            if nxt > mfl:
                return out + [(n - anchor, 0, 0)]
            h = lz4_hash(d[pos:pos + 5], mask)
            m = table.get(h, 0)
            table[h] = pos
            if d[m:m + 4] == d[pos:pos + 4] and m + 65535 >= pos:
                break
        while pos > anchor and m > 0 and d[pos - 1] == d[m - 1]:
            pos -= 1
            m -= 1
        lit = pos - anchor
        while True:
            k = 4
            while pos + k < limit and d[pos + k] == d[m + k]:
                k += 1
            out.append((lit, pos - m, k))
            pos += k
            anchor = pos
            if pos > mfl:
                return out + [(n - anchor, 0, 0)]
            table[lz4_hash(d[pos - 2:pos + 3], mask)] = pos - 2
            h = lz4_hash(d[pos:pos + 5], mask)
            m = table.get(h, 0)
            table[h] = pos
            if m + 65535 < pos or d[m:m + 4] != d[pos:pos + 4]:
                pos += 1
                break
            lit = 0


def snappy_model(d):
    """the same for SnappyRawCompressor.java"""
    out = []
    for at in range(0, len(d), 65536):
        b = d[at:at + 65536]
        n = len(b)
        size = min(max(1 << max(n - 1, 1).bit_length(), 256), 16384)
        shift = 32 - (size.bit_length() - 1)
        hash4 = lambda p: ((int.from_bytes(b[p:p + 4], "little") * 0x1e35a7bd) & 0xFFFFFFFF) >> shift
        table, fil, emit, pos, done = {}, n - 15, 0, 0, False
        while not done and pos <= fil:
            pos += 1
            skip = 32
            while pos + (skip >> 5) <= fil:
                h = hash4(pos)
                m = table.get(h, 0)
                table[h] = pos
                if b[m:m + 4] == b[pos:pos + 4]:
                    break
                pos += skip >> 5
                skip += 1
            else:
                break
            out += _lit(pos - emit)
            while True:
                k = 4
                while pos + k < n and b[pos + k] == b[m + k]:
                    k += 1
                out += _copy(pos - m, k)
                pos += k
                emit = pos
                if pos >= fil:
                    done = True
                    break
                table[hash4(pos - 1)] = pos - 1
                h = hash4(pos)
                m = table.get(h, 0)
                table[h] = pos
                if b[m:m + 4] != b[pos:pos + 4]:
                    break
        out += _lit(n - emit)
    return out


MODEL_LIMIT = 70000


def _build(codec, fn, *args):
    """fn(b, mask, *args) -> expect, over the salts until one fits; the LZ4 table mask depends on the length, which is known after a first pass"""
    why = None
    for salt in range(64):
        try:
            b = _B(salt)
            fn(b, None, *args)
            mask = lz4_table_mask(len(b))
            b = _B(salt)
            expect = fn(b, mask, *args)
            assert lz4_table_mask(len(b)) == mask
            data = bytes(b.d)
            if len(data) <= MODEL_LIMIT:
                why = check_parse(codec, data, lz4_model(data) if codec == "lz4" else snappy_model(data), expect)
                if why:
                    continue
            return data, expect
        except _Retry:
            continue
    raise AssertionError("no salt fits %s%r: %r" % (fn.__name__, args, why))


def _mixed(n, seed):
    """n bytes with matches of every kind, for the sizes where only the length matters"""
    rng = np.random.default_rng(seed)
    b = _B(seed % 50)
    while len(b) < n:
        b.ban = None
        b.fill(int(rng.integers(1, 24)))
        k = int(rng.integers(0, 4))
        if k == 0:
            b.run(int(rng.integers(4, 40)))
        elif len(b) > 40:
            src = int(rng.integers(max(0, len(b) - 70000), len(b) - 30))
            b.ban = None
            b.again(src, int(rng.integers(4, 30 if k < 3 else 300)))
    return bytes(b.d[:n])


def _lz4_slot_survives(d, pos, upto, mask):
    """whether the table still holds `pos` when the first search of the block probes `upto`: no probe between them has its hash"""
    probes = np.array([q for q in lz4_probe_positions(1, upto) if q > pos], dtype=np.int64)
    if probes.size == 0:
        return True
    a = np.frombuffer(bytes(d[:upto + 8]) + bytes(8), dtype=np.uint8).astype(np.uint64)
    five = sum(a[probes + k] << np.uint64(8 * k) for k in range(5))
    h = ((five * np.uint64(889523592379)) >> np.uint64(28)) & np.uint64(mask)
    return not (h == np.uint64(lz4_hash(d[pos:pos + 5], mask))).any()


def lz4_probe_positions(start, limit):
    """the positions the search that starts at `start` probes, below `limit`"""
    out, p, k = [], start, 0
    while p < limit:
        out.append(p)
        p += 1 if k == 0 else (63 + k) >> 6
        k += 1
    return out


def snappy_probe_offsets(limit):
    """the distances from a search's first probe to its probes, below `limit`"""
    out, p, t = [], 0, 0
    while p < limit:
        out.append(p)
        p += (32 + t) >> 5
        t += 1
    return out


# ---------------------------------------------------------------- LZ4 ----------------------------------------------------------------

def _lz4_two(b, mask, lead, length, gap, tail):
    """filler(lead) X filler(gap) X filler(tail), all of it inside the consecutive probes: one sequence"""
    b.fill(lead)
    x = len(b)
    b.fill(length)
    b.fill(gap, before=x)
    s = len(b)
    _again4(b, x, length, mask)
    b.fill(tail)
    n = len(b)
    tail = n - s - length
    if n < 13 or s > n - 13:
        return {"exact": [(n, 0, 0)]}
    m = min(length, n - 5 - s)
    return {"exact": [(s, s - x, m), (n - s - m, 0, 0)]}


def _lz4_far(b, mask, lead, length, s, tail):
    """the second occurrence at position s, wherever the skip schedule has got to by then: found some bytes into it and caught up"""
    b.fill(lead)
    x = len(b)
    b.fill(length)
    b.fill(s - len(b), before=x)
    _again4(b, x, length, mask)
    b.fill(tail)
    land = [q for q in lz4_probe_positions(1, s + length) if q >= s][0]
    assert length == 4 or land - s + 5 <= length, "the probe schedule steps over this occurrence"
    if mask is not None and not _lz4_slot_survives(b.d, x + land - s, land, mask):
        raise _Retry()
    return {"exact": [(s, s - x, length), (len(b) - s - length, 0, 0)]}


def _lz4_long_catchup(b, mask, back):
    """A catch-up of 63 .. 65 bytes needs a search that advances by more than that: 130 KiB of filler, and the first occurrence no more than 65 535 back, itself
    where the search already skips: X is placed so that its byte `back` is a probed position, and the probe that lands in the second X lands on that byte"""
    probes = lz4_probe_positions(1, 150000)
    land = [p for p, q in zip(probes[1:], probes[:-1]) if p - q >= 67][0]
    first = [p for p in probes if p >= land - 60000][0]
    x = first - back
    b.fill(x)
    b.fill(80)
    s = land - back
    b.fill(s - len(b), before=x)
    b.again(x, 80)
    b.fill(100)  # (a probe needs its successor, 67 on, inside the block)
    if mask is not None and not _lz4_slot_survives(b.d, first, land, mask):
        raise _Retry()
    return {"exact": [(s, s - x, 80), (100, 0, 0)]}


def _lz4_long_catchup_window(b, mask, back, gap):
    """A long catch-up behind a window: R where the search advances by 67 and more, its byte `back` the only probed position of it; 50 000 bytes on, a run of
    one byte that the batch-probe step finds (its second probe in the run meets its first), a window opens behind the run; `gap` literals; R again, probed
    position by position until byte `back` hits -- in the window (gap + back <= 61: the most a window's catch-up can be, its room is what lies between the anchor
    and its last lane) or in the batch-probe step the search goes on in -- then extended back to R's start"""
    probes = lz4_probe_positions(1, 260000)
    k = [i for i in range(1, len(probes)) if probes[i] - probes[i - 1] >= 67][0] + 2
    first = probes[k]
    x = first - back
    b.fill(x)
    b.fill(90)
    z0 = x + 50000
    b.fill(z0 - len(b))
    b.run(300)
    e = len(b)
    p0, p1 = [p for p in probes if p >= z0][:2]
    assert p1 + 5 <= e
    b.fill(gap, before=x)
    s = len(b)
    b.again(x, 90)
    b.fill(100)
    if mask is not None and not _lz4_slot_survives(b.d, first, p1, mask):
        raise _Retry()
    return {"exact": [(z0 + p1 - p0, p1 - p0, e - (z0 + p1 - p0)), (gap, s - x, 90), (100, 0, 0)]}


def _lz4_truncated(b, mask, length):
    """the equal bytes go on to the end of the block: the match stops at n - 5"""
    b.fill(4)
    x = len(b)
    b.fill(length)
    b.fill(3, before=x)
    s = len(b)
    b.again(x, length)
    return {"exact": [(s, s - x, length - 5), (5, 0, 0)]}


def _lz4_reprobe_at_limit(b, mask, tail):
    """X ... Y ... X Y: the second X ends `tail` + 7 bytes before the end, the second Y is probed right behind it -- if that is still at or below n - 12"""
    b.fill(4)
    y = len(b)
    b.fill(7)
    b.fill(3)
    x = len(b)
    b.fill(8)
    b.fill(3, before=x)
    s = len(b)
    b.again(x, 8)
    e = len(b)
    b.again(y, 7)
    b.fill(tail)
    n = len(b)
    if e > n - 12:
        return {"exact": [(s, s - x, 8), (n - e, 0, 0)]}
    m = min(7, n - 5 - e)
    return {"exact": [(s, s - x, 8), (0, e - y, m), (n - e - m, 0, 0)]}


def _lz4_period(b, mask, lead, p, length, tail):
    """a period of p bytes: one match of `length` bytes at offset p, measured from the registers and then from memory"""
    b.fill(lead)
    x = len(b)
    b.fill(p)
    s = len(b)
    _again4(b, x, length, mask)
    b.fill(tail)
    return {"exact": [(s, p, length), (len(b) - s - length, 0, 0)]}


def _lz4_window2(b, mask, wl, length, x_lead=2):
    """A match that ends beyond the first window opens a second one at a known place (base = e - 2: lane 2 is probed at once, the search starts at lane 3); the
    second occurrence of X starts at lane wl of it, its candidate the table's entry (X lies in the first window)"""
    b.fill(x_lead)
    x = len(b)
    b.fill(length)
    b.fill(2)
    z = len(b)
    b.fill(30)
    b.fill(2, before=z)
    s1 = len(b)
    assert s1 < 64
    b.again(z, 30)
    e = len(b)
    assert e >= 64
    b.fill(wl - 2, before=x)
    s2 = len(b)
    _again4(b, x, length, mask)
    b.fill(14)
    return {"exact": [(s1, s1 - z, 30), (wl - 2, s2 - x, length), (len(b) - s2 - length, 0, 0)]}


def _lz4_inwindow(b, mask, jl, offset, length, tail=14):
    """both occurrences in the first window: X at lane jl, again at lane jl + offset"""
    b.fill(jl)
    x = len(b)
    b.fill(length)
    b.fill(offset - length, before=x)
    s = len(b)
    _again4(b, x, length, mask)
    b.fill(tail)
    return {"exact": [(s, offset, length), (len(b) - s - length, 0, 0)]}


def _lz4_window_end(b, mask, end, follow):
    """a match that ends at lane `end` of the first window (62 .. 65: the last re-probe lanes, the first positions beyond); follow: a second Y right behind it"""
    b.fill(2)
    y = len(b)
    b.fill(8)
    b.fill(2)
    x = len(b)
    b.fill(8)
    b.fill(end - 8 - len(b), before=x)
    s = len(b)
    b.again(x, 8)
    if follow:
        b.again(y, 8)
        b.fill(14)
        return {"exact": [(s, s - x, 8), (0, end - y, 8), (14, 0, 0)]}
    b.fill(14)
    return {"exact": [(s, s - x, 8), (14, 0, 0)]}


def _lz4_behind_a_match(b, mask, gap):
    """Catch-up of one byte inside a window: the last byte of a match is never inserted (e - 2 and e are).  The bytes from e - 1
    occur again: the probe at their start misses, the next one meets e, and the match is extended back by one"""
    b.fill(4)
    z = len(b)
    b.fill(8)
    b.fill(3, before=z)
    s1 = len(b)
    b.again(z, 8)
    e = len(b)
    b.fill(9)
    b.fill(gap, before=e - 1)
    s2 = len(b)
    b.again(e - 1, 9)
    b.fill(13)
    return {"exact": [(s1, s1 - z, 8), (9 + gap, s2 - e + 1, 9), (13, 0, 0)]}


def _lz4_last_probe(b, mask, s, tail):
    """The second occurrence at a position the batch-probe step probes (s >= 64), the block ending so that this probe is the last one the schedule admits
    (s + step == n - 12), or the first it does not"""
    probes = lz4_probe_positions(1, s + 200)
    assert s in probes and s >= 64
    step = probes[probes.index(s) + 1] - s
    b.fill(4)
    x = len(b)
    b.fill(8)
    b.fill(s - len(b), before=x)
    b.again(x, 8)
    b.fill(tail)
    n = len(b)
    if s + step > n - 12:
        return {"exact": [(n, 0, 0)]}
    m = min(8, n - 5 - s)
    return {"exact": [(s, s - x, m), (n - s - m, 0, 0)]}


def _lz4_reprobe_behind(b, mask, s, tail, x_first):
    """Y and X early, X again at position s, Y again right behind it, the block ending `tail` bytes behind that: the second X ends at n - 12 (tail 5: the second Y
    is still probed), one before, one beyond (it is not).  s picks the way the second X is found and measured: a middle lane (vector), lane 60 (scalar: no
    facts), 70 (the batch-probe step); x_first: X at lane 1, a candidate inside the window below lane 4 (scalar)"""
    if x_first:
        b.fill(1)
        x = len(b)
        b.fill(8)
        b.fill(3)
        y = len(b)
        b.fill(7)
    else:
        b.fill(4)
        y = len(b)
        b.fill(7)
        b.fill(3)
        x = len(b)
        b.fill(8)
    b.fill(s - len(b), before=x)
    b.again(x, 8)
    e = len(b)
    b.again(y, 7)
    b.fill(tail)
    n = len(b)
    if e > n - 12:
        return {"exact": [(s, s - x, 8), (n - e, 0, 0)]}
    m = min(7, n - 5 - e)
    return {"exact": [(s, s - x, 8), (0, e - y, m), (n - e - m, 0, 0)]}


def _lz4_third(b, mask, s2, gap, lead=4):
    """X, X again where the batch-probe step finds it (its winning probe enters the table), X a third time: its candidate is the second X, not the first.
    lead >= 64: the first X is a probe of the same batch as the second -- two lanes of one hash, the table takes the winner's position"""
    b.fill(lead)
    x = len(b)
    b.fill(8)
    b.fill(s2 - len(b), before=x)
    b.again(x, 8)
    b.fill(gap, before=x)
    s3 = len(b)
    b.again(x, 8)
    b.fill(13)
    if mask is not None and not _lz4_slot_survives(b.d, x, s2, mask):  # (the probe AT s2 must be the one that hits: a later one, caught up, would leave s2 to a loser's insert)
        raise _Retry()
    return {"exact": [(s2, s2 - x, 8), (gap, s3 - s2, 8), (13, 0, 0)]}


def _lz4_literals(b, mask, n):
    b.fill(n)
    return {"exact": [(n, 0, 0)]}


def _lz4_then_literals(b, mask, n):
    """one match, then filler to the end: the search behind the match runs off the end in its window or in the batch-probe step"""
    b.fill(4)
    x = len(b)
    b.fill(8)
    b.fill(4, before=x)
    b.again(x, 8)
    b.fill(n)
    return {"exact": [(16, 12, 8), (n, 0, 0)]}


def _lz4_distance(b, mask, distance, gap):
    """X, a long run of one byte (one match: nothing of it enters the table, X's slot stays alive), X again `distance` behind the first -- probed at once behind
    the run's match, or three literals later in a search"""
    b.fill(4)
    x = len(b)
    b.fill(12)
    b.fill(3)
    r0 = len(b)
    b.run(x + distance - gap - r0)
    b.fill(gap, before=x)
    s = len(b)
    assert s - x == distance
    b.again(x, 12)
    b.fill(13)
    run = (r0 + 1, 1, s - gap - r0 - 1)
    if distance <= 65535:
        return {"exact": [run, (gap, distance, 12), (13, 0, 0)]}
    return {"exact": [run, (gap + 12 + 13, 0, 0)], "max_offset": 65535}


def _lz4_skipped_first(b, mask, skip_to, gap):
    """Catch-up inside a window.  Q early; filler until the search advances by 6 and more; R there: only some of its positions enter the table; Q again: a match
    that the batch-probe step finds, a window opens behind it; `gap` literals; R again: the window's consecutive probes miss until one meets a position of R
    that was inserted, and the match is extended back to R's start"""
    b.fill(4)
    q = len(b)
    b.fill(12)
    b.fill(skip_to - len(b))
    r = len(b)
    b.fill(24)
    b.fill(30, before=q)
    s1 = len(b)
    b.again(q, 12)
    b.fill(gap, before=r)
    s2 = len(b)
    b.again(r, 24)
    b.fill(13)
    return {"exact": [(s1, s1 - q, 12), (gap, s2 - r, 24), (13, 0, 0)]}


def _lz4_anchor_stops(b, mask, skip_to):
    """The same, the catch-up stopped by the anchor: R holds Q's last three bytes in front of its 14th byte, and Q R[13:] follows -- the bytes before R[13:] are
    equal on both sides, but they belong to the match before"""
    b.fill(4)
    q = len(b)
    b.fill(12)
    b.fill(skip_to - len(b))
    r = len(b)
    b.fill(10)
    b.ban = None
    b.again(q + 9, 3)
    b.ban = None
    b.fill(11)
    b.fill(30, before=q)
    s1 = len(b)
    b.again(q, 12)
    s2 = len(b)
    b.again(r + 13, 11)
    b.fill(13)
    return {"exact": [(s1, s1 - q, 12), (0, s2 - r - 13, 11), (13, 0, 0)]}


def _lz4_periods(b, mask, p):
    """stretches of period p with a filler byte between them: positions of the same hash in one window, some inserted and some inside matches"""
    for k in range(4):
        b.ban = None
        b.period(p, max(2 * p + 5, 24))
        b.ban = None
        b.fill(1 + k)
    b.fill(13)
    return {"min_count": 2 if p <= 40 else 1}


_lz4 = None


def lz4_cases():
    global _lz4
    if _lz4 is not None:
        return _lz4
    out = []

    def add(name, fn, *args):
        data, expect = _build("lz4", fn, *args)
        out.append(("lz4 " + name, data, expect))

    # ---- input length
    for n in (0, 1, 12, 13, 14, 16, 17):
        add("length %d, filler" % n, _lz4_literals, n)
    for n in (12, 13, 14, 16, 17, 20):
        out.append(("lz4 length %d, one byte" % n, bytes(n), {"exact": [(n, 0, 0)] if n < 14 else [(1, 1, n - 6), (5, 0, 0)]}))
    for n in (4096, 4097, 65535, 65536, 65537):
        out.append(("lz4 length %d, mixed" % n, _mixed(n, n), {"min_count": 20}))
    for n in (65535, 65536, 65537):
        out.append(("lz4 length %d, one byte: a match to the end of the run" % n, bytes(n), {"exact": [(1, 1, n - 6), (5, 0, 0)]}))
    # a match that ends on matchLimit = n - 5 / one short of it / is cut there; that starts at matchFindLimit - 1 = n - 13 (the last probe) / at n - 12 (never found)
    for tail in (5, 6, 7):
        add("match ends %d before the end" % tail, _lz4_two, 4, 10, 4, tail)
    for length in (13, 14, 17, 30):
        add("match of %d cut at the end" % length, _lz4_truncated, length)
    for length in (6, 7, 8, 9):
        add("match starts %d before the end" % (length + 5), _lz4_two, 4, length, 4, 5)
    for s in (64, 65, 66, 68, 70, 194, 197):  # (the last admitted probe of the batch-probe step advancing by 1, 2, 3, and the first not admitted)
        step = 1 if s < 66 else (2 if s < 194 else 3)
        for tail in (step + 3, step + 4, step + 5):
            add("second occurrence at %d, the block ends %d behind it" % (s, tail), _lz4_last_probe, s, tail)
    for s, x_first, how in ((25, False, "vector"), (25, True, "candidate at lane 1"), (60, False, "lane 60"), (62, True, "lane 62, candidate at lane 1"), (70, False, "batch-probe step"), (197, False, "batch-probe step at 197")):
        for tail in (4, 5, 6):
            add("a match (%s) that ends %d before the end, another right behind it" % (how, tail + 7), _lz4_reprobe_behind, s, tail, x_first)
    for s2, gap in ((70, 5), (70, 0), (190, 5), (64, 30)):
        add("third occurrence %d behind a second one at %d" % (gap, s2), _lz4_third, s2, gap)
    for lead, s2 in ((66, 90), (64, 188), (70, 80)):
        add("third occurrence behind two in one batch of probes, at %d and %d" % (lead, s2), _lz4_third, s2, 5, lead)
    for x, s in ((70, 90), (66, 190), (128, 188)):
        add("both occurrences in one batch of probes, at %d and %d" % (x, s), _lz4_far, x, 8, s, 13)
    for tail in (4, 5, 6):
        add("re-probe %d before the end" % (tail + 7), _lz4_reprobe_at_limit, tail)
    for tail in (5, 14, 15, 16, 269, 270, 271):
        add("last literals %d" % tail, _lz4_two, 4, 8, 4, tail)
    # ---- literal run before a match (0: the re-probe cases; 1: the runs)
    for lit in (13, 14, 15, 16, 17):
        add("literal run %d" % lit, _lz4_two, 4, 6, lit - 10, 13)
    for lit in (268, 269, 270, 271, 272, 524, 525, 526):
        add("literal run %d" % lit, _lz4_far, 4, 12, lit, 13)
    # ---- match length code: behind a search that has left the window (scalar emit), from a period (vector emit), from a run at lane 1 (no facts)
    for code in (0, 1, 14, 15, 16, 269, 270, 271, 524, 525, 526, 779, 780, 781, 1035):
        add("match length code %d, far" % code, _lz4_far, 4, code + 4, 2 * (code + 4) + 4 + 4 - (code + 4), 12)
        add("match length code %d, period 8" % code, _lz4_period, 4, 8, code + 4, 12)
        add("match length code %d, run" % code, _lz4_period, 0, 1, code + 4, 12)
    # ---- the forward count of the registers: total lengths 4 .. 17 at lane 2 (no literals), 3, a middle lane, the last lanes
    for length in range(4, 18):
        for wl in (2, 3, 30, 59, 60, 61, 62, 63):
            add("length %d at lane %d of the second window" % (length, wl), _lz4_window2, wl, length)
    for length in (4, 5, 8, 11, 12, 13, 17):
        for wl in (3, 60):
            add("length %d at lane %d of the second window, candidate below 4" % (length, wl), _lz4_window2, wl, length, 1)
    # ---- candidate inside the same window
    for p in (1, 2, 3, 4):
        for lead in (0, 1, 5):
            add("period %d from lane %d" % (p, lead), _lz4_period, lead, p, 40, 13)
    for offset in range(5, 60):
        add("in-window candidate at lane 4, offset %d" % offset, _lz4_inwindow, 4, offset, 5 if offset < 8 else 8)
    for jl in (0, 1, 2, 3):
        for wl in (60, 61, 62, 63):
            add("in-window candidate at lane %d, match at lane %d" % (jl, wl), _lz4_inwindow, jl, wl - jl, 9)
        add("in-window candidate at lane %d, match at lane 64" % jl, _lz4_inwindow, jl, 64 - jl, 9)
    for length in (4, 5, 11, 12, 13, 16, 17):
        add("in-window candidate, length %d" % length, _lz4_inwindow, 6, 20, length)
    add("in-window candidate, length 40", _lz4_period, 6, 20, 40, 13)
    for tail in (5, 6, 8, 9, 12):
        add("in-window candidate, the block ends %d behind the match" % tail, _lz4_inwindow, 5, 30, 8, tail)
    # ---- window geometry
    for end in (62, 63, 64, 65):
        add("match ends at lane %d" % end, _lz4_window_end, end, False)
        add("match ends at lane %d, another right behind it" % end, _lz4_window_end, end, True)
    for s in list(range(60, 71)) + list(range(124, 135)) + list(range(186, 194)):
        add("%d positions before the first match" % s, _lz4_far, 4, 10, s, 13)
    for s in (64, 188, 190):
        add("match at position %d: an end lane of a batch of probes" % s, _lz4_far, 0, 10, s, 13)
    for n in (61, 62, 63, 64, 65, 66, 77, 78, 79, 100, 141, 142, 143, 200, 300, 700):
        add("filler of %d: the search runs off the end" % n, _lz4_literals, n)
    for n in (5, 11, 12, 13, 14, 40, 46, 47, 48, 49, 50, 60, 75, 76, 77, 100, 250):
        add("a match, then filler of %d" % n, _lz4_then_literals, n)
    for gap in (1, 5, 20, 30):
        add("catch-up of one byte: the last byte of a match again, %d literals on" % gap, _lz4_behind_a_match, gap)
    # ---- backward catch-up: the skip schedule lands 0 .. step - 1 bytes into the second occurrence
    for s in list(range(100, 104)) + list(range(200, 206)) + list(range(1000, 1012)):
        add("catch-up, second occurrence at %d" % s, _lz4_far, 4, 16, s, 13)
    for s in list(range(1000, 1008)):
        add("catch-up stopped by the candidate, second occurrence at %d" % s, _lz4_far, 0, 16, s, 13)
    for back in (63, 64, 65):
        add("catch-up of %d bytes" % back, _lz4_long_catchup, back)
        add("catch-up of %d bytes where a search leaves its window" % back, _lz4_long_catchup_window, back, 2 if back < 65 else 3)  # (lane 2 + gap + back)
    for back, gap in ((58, 1), (59, 1), (60, 1), (59, 2)):
        add("catch-up of %d bytes in a window, %d literals" % (back, gap), _lz4_long_catchup_window, back, gap)
    for skip_to in range(1000, 1008):
        for gap in (0, 1, 3, 9):
            add("catch-up in a window, first occurrence at %d, %d literals" % (skip_to, gap), _lz4_skipped_first, skip_to, gap)
        add("catch-up stopped by the anchor, first occurrence at %d" % skip_to, _lz4_anchor_stops, skip_to)
    # ---- distance
    for distance in (65534, 65535, 65536, 65537):
        for gap, how in ((0, "right behind a match"), (3, "in a search"), (69, "behind 69 literals: in the batch-probe step"), (131, "behind 131 literals: in the batch-probe step")):
            add("distance %d, %s" % (distance, how), _lz4_distance, distance, gap)
    # ---- positions of the same hash inside one window
    for p in range(1, 71):
        add("periods of %d" % p, _lz4_periods, p)
    assert len(set(n for n, _, _ in out)) == len(out)
    out.sort(key=lambda c: c[0].endswith("mixed"))  # (the constructed cases first: the counting build names the first case that takes a path)
    _lz4 = out
    return out


# ---------------------------------------------------------------- Snappy ----------------------------------------------------------------

def _copy(offset, n):
    """what emitCopy writes for one match"""
    out = []
    while n >= 68:
        out.append(("C2", offset, 64))
        n -= 64
    if n > 64:
        out.append(("C2", offset, 60))
        n -= 60
    out.append(("C1", offset, n) if n < 12 and offset < 2048 else ("C2", offset, n))
    return out


def _lit(n):
    return [("L", n)] if n > 0 else []


def _sn_two(b, mask, lead, length, gap, tail):
    """filler(lead) X filler(gap) X filler(tail); lead >= 1 (position 0 never enters the table), the second X inside the first 33 probes"""
    b.fill(lead)
    x = len(b)
    b.fill(length)
    b.fill(gap)
    s = len(b)
    b.again(x, length)
    b.fill(tail)
    n = len(b)
    if n < 15 or s > n - 16:
        return {"exact": _lit(n)}
    return {"exact": _lit(s) + _copy(s - x, length) + _lit(tail)}


def _sn_literals(b, mask, n):
    b.fill(n)
    return {"exact": [("L", min(65536, n - k)) for k in range(0, n, 65536)]}


def _sn_to_the_end(b, mask, length):
    """the equal bytes go on to the end of the block: so does the copy"""
    b.fill(1)
    b.fill(length)
    b.fill(2)
    s = len(b)
    b.again(1, length)
    return {"exact": _lit(s) + _copy(s - 1, length)}


def _sn_period(b, mask, lead, p, length, tail):
    """a period of p bytes from position lead: found at lead + p (a probed position: below 34), one copy of `length` bytes"""
    b.fill(lead)
    x = len(b)
    b.fill(p)
    s = len(b)
    b.again(x, length)
    b.fill(tail)
    if tail == 0:
        b.ban = None
    return {"exact": _lit(s) + _copy(p, length) + _lit(tail)}


def _sn_run(b, mask, length, tail):
    """a run from position 0: the empty table slot is position 0, the probe at 1 finds it"""
    b.run(length + 1)
    b.fill(tail)
    return {"exact": [("L", 1)] + _copy(1, length) + _lit(tail)}


def _sn_far(b, mask, offset, length, x_at=1):
    """X, a long run (one copy in pieces of 64: nothing of it enters the table), X again `offset` behind the first, looked up right behind the run's copy"""
    b.fill(x_at)
    x = len(b)
    b.fill(length)
    b.fill(2)
    r0 = len(b)
    b.run(x + offset - r0)
    s = len(b)
    b.again(x, length)
    b.fill(16)
    grid = [1 + o for o in snappy_probe_offsets(r0 + 8) if 1 + o >= r0]  # the first probe in the run enters the table, the second finds it
    return {"exact": _lit(grid[1]) + _copy(grid[1] - grid[0], s - grid[1]) + _copy(offset, length) + _lit(16)}


def _sn_window2(b, mask, wl, length, tail=16):
    """A copy that ends beyond the first window opens a second one (base = e - 1: lane 1 is looked up at once, the search starts at lane 2); the second X starts
    at lane wl: 1, or a lane the search probes (2 .. 34, then the even ones)"""
    b.fill(1)
    x = len(b)
    b.fill(length)
    b.fill(2)
    z = len(b)
    b.fill(30)
    b.fill(2 + (length & 1))  # (the second Z at an odd position: beyond its 33rd probe the search takes every second one)
    s1 = len(b)
    b.again(z, 30)
    e = len(b)
    assert e >= 64
    b.fill(wl - 1)
    s2 = len(b)
    b.again(x, length)
    b.fill(tail)
    n = len(b)
    t = wl - 2 if wl - 2 <= 32 else 32 + (wl - 2 - 32) // 2  # the search's probe at lane wl, its advance
    if (wl == 1 and e >= n - 15) or (wl > 1 and s2 + ((32 + t) >> 5) > n - 15):
        return {"exact": _lit(s1) + _copy(s1 - z, 30) + _lit(n - e)}
    return {"exact": _lit(s1) + _copy(s1 - z, 30) + _lit(wl - 1) + _copy(s2 - x, length) + _lit(tail)}


def _sn_inwindow(b, mask, jl, wl, length, tail=16):
    """both occurrences in the first window: X at lane jl >= 1, again at lane wl (1 .. 33, or odd)"""
    b.fill(jl)
    b.fill(length)
    b.fill(wl - jl - length)
    b.again(jl, length)
    b.fill(tail)
    return {"exact": _lit(wl) + _copy(wl - jl, length) + _lit(tail)}


def _sn_inwindow2(b, mask, jl, wl, length):
    """both occurrences in the second window (lanes from e - 1)"""
    b.fill(1)
    z = len(b)
    b.fill(30)
    b.fill(2)
    s1 = len(b)
    b.again(z, 30)
    e = len(b)
    assert e < 64
    b.fill(39)
    s2 = len(b)
    b.again(z, 30)  # ends beyond the first window
    e = len(b)
    assert e >= 64
    base = e - 1
    b.fill(jl - 1)
    x = len(b)
    b.fill(length)
    b.fill(base + wl - len(b))
    s3 = len(b)
    b.again(x, length)
    b.fill(16)
    return {"exact": _lit(s1) + _copy(s1 - z, 30) + _lit(39) + _copy(s2 - s1, 30) + _lit(s3 - e) + _copy(s3 - x, length) + _lit(16)}


def _sn_insert_behind(b, mask, back):
    """the `input - 1` insert: the bytes from one before the end of a copy occur again -- found there (back = 1), or at the copy's end (back = 0)"""
    b.fill(1)
    b.fill(8)
    b.fill(3)
    b.again(1, 8)
    e = len(b)
    b.fill(10)
    b.ban = None
    s = len(b)
    b.again(e - back, 8)
    b.fill(16)
    return {"exact": [("L", 12)] + _copy(11, 8) + _lit(10) + _copy(s - e + back, 8) + _lit(16)}


def _sn_search_from(b, mask, c, t):
    """a copy that ends at lane c - 1 of the first window, no hit behind it: a search that starts at lane c, runs through the window into the batch-probe step
    and finds the second X with its probe t"""
    size = 6 if c - 7 <= 33 or (c - 7) % 2 else 5  # (the first X again at a position the first search probes)
    b.fill(1)
    x = len(b)
    b.fill(size)
    b.fill(c - 1 - size - len(b))
    s1 = len(b)
    b.again(x, size)
    e = len(b)
    assert e == c - 1
    lit = 1 + snappy_probe_offsets(100000)[t]
    b.fill(lit)
    b.ban = None
    s2 = len(b)
    b.again(x, size)
    b.fill(16)
    return {"exact": _lit(s1) + _copy(s1 - x, size) + _lit(lit) + _copy(s2 - s1, size) + _lit(16)}


def _sn_straddle(b, mask, before, length):
    """X early in the first sub-block, X again across the 64 KiB boundary: a copy up to the boundary, the rest is the second sub-block's literal"""
    b.fill(1)
    b.fill(length)
    b.fill(2)
    r0 = len(b)
    b.run(65536 - before - r0)
    s = len(b)
    b.again(1, length)
    b.fill(20)
    if before < 16:  # (the look-up behind the run's copy is not made within 15 bytes of the sub-block's end)
        return {"none": [("C1", s - 1, None), ("C2", s - 1, None)], "last": ("L", length - before + 20)}
    return {"has": [_copy(s - 1, before)], "last": ("L", length - before + 20)}


def _sn_probe_step(s):
    """the advance of the probe at position s of a block's first search"""
    offs = snappy_probe_offsets(s + 8)
    return (32 + offs.index(s - 1)) >> 5


def _sn_last_probe(b, mask, s, tail):
    """The second occurrence at a probed position s, the block ending so that this probe is the last one the schedule admits (s + step == n - 15), or the
    first it does not"""
    step = _sn_probe_step(s)
    b.fill(1)
    b.fill(8)
    b.fill(s - len(b))
    b.again(1, 8)
    b.fill(tail)
    n = len(b)
    if s + step > n - 15:
        return {"exact": _lit(n)}
    return {"exact": _lit(s) + _copy(s - 1, 8) + _lit(tail)}


def _sn_lookup_behind(b, mask, s, tail):
    """Y and X early, X again at the probed position s, Y again right behind it, the block ending `tail` bytes behind that: the second X ends one before
    n - 15 (tail 9: the second Y is looked up), at it, one beyond (it is not).  s picks the way the second X is found and measured: 25 (vector), 61 (scalar:
    the last lanes), 65 and 100 (the batch-probe step)"""
    _sn_probe_step(s)
    b.fill(1)
    y = len(b)
    b.fill(7)
    b.fill(3)
    x = len(b)
    b.fill(8)
    b.fill(s - len(b))
    b.again(x, 8)
    e = len(b)
    b.again(y, 7)
    b.fill(tail)
    n = len(b)
    if e >= n - 15:
        return {"exact": _lit(s) + _copy(s - x, 8) + _lit(n - e)}
    return {"exact": _lit(s) + _copy(s - x, 8) + _copy(e - y, 7) + _lit(tail)}


def _sn_third(b, mask, lead, s2, gap):
    """X, X again at a position the batch-probe step probes (its winning probe enters the table), X a third time: its candidate is the second X.  lead >= 65: the
    first X is a probe of the same batch as the second"""
    _sn_probe_step(lead), _sn_probe_step(s2)
    b.fill(lead)
    b.fill(8)
    b.fill(s2 - len(b))
    b.again(lead, 8)
    b.fill(gap)
    s3 = len(b)
    b.again(lead, 8)
    b.fill(16)
    return {"exact": _lit(s2) + _copy(s2 - lead, 8) + _lit(gap) + _copy(s3 - s2, 8) + _lit(16)}


def _sn_two_blocks(b, mask, second):
    """a full sub-block with matches and a second one of `second` bytes that repeats the first one's start: nothing may be found across the boundary"""
    b.d += _mixed(65536, 77)
    b.ban = None
    b.again(100, second)
    b.ban = None
    return {"min_count": 20} if second > 16 else {"min_count": 20, "last": ("L", second)}


def _sn_periods(b, mask, p):
    for k in range(4):
        b.ban = None
        b.period(p, max(2 * p + 5, 24))
        b.ban = None
        b.fill(1 + k)
    b.fill(16)
    return {"min_count": 2 if p <= 30 else 1}


_snappy = None


def snappy_cases():
    global _snappy
    if _snappy is not None:
        return _snappy
    out = []

    def add(name, fn, *args):
        data, expect = _build("snappy", fn, *args)
        out.append(("snappy " + name, data, expect))

    # ---- length
    for n in (0, 1, 14, 15, 16, 17, 127, 128):
        add("length %d, filler" % n, _sn_literals, n)
    for n in (14, 15, 16, 17, 18, 30):
        out.append(("snappy length %d, one byte" % n, bytes(n), {"exact": _lit(n) if n < 17 else [("L", 1)] + _copy(1, n - 1)}))
    for n in (127, 128, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16383, 16384, 16385, 65535, 65536, 65537, 65536 + 14, 65536 + 15, 65536 + 16, 131072, 131073):
        out.append(("snappy length %d, mixed" % n, _mixed(n, n + 1), {"min_count": 3 if n < 4096 else 20}))
    for second in (1, 14, 15, 16, 17, 40, 3000):
        add("a sub-block of 65536 and one of %d that repeats it" % second, _sn_two_blocks, second)
    for before in (4, 15, 16, 20):
        add("a repeat across the 64 KiB boundary, %d bytes before it" % before, _sn_straddle, before, 24)
    # ---- literal length: the last literal takes any value, the literal before a copy the values of the probe schedule
    for n in (1, 2, 59, 60, 61, 62, 255, 256, 257, 258):
        add("last literal %d" % n, _sn_two, 1, 16, 2, n)
    reach = set(1 + o for o in snappy_probe_offsets(700))
    for n in (59, 60, 61, 255, 256, 257):
        if n in reach:
            add("literal %d before a copy" % n, _sn_search_from, 30, snappy_probe_offsets(700).index(n - 1))
    for n in (65535, 65536, 65537, 131072):
        add("filler of %d: whole incompressible sub-blocks" % n, _sn_literals, n)
    # ---- copy length and offset
    for length in range(4, 13):
        add("copy of %d at offset 1" % length, _sn_run, length, 16)
        for offset in (2047, 2048, 2049):
            add("copy of %d at offset %d" % (length, offset), _sn_far, offset, length)
    for length in (63, 64, 65, 67, 68, 69, 71, 72, 127, 128, 129, 130, 131, 132, 133, 134, 135, 192, 193, 194, 195, 196, 199):
        add("copy of %d at offset 8" % length, _sn_period, 1, 8, length, 16)
        add("copy of %d at offset 1" % length, _sn_run, length, 16)
    for length in (64, 65, 67, 68, 71, 72, 128 + 3, 128 + 4, 128 + 11):
        add("copy of %d at offset 2047" % length, _sn_far, 2047, length)
        add("copy of %d at offset 2048" % length, _sn_far, 2048, length)
    for offset in (65000, 65500, 65520):
        add("copy at offset %d" % offset, _sn_far, offset, 16, 0)
    for length in (16, 17, 40, 70):
        add("copy of %d to the end of the block" % length, _sn_to_the_end, length)
    for tail in (0, 1, 14, 15, 16, 17):
        add("copy of 20 at offset 8, %d bytes before the end" % tail, _sn_period, 1, 8, 20, tail)
    for tail in (7, 8, 9):
        add("second occurrence %d before the end" % (tail + 8), _sn_two, 1, 8, 2, tail)
    for s in (33, 35, 63, 65, 67, 97, 100, 103):  # (the last admitted probe of the window and of the batch-probe step, advancing by 1, 2, 3, and the first not admitted)
        step = _sn_probe_step(s)
        for tail in (step + 6, step + 7, step + 8):
            add("second occurrence at %d, the block ends %d behind it" % (s, tail), _sn_last_probe, s, tail)
    for lead, s2, gap in ((1, 65, 5), (1, 65, 0), (1, 100, 20), (65, 85, 5), (67, 97, 0)):
        add("third occurrence %d behind a second one at %d, the first at %d" % (gap, s2, lead), _sn_third, lead, s2, gap)
    for s in (25, 59, 61, 63, 65, 100):
        for tail in (7, 8, 9):
            add("a copy at %d that ends %d before the end, another right behind it" % (s, tail + 7), _sn_lookup_behind, s, tail)
    # ---- the forward count of the registers: lengths 4 .. 17 at lane 1 (the look-up behind a copy), 2, 3, a middle lane, the last probed lanes
    for length in range(4, 18):
        for wl in (1, 2, 3, 20, 34, 36, 58, 60, 62):
            add("length %d at lane %d of the second window" % (length, wl), _sn_window2, wl, length)
        for wl in (59, 61, 63):
            add("length %d at lane %d of the first window" % (length, wl), _sn_inwindow, 2, wl, length)
    for tail in (0, 1, 3, 4, 7, 8, 11, 12, 15):
        add("length 8 at lane 60 of the second window, %d bytes before the end" % tail, _sn_window2, 60, 8, tail)
    # ---- candidate inside the same window
    for jl in (1, 2, 3, 10):
        for wl in (20, 33, 35, 59, 61, 63):
            add("in-window candidate at lane %d, copy at lane %d" % (jl, wl), _sn_inwindow, jl, wl, 8)
    for jl in (1, 2, 3, 10):
        for wl in (20, 34, 36, 60, 62):
            add("in-window candidate at lane %d, copy at lane %d, second window" % (jl, wl), _sn_inwindow2, jl, wl, 8)
    for p in (1, 2, 3, 4, 5, 7):
        for lead in (1, 2, 6):
            add("period %d from lane %d" % (p, lead), _sn_period, lead, p, 40, 16)
    for back in (0, 1):
        add("second occurrence of the bytes %d before a copy's end" % back, _sn_insert_behind, back)
    # ---- searches that start at lane c and run through the window; the batch-probe step finds the copy with probe t, or runs off the end
    for c in (29, 30, 31, 32, 33, 63):
        for t in (70, 130):
            add("search from lane %d, hit at probe %d" % (c, t), _sn_search_from, c, t)
    offs = snappy_probe_offsets(400)
    for t in (31, 32, 33, 34, 47, 48, 49, 63, 64, 65, 96, 97, 110, 111, 112):
        add("first copy at probe %d" % t, _sn_two, 1, 8, offs[t] - 8, 16)
    for n in (18, 30, 33, 34, 35, 36, 47, 48, 49, 50, 63, 64, 65, 66, 79, 80, 81, 100, 200, 300, 700):
        add("filler of %d: the search runs off the end" % n, _sn_literals, n)
    for n in (1, 14, 15, 16, 17, 30, 45, 46, 47, 48, 49, 50, 60, 64, 100, 250):
        add("a copy, then filler of %d" % n, _sn_two, 1, 8, 2, n)
    # ---- positions of the same hash inside one window
    for p in range(1, 71):
        add("periods of %d" % p, _sn_periods, p)
    assert len(set(n for n, _, _ in out)) == len(out)
    out.sort(key=lambda c: c[0].endswith("mixed"))  # (the constructed cases first: the counting build names the first case that takes a path)
    _snappy = out
    return out


def cases(codec):
    return lz4_cases() if codec == "lz4" else snappy_cases()


def emulator_cases(codec, limit=20000):
    """the entries an emulator run takes (a fiber switch per memory access): those of at most 20 000 bytes, and the longer ones that are cheap there -- a run of one
    byte is one match measured 64 bytes a step, 100 KiB of filler are a few thousand probes of the skip schedule.  What is left to the GPU is 64 KiB and more of
    mixed data (seconds each, per variant)."""
    return [c for c in cases(codec) if len(c[1]) <= limit or not (c[0].endswith("mixed") or "a sub-block of 65536" in c[0])]
