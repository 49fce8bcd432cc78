"""Cases for achip_compress_bound_batch / achip_pack_outputs, shared by the GPU test (tests/test_gpu_pack.py) and the emulator check (tools/hostemu/check_pack.py):
the lengths the bounds are asked for with their expected values restated in Python integers, the item sets the pack call is run over, and the numpy statement of
what it must produce (offsets, lengths, stored flags, totals, and the dense image byte for byte)."""
import numpy as np

INT32_MAX = 0x7FFFFFFF
INVALID_ARGUMENT = 3
PREFILL = 0xA5   # every destination byte before the call
GUARD = 64       # bytes behind the dense buffer that must keep the prefill
SRC_FILLER = 0xC3  # between the items of the source buffer (the raw buffer: 0x3C)
RAW_FILLER = 0x3C
ALIGNS = (1, 16, 4096)

COMPRESS_OPS = {"lz4": 1, "snappy": 3, "zstd": 5, "lz4frame": 7, "snappyframed": 9, "lz4hadoop": 11, "snappyhadoop": 13, "zstdstream": 14}
HADOOP_DEFAULT_BUFFER = 262144
HADOOP_OTHER_BUFFER = 4096
BOUND_LENGTHS = [0, 1, 5, 6, 254, 255, 256, 65535, 65536, 131071, 131072, 4194304, 4194305, 1 << 30, -1,
                 # near INT32_MAX: every op's 64-bit bound is past INT32_MAX for the last ones, some ops' only
                 2100000000, 2139095039, 2139095040, 2139127680, 2139127681, 2147483647 - 4 * 512 - 11, 2147483647 - 4 * 512 - 10, 2147418112, 2147483646, 2147483647,
                 -2147483648]


def exact_bound(name, n, buffer_size=HADOOP_DEFAULT_BUFFER):
    """The op's maxCompressedLength in Python integers (no width): what the device must give wherever this is <= INT32_MAX."""
    lz4 = lambda m: m + m // 255 + 16
    snappy = lambda m: 32 + m + m // 6
    zstd = lambda m: m + (m >> 8) + (((128 * 1024 - m) >> 11) if m < 128 * 1024 else 0)
    if name == "lz4":
        return lz4(n)
    if name == "snappy":
        return snappy(n)
    if name == "zstd":
        return zstd(n)
    if name == "zstdstream":
        return zstd(n) + 16
    if name == "lz4frame":
        return 7 + 4 + n + 4 * ((n + (4 << 20) - 1) // (4 << 20))
    if name == "snappyframed":
        return 10 + 8 * ((n + 65535) // 65536) + n
    is_snappy = name == "snappyhadoop"
    overhead = buffer_size // 6 + 32 if is_snappy else max(int(buffer_size * 0.01), 10)
    chunk = buffer_size - overhead
    one = snappy if is_snappy else lz4
    rest = n % chunk
    return (n // chunk) * (8 + one(chunk)) + (8 + one(rest) if rest > 0 else 0)


def host_bound(lib, name, n, buffer_size=HADOOP_DEFAULT_BUFFER):
    """The library's host function for the op."""
    if name in ("lz4hadoop", "snappyhadoop"):
        return lib.achip_hadoop_max_compressed_length(1 if name == "snappyhadoop" else 0, n, buffer_size)
    return getattr(lib, "achip_%s_max_compressed_length" % name)(n)


def check_bounds(lib, name, lengths, out_size, status, status_class, buffer_size=HADOOP_DEFAULT_BUFFER):
    """-> list of complaints (empty: all as the contract says)"""
    wrong = []
    for n, size, st in zip(lengths, out_size, status):
        n, size, st = int(n), int(size), int(st)
        exact = exact_bound(name, n, buffer_size) if n >= 0 else None
        if n < 0 or exact > INT32_MAX:
            if status_class(st) != INVALID_ARGUMENT or size != 0:
                wrong.append("%s(%d): want INVALID_ARGUMENT and size 0, got status %d size %d" % (name, n, st, size))
            continue
        # (exact <= INT32_MAX: the host function's own int arithmetic has stayed in range, and must agree)
        host = host_bound(lib, name, n, buffer_size)
        if st != 0 or size != exact or size != host:
            wrong.append("%s(%d): want %d (host function %d) and status 0, got status %d size %d" % (name, n, exact, host, st, size))
    return wrong


class Case:
    """A compress call's result as the pack call sees it: item i has out_len[i] bytes at src[src_off[i]:], or is left out (status[i] != 0 or out_len[i] < 0)."""

    def __init__(self, name):
        self.name = name
        self.lens, self.stat, self.want_src_mod = [], [], []
        self.raw = self.raw_off = self.raw_len = None

    def add(self, length, status=0, src_mod=None):
        self.lens.append(int(length))
        self.stat.append(int(status))
        self.want_src_mod.append(src_mod)

    def finish(self, rng):
        """Lays the items out in a source buffer: odd offsets, gaps of filler between the items, a left-out item's slot full of bytes nobody may copy."""
        self.n = len(self.lens)
        self.out_len = np.array(self.lens, dtype=np.int32)
        self.status = np.array(self.stat, dtype=np.int32)
        held = np.where(self.out_len > 0, self.out_len, 0).astype(np.int64)
        gap = rng.integers(1, 8, self.n).astype(np.int64) * 2 + 1  # odd gaps: the offsets run through every residue
        off = np.cumsum(held + gap) - held
        for i, m in enumerate(self.want_src_mod):  # (the items that want a residue: slide the rest of the layout)
            if m is not None:
                off[i:] += (m - off[i]) % 16
        self.src_off = off.astype(np.int64)
        self.src = np.full(int(off[-1] + held[-1]) + 37, SRC_FILLER, dtype=np.uint8)
        idx = _ranges(self.src_off, held)
        self.src[idx] = rng.integers(0, 256, len(idx), dtype=np.uint8)
        self.packed = (self.status == 0) & (self.out_len >= 0)
        return self

    def with_raw(self, rng):
        """The plaintexts beside it: about half the packed items have out_len >= raw_len, some with equality."""
        k = rng.integers(0, 4, self.n)
        base = np.where(self.out_len > 0, self.out_len, 0).astype(np.int64)
        self.raw_len = np.where(k == 0, base, np.where(k == 1, base // 2, np.where(k == 2, base + 1 + base // 3, base * 3 + 7))).astype(np.int32)
        gap = rng.integers(1, 8, self.n).astype(np.int64) * 2 + 1
        held = self.raw_len.astype(np.int64)
        self.raw_off = (np.cumsum(held + gap) - held).astype(np.int64)
        self.raw = np.full(int(self.raw_off[-1] + held[-1]) + 41, RAW_FILLER, dtype=np.uint8)
        idx = _ranges(self.raw_off, held)
        self.raw[idx] = rng.integers(0, 256, len(idx), dtype=np.uint8)
        return self

    def expect(self, align, use_raw=False):
        """-> packed_off, packed_len, stored, total_bytes, left_out, image (the dense stream's total_bytes bytes)"""
        ln = np.where(self.packed, self.out_len, 0).astype(np.int64)
        stored = np.zeros(self.n, dtype=np.int32)
        if use_raw:
            stored = (self.packed & (self.out_len >= self.raw_len)).astype(np.int32)
            ln = np.where(stored == 1, self.raw_len, ln).astype(np.int64)
        room = (ln + align - 1) // align * align
        off = np.cumsum(room) - room
        total = int(room.sum())
        image = np.zeros(total, dtype=np.uint8)
        for which, buf, boff in ((0, self.src, self.src_off), (1, self.raw, self.raw_off)):
            if which == 1 and not use_raw:
                continue
            pick = np.where(stored == which, ln, 0)
            image[_ranges(off, pick)] = buf[_ranges(boff, pick)]
        return off.astype(np.int64), ln.astype(np.int32), stored, total, int((~self.packed).sum()), image


def _ranges(starts, lens):
    """the indices starts[i] .. starts[i] + lens[i] of every i, concatenated"""
    lens = np.asarray(lens, dtype=np.int64)
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, dtype=np.int64)
    first = np.cumsum(lens) - lens
    return np.repeat(np.asarray(starts, dtype=np.int64) - first, lens) + np.arange(total, dtype=np.int64)


def _status_for(rng, count):
    """one ninth of the items carry a status"""
    return np.where(rng.integers(0, 9, count) == 0, -35, 0)


def case_a(rng):
    c = Case("a: one item")
    c.add(4321)
    return c.finish(rng)


def case_b(rng, tile, align, big=5 << 20, hi=70000, n=1000):
    """Lengths 0..hi with a ninth left out and one negative length; one item of `big` bytes (many tiles); with align 1 an item that ends exactly on a tile
    boundary and one that begins a byte before the next; and, again with align 1, every (source address mod 16, destination address mod 16) pair with
    lengths 0..48 (source and destination buffers 16-byte aligned)."""
    c = Case("b: %d items, mixed" % n)
    at = [0]  # the dense offset the next item gets

    def add(length, status=0, src_mod=None):
        c.add(length, status, src_mod)
        if status == 0 and length >= 0:
            at[0] += (length + align - 1) // align * align

    uniform = n - 512 - 4
    lens = rng.integers(0, hi + 1, uniform)
    stat = _status_for(rng, uniform)
    for i in range(uniform):
        if i == uniform // 3:
            add(big)
        if i == uniform // 2:
            add(tile - at[0] % tile)      # ends exactly on a tile boundary
            add(tile - 1)                 # (align 1: the next item begins one byte before a boundary)
            add(100)
        add(-1 if i == 7 else lens[i], stat[i])
    for k in range(256):  # a spacer puts the destination on residue k % 16, the layout the source on k // 16
        add((k % 16 - at[0]) % 16)
        add(int(rng.integers(0, 49)) if k % 5 else (0, 1, 15, 16, 17, 31, 32, 33, 47, 48)[k // 5 % 10], 0, k // 16)
    assert len(c.lens) == n
    c.finish(rng)
    if align == 1:  # the set is what it says
        off, ln, _, _, _, _ = c.expect(1)
        assert any(l > 0 and (o + l) % tile == 0 for o, l in zip(off, ln)) and any(l > 0 and o % tile == tile - 1 for o, l in zip(off, ln))
        pairs = {(int(s) % 16, int(o) % 16) for s, o, m in zip(c.src_off, off, c.want_src_mod) if m is not None}
        assert len(pairs) == 256
    return c


def case_c(rng, n=300001, run=20000, hi=200):
    """Many short items; a run of zero-length items, a run of left-out ones, the first and the last item left out."""
    c = Case("c: %d short items" % n)
    lens = rng.integers(0, hi + 1, n)
    stat = _status_for(rng, n)
    lens[n // 5:n // 5 + run] = 0
    stat[n // 5:n // 5 + run] = 0
    stat[n // 2:n // 2 + run] = -19
    stat[0] = stat[n - 1] = -35
    lens[n // 3] = -1
    for l, s in zip(lens, stat):
        c.add(l, s)
    return c.finish(rng)


def case_d(rng, n=1000):
    c = Case("d: every item left out")
    for i in range(n):
        c.add(int(rng.integers(0, 500)) if i % 2 else -1, -35 if i % 2 else 0)
    return c.finish(rng)


def pack_cases(tile, align, quick=False, seed=11):
    """(a) .. (d) for one alignment.  quick: the same shapes at a tenth of the size (for the emulator, which runs a lane at a time)."""
    rng = np.random.default_rng(seed + align)
    if quick:
        return [case_a(rng), case_b(rng, tile, align, big=9 * tile + 12345, hi=7000), case_c(rng, n=30001, run=2000), case_d(rng, n=300)]
    return [case_a(rng), case_b(rng, tile, align), case_c(rng), case_d(rng)]


def mismatches(case, align, use_raw, copied, buf, at, off, ln, stored, total):
    """What a pack call left (buf: the whole prefilled destination with its guard, the dense stream wanted at buf[at:]; off / ln / stored / total: its arrays)
    against case.expect: a list of words, empty if all is as the contract says."""
    want_off, want_len, want_stored, want_total, want_left, image = case.expect(align, use_raw)
    wrong = []
    if not (off == want_off).all():
        wrong.append("packedOff")
    if not (ln == want_len).all():
        wrong.append("packedLen")
    if use_raw and not (stored == want_stored).all():
        wrong.append("stored")
    if [int(t) for t in total] != [want_total, want_left, 1 if copied else 0]:
        wrong.append("total %s, want %s" % ([int(t) for t in total], [want_total, want_left, 1 if copied else 0]))
    expected = np.full(len(buf), PREFILL, dtype=np.uint8)
    if copied:
        expected[at:at + want_total] = image
    if not (buf == expected).all():
        wrong.append("bytes (first at dense offset %d of %d)" % (int(np.nonzero(buf != expected)[0][0]) - at, want_total))
    return wrong
