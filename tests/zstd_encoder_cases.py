"""Constructed inputs for the Zstd encoder (zstd_compress_body.h, zstd_dfast_mw.h, zstd_compress.hip): cases() names an edge of the frame, block, literals,
sequences or match-finder code per input and says what the oracle's frame of it must look like; describe() reads a frame back from RFC 8878 alone
(headers, FSE table descriptions, the backward bit stream of the sequences -- no Huffman decoding: literals are skipped by their size); check() holds a
frame to a case's expectation and to the plaintext.  tests/test_zstd_encoder_cases.py proves every case by the oracle without a GPU and runs
emulator_cases() through a counting build of the kernel source; tests/test_gpu_zstd_encoder_edges.py runs the catalog on the GPU.
Imports numpy, the standard library and the two sibling catalogs."""
import numpy as np

from tests import encoder_edge_cases as ec
from tests import zstd_frame_cases as zc

BLOCK = zc.MAX_BLOCK  # 131072
MODES = ("predefined", "rle", "fse", "repeat")
# RFC 8878 3.1.1.3.2.2: the predefined distributions
LL_DEFAULT = ([4, 3] + [2] * 11 + [1, 1, 1] + [2] * 9 + [3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6)
ML_DEFAULT = ([1, 4, 3] + [2] * 6 + [1] * 37 + [-1] * 7, 6)
OF_DEFAULT = ([1] * 6 + [2, 2, 2] + [1] * 15 + [-1] * 5, 5)
assert len(LL_DEFAULT[0]) == 36 and len(ML_DEFAULT[0]) == 53 and len(OF_DEFAULT[0]) == 29
assert all(sum(abs(v) for v in d) == 1 << log for d, log in (LL_DEFAULT, ML_DEFAULT, OF_DEFAULT))


class Malformed(Exception):
    """describe() refuses the frame"""


def _need(cond, what):
    if not cond:
        raise Malformed(what)


# ---------------------------------------------------------------- FSE (RFC 8878 4.1) ----------------------------------------------------------------

class _Forward:
    """bits from the least significant bit of the first byte on (the table descriptions)"""

    def __init__(self, buf, pos, end):
        self.v = int.from_bytes(buf[pos:end], "little")
        self.n = (end - pos) * 8
        self.at = 0

    def read(self, bits):
        _need(self.at + bits <= self.n, "a table description runs beyond its section")
        r = (self.v >> self.at) & ((1 << bits) - 1)
        self.at += bits
        return r


def read_fse_description(buf, pos, end, max_log, max_symbol):
    """-> (the normalized counts [-1 = "less than 1"], the accuracy log, the position behind the description)"""
    f = _Forward(buf, pos, end)
    log = f.read(4) + 5
    _need(log <= max_log, "accuracy log %d beyond %d" % (log, max_log))
    remaining = 1 << log
    counts = []
    while remaining > 0:
        _need(len(counts) <= max_symbol, "more than %d symbols" % (max_symbol + 1))
        bits = (remaining + 1).bit_length()
        lower = (1 << (bits - 1)) - 1
        threshold = (1 << bits) - 1 - (remaining + 1)
        v = (f.v >> f.at) & ((1 << bits) - 1)  # (bits beyond the description read as zero; the position is checked below)
        if (v & lower) < threshold:
            f.at += bits - 1
            v &= lower
        else:
            f.at += bits
            if v > lower:
                v -= threshold
        _need(f.at <= f.n, "a table description runs beyond its section")
        p = v - 1
        remaining -= abs(p)
        _need(remaining >= 0, "the counts add up to more than the table")
        counts.append(p)
        if p == 0:
            while True:
                r = f.read(2)
                counts += [0] * r
                if r != 3:
                    break
    _need(len(counts) <= max_symbol + 1, "more than %d symbols" % (max_symbol + 1))
    return counts, log, pos + (f.at + 7) // 8


def fse_decode_table(counts, log):
    """[(symbol, bits, baseline)] per state (4.1.1)"""
    size = 1 << log
    symbols = [0] * size
    high = size
    for s, c in enumerate(counts):
        if c == -1:
            high -= 1
            symbols[high] = s
    step, mask, pos = (size >> 1) + (size >> 3) + 3, size - 1, 0
    for s, c in enumerate(counts):
        for _ in range(max(c, 0)):
            symbols[pos] = s
            pos = (pos + step) & mask
            while pos >= high:
                pos = (pos + step) & mask
    _need(pos == 0, "the counts do not fill the table")
    nxt = [max(abs(c), 1) for c in counts]
    table = []
    for st in range(size):
        s = symbols[st]
        x = nxt[s]
        nxt[s] += 1
        bits = log - (x.bit_length() - 1)
        table.append((s, bits, (x << bits) - size))
    return table


class _Backward:
    """the bit stream that is read from its last byte's end mark backwards (4.1: FSE and the sequences)"""

    def __init__(self, buf, pos, end):
        _need(end > pos and buf[end - 1] != 0, "a bit stream without its end mark")
        self.v = int.from_bytes(buf[pos:end], "little")
        self.at = (end - pos - 1) * 8 + buf[end - 1].bit_length() - 1  # the bits below the end mark

    def read(self, bits):
        """(beyond the stream's start: zeros, and `at` goes negative -- the callers look at it)"""
        self.at -= bits
        return (self.v >> self.at) & ((1 << bits) - 1) if self.at >= 0 else 0


def _table_for(mode, buf, pos, end, default, max_log, max_symbol, previous):
    """-> (decode table, its description for describe(), the position behind what the mode wrote)"""
    if mode == 0:
        return fse_decode_table(*default), {"log": default[1], "counts": None}, pos
    if mode == 1:
        _need(pos < end, "the RLE symbol is missing")
        _need(buf[pos] <= max_symbol, "RLE symbol %d beyond %d" % (buf[pos], max_symbol))
        return [(buf[pos], 0, 0)], {"log": 0, "symbol": buf[pos], "counts": None}, pos + 1
    if mode == 2:
        counts, log, at = read_fse_description(buf, pos, end, max_log, max_symbol)
        return fse_decode_table(counts, log), {"log": log, "counts": counts, "bytes": at - pos}, at
    _need(previous is not None, "repeat mode without a table before it")
    return previous, {"log": None, "counts": None}, pos


def _max_bits(weights):
    """the longest code of a tree description: the weights add up (in units of 2^(w - 1)) to just below a power of two, the last symbol's weight fills it"""
    total = sum(1 << (w - 1) for w in weights if w)
    _need(total > 0, "a tree description without a weight")
    return total.bit_length()


def read_huffman_weights(buf, pos, end):
    """the tree description at `pos` (4.2.1): -> ({form: "direct" | "fse", count: the weights written, log: the FSE table's accuracy log}, the position behind it)"""
    h = buf[pos]
    if h >= 128:
        n = h - 127
        _need(pos + 1 + (n + 1) // 2 <= end, "direct weights beyond the section")
        w = [(buf[pos + 1 + i // 2] >> (4 if i % 2 == 0 else 0)) & 15 for i in range(n)]
        return {"form": "direct", "count": n, "log": None, "weights": w, "max_bits": _max_bits(w), "bytes": 1 + (n + 1) // 2}, pos + 1 + (n + 1) // 2
    _need(h > 0 and pos + 1 + h <= end, "compressed weights beyond the section")
    counts, log, at = read_fse_description(buf, pos + 1, pos + 1 + h, 6, 12)
    table = fse_decode_table(counts, log)
    b = _Backward(buf, at, pos + 1 + h)
    s1 = b.read(log)
    s2 = b.read(log)
    w = []
    while True:  # two states in turn; the stream ends where a state's update would read beyond its start
        sym, bits, base = table[s1]
        w.append(sym)
        if b.at < bits:
            w.append(table[s2][0])
            break
        s1 = base + b.read(bits)
        sym, bits, base = table[s2]
        w.append(sym)
        if b.at < bits:
            w.append(table[s1][0])
            break
        s2 = base + b.read(bits)
        _need(len(w) <= 255, "more than 255 weights")
    return {"form": "fse", "count": len(w), "log": log, "weights": w, "max_bits": _max_bits(w), "bytes": 1 + h}, pos + 1 + h


# ---------------------------------------------------------------- the frame reader ----------------------------------------------------------------

def describe(frame):
    """What a Zstd frame says, from RFC 8878: the frame header's fields and per block its type, the literals section's header (and, for a new Huffman
    table, how its weights are written), the sequence count and its byte form, the three table modes, and the sequences as (literal_length, offset_value,
    match_length) with `offsets`: the distances they copy from, repeat offsets resolved across the frame's blocks.  Raises Malformed."""
    frame = bytes(frame)
    try:
        return _describe(frame)
    except (IndexError, AssertionError) as e:
        raise Malformed("truncated or not a frame: %r" % (e,))


def _describe(frame):
    h = zc.read_frame_header(frame)
    _need(h["descriptor"] & 8 == 0, "reserved bit in the frame header")
    pos = h.pop("end")
    blocks = []
    rep = [1, 4, 8]
    tables = [None, None, None]
    have_tree = False
    while True:
        _need(pos + 3 <= len(frame), "block header beyond the frame")
        last, kind, size = zc.read_block_header(frame, pos)
        pos += 3
        _need(kind != 3, "reserved block type")
        b = {"type": ("raw", "rle", "compressed")[kind], "last": bool(last), "size": size, "at": pos}
        if kind < 2:
            _need(pos + (1 if kind == 1 else size) <= len(frame), "block beyond the frame")
            b["regenerated"] = size
            pos += 1 if kind == 1 else size
        else:
            _need(size >= 2 and size <= BLOCK and pos + size <= len(frame), "compressed block of %d bytes" % size)
            end = pos + size
            lit = zc.read_literals_header(frame, pos)
            _need(lit["end"] < end, "literals section beyond the block")
            weights = None
            if lit["kind"] == 2:
                weights, at = read_huffman_weights(frame, pos + lit["header_bytes"], lit["end"])
                weights = {k: v for k, v in weights.items()}
                have_tree = True
                if lit["streams"] == 4:
                    _need(at + 6 <= lit["end"], "jump table beyond the literals")
            if lit["kind"] == 3:
                _need(have_tree, "treeless literals without a table before them")
            b["literals"] = {"kind": zc.LITERAL_KINDS[lit["kind"]], "form": lit["form"], "header_bytes": lit["header_bytes"], "regenerated": lit["regenerated"],
                             "compressed": lit["compressed"], "streams": lit["streams"], "weights": weights}
            nseq, form, at = zc.read_sequence_count(frame, lit["end"])
            _need(at <= end, "sequence count beyond the block")
            b["nseq"], b["count_form"] = nseq, zc.COUNT_FORMS[form]
            b["modes"], b["tables"], b["sequences"], b["offsets"], b["codes"] = None, None, [], [], []
            if nseq == 0:
                _need(at == end, "bytes behind an empty sequences section")
            else:
                _need(at < end, "modes byte beyond the block")
                m = frame[at]
                _need(m & 3 == 0, "reserved bits in the modes byte")
                modes = (m >> 6, (m >> 4) & 3, (m >> 2) & 3)
                at += 1
                desc = []
                for k, (default, max_log, max_symbol) in enumerate(((LL_DEFAULT, 9, 35), (OF_DEFAULT, 8, 31), (ML_DEFAULT, 9, 52))):
                    tables[k], d, at = _table_for(modes[k], frame, at, end, default, max_log, max_symbol, tables[k])
                    desc.append(d)
                b["modes"] = tuple(MODES[x] for x in modes)
                b["tables"] = dict(zip(("ll", "of", "ml"), desc))
                _need(at < end, "no bit stream behind the tables")
                b["stream_bytes"] = end - at
                bits = _Backward(frame, at, end)
                sl, so, sm = bits.read(len(tables[0]).bit_length() - 1), bits.read(len(tables[1]).bit_length() - 1), bits.read(len(tables[2]).bit_length() - 1)
                _need(bits.at >= 0, "the bit stream is shorter than its initial states")
                for i in range(nseq):
                    cl, bl, basel = tables[0][sl]
                    co, bo, baseo = tables[1][so]
                    cm, bm, basem = tables[2][sm]
                    _need(cl <= 35 and cm <= 52 and co <= 31, "a code beyond its alphabet")
                    ov = (1 << co) + bits.read(co)
                    ml = zc.ML_BASE[cm] + bits.read(zc.ML_BITS[cm])
                    ll = zc.LL_BASE[cl] + bits.read(zc.LL_BITS[cl])
                    _need(bits.at >= 0, "the bit stream ends inside sequence %d" % i)
                    b["sequences"].append((ll, ov, ml))
                    b["codes"].append((cl, co, cm))
                    if i + 1 < nseq:
                        sl = basel + bits.read(bl)
                        sm = basem + bits.read(bm)
                        so = baseo + bits.read(bo)
                        _need(bits.at >= 0, "the bit stream ends behind sequence %d" % i)
                _need(bits.at == 0, "%d bits left over behind the last sequence" % bits.at)
                # repeat offsets (3.1.1.5)
                for ll, ov, ml in b["sequences"]:
                    if ov > 3:
                        o = ov - 3
                        rep = [o, rep[0], rep[1]]
                    else:
                        idx = ov - 1 + (1 if ll == 0 else 0)
                        if idx == 0:
                            o = rep[0]
                        else:
                            o = rep[0] - 1 if idx == 3 else rep[idx]
                            _need(o != 0, "repeat offset 0")
                            if idx != 1:
                                rep[2] = rep[1]
                            rep[1] = rep[0]
                            rep[0] = o
                    b["offsets"].append(o)
                total = sum(s[0] + s[2] for s in b["sequences"])
                _need(sum(s[0] for s in b["sequences"]) <= lit["regenerated"], "the literal lengths exceed the literals")
                b["last_literals"] = lit["regenerated"] - sum(s[0] for s in b["sequences"])
                b["regenerated"] = total + b["last_literals"]
            if nseq == 0:
                b["last_literals"] = lit["regenerated"]
                b["regenerated"] = lit["regenerated"]
            _need(b["regenerated"] <= BLOCK, "a block of more than 128 KiB")
            pos = end
        blocks.append(b)
        if last:
            break
    if h["checksum"]:
        _need(pos + 4 <= len(frame), "checksum beyond the frame")
        h["checksum_value"] = int.from_bytes(frame[pos:pos + 4], "little")
        pos += 4
    _need(pos == len(frame), "%d bytes behind the frame" % (len(frame) - pos))
    h["blocks"] = blocks
    h["regenerated"] = sum(b["regenerated"] for b in blocks)
    _need(h["content_size"] is None or h["content_size"] == h["regenerated"], "the blocks regenerate %d bytes, the header says %r" % (h["regenerated"], h["content_size"]))
    return h


# ---------------------------------------------------------------- a case against its frame ----------------------------------------------------------------

def block_literals(data, d):
    """the literal bytes of every block of `d` = describe(frame of data) (b"" for raw and RLE blocks), with the reasons the sequences do not fit the plaintext:
    every match must repeat the plaintext at its offset, the lengths must add up"""
    bad, out, pos = [], [], 0
    for k, b in enumerate(d["blocks"]):
        if b["type"] != "compressed":
            out.append(b"")
            pos += b["regenerated"]
            continue
        start, lits = pos, bytearray()
        for i, ((ll, _, ml), off) in enumerate(zip(b["sequences"], b["offsets"])):
            lits += data[pos:pos + ll]
            pos += ll
            if off > pos:
                bad.append("block %d sequence %d: offset %d at position %d" % (k, i, off, pos))
            elif off >= ml and data[pos:pos + ml] != data[pos - off:pos - off + ml] or off < ml and data[pos:pos + ml] != (data[pos - off:pos] * (ml // off + 1))[:ml]:
                bad.append("block %d sequence %d: the %d bytes at %d are not those %d before" % (k, i, ml, pos, off))
            pos += ml
        lits += data[pos:pos + b["last_literals"]]
        pos += b["last_literals"]
        if pos - start != b["regenerated"] or len(lits) != b["literals"]["regenerated"]:
            bad.append("block %d adds up to %d bytes, %d literals" % (k, pos - start, len(lits)))
        out.append(bytes(lits))
    if pos != len(data):
        bad.append("the blocks add up to %d of %d bytes" % (pos, len(data)))
    return out, bad


def huffman_depth(counts):
    """the depth of an unlimited Huffman tree of these symbol counts (where counts tie the shallower tree: the least a builder can reach)"""
    import heapq
    heap = [(c, 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def zero_runs(counts):
    """how many zeros follow each zero that a table description writes (what its repeat flags encode)"""
    runs, i = [], 0
    while i < len(counts):
        if counts[i] == 0:
            j = i
            while j < len(counts) and counts[j] == 0:
                j += 1
            runs.append(j - i - 1)
            i = j
        else:
            i += 1
    return runs


def _get(b, key):
    for part in key.split("."):
        if b is None:
            return None
        b = b.get(part) if isinstance(b, dict) else None
    return b


def _block_misses(b, want, lits):
    bad = []
    for key, v in want.items():
        if key == "huffman_depth_over":  # the literals' own tree is deeper than v, the written one is not
            w = _get(b, "literals.weights.weights") or []
            hist = np.bincount(np.frombuffer(lits, dtype=np.uint8), minlength=256).tolist()
            if not (huffman_depth(hist) > v and w and _get(b, "literals.weights.max_bits") <= v):
                bad.append("tree depth %d, written bits %r: not limited to %d" % (huffman_depth(hist), _get(b, "literals.weights.max_bits"), v))
        elif key == "largest_count":  # of the literals' histogram: what the (n >> 7) + 4 shortcut looks at
            got = int(np.bincount(np.frombuffer(lits, dtype=np.uint8), minlength=256).max()) if lits else 0
            if got != v:
                bad.append("largest literal count %d, expected %d" % (got, v))
        elif key == "symbols":
            if len(set(lits)) != v:
                bad.append("%d distinct literals, expected %d" % (len(set(lits)), v))
        elif key == "weights_equal":
            w = _get(b, "literals.weights.weights") or [0, 1]
            if len(set(w)) != 1:
                bad.append("weights %r are not all equal" % w[:20])
        elif key == "max_bits":
            if _get(b, "literals.weights.max_bits") != v:
                bad.append("table of %r bits, expected %d" % (_get(b, "literals.weights.max_bits"), v))
        elif key.endswith(".zero_runs"):  # [(lo, hi)]: a run of zeros of lo..hi symbols in this table's description
            runs = zero_runs(_get(b, key[:-10] + ".counts") or [])
            bad += ["no run of %d..%d zeros in %r" % (lo, hi, runs) for lo, hi in v if not any(lo <= r <= hi for r in runs)]
        elif key.endswith(".has_count"):  # a normalized count of this value (-1: "less than one")
            if v not in (_get(b, key[:-10] + ".counts") or []):
                bad.append("no count %d in %s" % (v, key[:-10]))
        elif key.endswith(">=") or key.endswith("<="):
            got = _get(b, key[:-2])
            if got is None or (got < v if key.endswith(">=") else got > v):
                bad.append("%s is %r, expected %s %r" % (key[:-2], got, key[-2:], v))
        elif _get(b, key) != v:
            bad.append("%s is %r, expected %r" % (key, _get(b, key), v))
    return bad


def check(data, frame, expect):
    """-> the list of what `frame` (the oracle's frame of `data`) lacks of `expect`; [] is a case that reaches its edge.  Whatever `expect` says, the frame
    must read as RFC 8878 says and its sequences must rebuild the plaintext.  Keys of `expect` (sequences are (literal_length, offset_value, match_length),
    None in a pattern is "any"):
      frame: {field: value} of the frame header;  nblocks;  types: the block types in order;
      blocks: {index: {key: value}} -- keys are describe()'s, dotted ("literals.kind", "literals.weights.form", "tables.of.log", "modes", "nseq",
              "count_form", "last_literals"), with >= / <= behind a key for a bound, and huffman_depth_over, symbols, weights_equal, max_bits,
              tables.X.zero_runs, tables.X.has_count (see _block_misses);  any: {key: value} that some compressed block must meet;
      exact: {index: the block's sequences};  has: [run, ...] (patterns next to each other in one block);  none: [pattern, ...];
      count / min_count: sequences in the frame;  offset: the largest distance copied from;  max_offset: a bound on it;
      rep: [(offset_value, literals before it: True / False)] repeat-offset uses that must occur;  codes: {"ll" | "of" | "ml": [code, ...]} that must occur."""
    try:
        d = describe(frame)
    except Malformed as e:
        return ["the frame does not read: %s" % e]
    lits, bad = block_literals(data, d)
    blocks = d["blocks"]
    comp = [b for b in blocks if b["type"] == "compressed"]
    seqs = [s for b in comp for s in b["sequences"]]
    offs = [o for b in comp for o in b["offsets"]]
    for key, want in expect.items():
        if key == "frame":
            bad += ["frame header %s is %r, expected %r" % (k, d.get(k), v) for k, v in want.items() if d.get(k) != v]
        elif key == "nblocks":
            if len(blocks) != want:
                bad.append("%d blocks, expected %d" % (len(blocks), want))
        elif key == "types":
            if [b["type"] for b in blocks] != list(want):
                bad.append("blocks %r, expected %r" % ([b["type"] for b in blocks], list(want)))
        elif key == "blocks":
            for k, w in want.items():
                if k >= len(blocks):
                    bad.append("no block %d" % k)
                else:
                    bad += ["block %d: %s" % (k, m) for m in _block_misses(blocks[k], w, lits[k])]
        elif key == "any":
            if not any(not _block_misses(b, want, lits[blocks.index(b)]) for b in comp):
                bad.append("no compressed block with %r" % (want,))
        elif key == "exact":
            for k, w in want.items():
                got = blocks[k].get("sequences") if k < len(blocks) else None
                if got != list(w):
                    at = next((i for i, (a, b) in enumerate(zip(got or [], w)) if a != b), min(len(got or []), len(w)))
                    bad.append("block %d has %d sequences, expected %d; from %d on %r, expected %r" % (k, len(got or []), len(w), at, (got or [])[at:at + 3], list(w)[at:at + 3]))
        elif key == "has":
            bad += ["no %r in %r" % (run, seqs[:8]) for run in want if not any(ec._has_run(b["sequences"], run) for b in comp)]
        elif key == "none":
            bad += ["%r among the sequences" % (p,) for p in want if ec._has_run(seqs, [p])]
        elif key == "count":
            if len(seqs) != want:
                bad.append("%d sequences, expected %d" % (len(seqs), want))
        elif key == "min_count":
            if len(seqs) < want:
                bad.append("%d sequences, expected at least %d" % (len(seqs), want))
        elif key == "offset":
            if max(offs, default=0) != want:
                bad.append("largest offset %d, expected %d" % (max(offs, default=0), want))
        elif key == "max_offset":
            if max(offs, default=0) > want:
                bad.append("offset %d beyond %d" % (max(offs), want))
        elif key == "rep":
            uses = {(s[1], s[0] > 0) for s in seqs if s[1] <= 3}
            bad += ["no repeat offset value %d with ll %s 0" % (v, ">" if with_ll else "=") for v, with_ll in want if (v, with_ll) not in uses]
        elif key == "codes":
            for which, col in (("ll", 0), ("of", 1), ("ml", 2)):
                have = {c[col] for b in comp for c in b["codes"]}
                bad += ["no %s code %d" % (which, c) for c in want.get(which, ()) if c not in have]
        else:
            raise KeyError(key)
    return bad


# ---------------------------------------------------------------- building inputs ----------------------------------------------------------------
# The match finder (DoubleFastBlockCompressor) probes every position of a literal run while the run is shorter than 256 bytes, then every
# ((position - anchor) >> 8) + 1; it finds a second occurrence of 8 bytes (long table) or of 4 / 5 (short table; 5 where the input is 16 KiB + 1 .. 128 KiB or
# beyond 256 KiB) where the first was probed, extends it backwards while the bytes before agree, and tests the last offset one position ahead first.  A
# position in the middle of a match is not in the tables.  So: filler without a repeated 4-gram never matches; `again` of bytes that began in a literal
# run, with a different byte before and behind, is one sequence of exactly that length and offset.

_streams = {}


def _stream(key, counts, n=None, seed=1, avoid=b""):
    """bytes with exactly these symbol counts ({symbol: count}; n = None) or drawn by these weights (n bytes), no 4-gram twice; cached under `key`"""
    if key in _streams:
        return _streams[key]
    syms = np.array(sorted(counts), dtype=np.int64)
    for attempt in range(50):
        rng = np.random.default_rng(seed * 1000 + attempt)
        left = np.array([counts[s] for s in syms], dtype=np.float64)
        total = int(left.sum()) if n is None else n
        out, seen, ok = [], {int.from_bytes(avoid[i:i + 4], "big") for i in range(len(avoid) - 3)}, True
        g = 0
        draws = rng.random(total * 8).tolist()
        di = 0
        for _ in range(total):
            for tries in range(60):
                if di >= len(draws):
                    draws, di = rng.random(total * 8).tolist(), 0
                cum = np.cumsum(left)
                k = int(np.searchsorted(cum, draws[di] * cum[-1], side="right"))
                di += 1
                k = min(k, len(syms) - 1)
                s = int(syms[k])
                gg = ((g << 8) | s) & 0xFFFFFFFF
                if len(out) < 3 or gg not in seen:
                    break
            else:
                ok = False
                break
            out.append(s)
            g = gg
            if len(out) >= 4:
                seen.add(g)
            if n is None:
                left[k] -= 1
        if ok:
            _streams[key] = bytes(out)
            return _streams[key]
    raise AssertionError("no stream for %r" % (key,))


def text_like(n, seed=1, symbols=200, power=0.7, avoid=b""):
    """n bytes over a skewed alphabet of `symbols` letters (Huffman gains about an eighth), no 4-gram twice -- and few enough 4-grams alike that a literal
    run's last bytes with a match's first ones seldom repeat one by chance"""
    w = {40 + i: (i + 1.0) ** -power for i in range(symbols)}
    return _stream(("text", n, seed, symbols, power, len(avoid)), w, n=n, seed=seed, avoid=avoid)


class Z(ec._B):
    """an input under construction (encoder_edge_cases._B: fill / again / run / byte), with literals of a chosen kind"""

    def __init__(self, salt=0, literals=None):
        super().__init__(salt)
        self.src, self.at = literals, 0  # literals: bytes to draw the filler from (None: the pool of random bytes, which Huffman coding does not shrink)

    def fill(self, n, before=None):
        if self.src is None:
            return super().fill(n, before)
        not_last = self.d[before - 1] if before else None
        if n == 0:
            return super().fill(0, before)
        while self.src[self.at] == self.ban or self.src[self.at + n - 1] == not_last:
            self.at += 1
        self.ban = None
        self.d += self.src[self.at:self.at + n]
        self.at += n
        return self

    def again(self, src, n):
        if src + n < len(self.d):  # (no overlap: a slice)
            if self.ban is not None and self.d[src] == self.ban:
                raise ec._Retry()
            self.d += self.d[src:src + n]
            self.ban = self.d[src + n]
            return self
        return super().again(src, n)

    def seq(self, ll, offset, ml):
        """one sequence: ll fresh bytes, then the ml bytes `offset` back once more"""
        src = len(self.d) + ll - offset
        assert src >= 1, "position 0 is never in the tables"
        if src > len(self.d):  # (the source lies in this sequence's own literals)
            ll -= src - len(self.d)
            self.fill(src - len(self.d))
        self.fill(ll, before=src)
        if ll == 0 and self.d[-1] == self.d[src - 1]:
            raise ec._Retry()
        return self.again(src, ml)

    def done(self, tail=0):
        if tail:
            self.fill(tail)
        return bytes(self.d)


def of_code(offset):
    """the offset code of a real offset (its value is offset + 3)"""
    return (offset + 3).bit_length() - 1


class S(Z):
    """... that keeps the sequences it builds (`want`: what the oracle's block must hold) and the two offsets the match finder carries"""

    def __init__(self, salt=0, literals=None):
        super().__init__(salt, literals)
        self.want, self.o1, self.o2, self.spots, self.pending = [], 1, 0, {}, 0  # (spots: an ordered set)

    def fill(self, n, before=None):
        at = len(self.d)
        super().fill(n, before)
        self.pending += n
        self.spots.update((q, None) for q in range(max(at, 1), min(len(self.d), at + 250), 12))  # (every 12th: a source's eight bytes are used once)
        return self

    def _close(self, value, ml):
        self.want.append((self.pending, value, ml))
        self.pending = 0

    def seq(self, ll, offset, ml):
        src = len(self.d) + ll - offset
        for q in list(range(src - 3, src + 4)) + list(range(src + ml - 4, src + ml + 1)):  # (their bytes have a later occurrence in the tables now)
            self.spots.pop(q, None)
        super().seq(ll, offset, ml)
        if offset == self.o1 and self.pending:  # (the match finder tries the last offset first)
            self._close(1, ml)
            return self
        self._close(offset + 3, ml)
        self.o1, self.o2 = offset, self.o1
        return self

    def coded(self, ll, code, ml):
        """a sequence whose offset has this code: its source is a spot of an earlier literal run that no sequence has used"""
        pos = len(self.d) + ll
        if len(self.d) and of_code(ll) == code and ll >= 8:
            return self.seq(ll, ll, ml)  # (the start of its own literals)
        for p in self.spots:
            if of_code(pos - p) == code and p + 8 <= pos:
                return self.seq(ll, pos - p, ml)
        raise AssertionError("no source for offset code %d at %d" % (code, pos))

    def rep(self, ll, ml):
        """the last offset once more behind ll >= 1 literals: offset value 1"""
        assert ll >= 1
        src = len(self.d) + ll - self.o1
        self.fill(ll, before=src)
        self.again(src, ml)
        self._close(1, ml)
        return self

    def rep0(self, ml):
        """the offset before the last one right behind a match: offset value 1 with no literals, the two offsets change places"""
        assert self.pending == 0
        self.again(len(self.d) - self.o2, ml)
        self._close(1, ml)
        self.o1, self.o2 = self.o2, self.o1
        return self

    def next_block(self):
        """the block ends here (in literals)"""
        self.blocks = getattr(self, "blocks", []) + [self.want]
        self.want, self.pending = [], 0
        return self

    def runs(self, k, n=200):
        """k literal runs of n bytes (sources for later sequences), a short match between them"""
        for _ in range(k):
            self.seq(n, n - 60 - len(self.want), 10)
        return self


def _try(fn, *args, **kw):
    for salt in range(40):
        try:
            return fn(salt, *args, **kw)
        except ec._Retry:
            continue
    raise AssertionError("no salt for %s%r" % (fn.__name__, args))


# ---------------------------------------------------------------- the catalog ----------------------------------------------------------------

def _t2():
    """... and the few-letter one for literals of a few hundred bytes, where a table of 200 weights would cost more than it gains (its letters are T's most
    frequent ones: a table built for T codes them)"""
    return text_like(6000, seed=2, symbols=24, power=1.0)


def _t(n=40000):
    """the skewed literals most cases draw from (Huffman codes them at about five bits a byte)"""
    return text_like(n)


def _lits_then_match(salt, lits, n, ml=None, tail=0):
    """n literals drawn from `lits`, one match of the bytes from position 8 on, `tail` more literals: (data, the sequence)"""
    ml = ml or (24 + (n >> 8) * 2)
    z = S(salt, lits)
    z.seq(n, n - 8, ml)
    return z.done(tail), z.want


def _compressible(n, salt=0, head=b""):
    """n bytes that one block compresses well whatever its parameters: `head`, 600 bytes of text-like filler, and the filler over and over"""
    z = Z(salt, _t() if n > 2000 else _t2())
    z._push(head)
    z.fill(600)
    start = len(z.d) - 599
    while len(z.d) < n:
        z.again(start, min(n - len(z.d), 65000))
        if len(z.d) < n:
            z.fill(min(n - len(z.d), 40))
    return bytes(z.d[:n])


def _sequences(salt, spec, literals=None, runs=4, tail=9):
    """spec: [(ll, offset code | "rep" | "rep0" | ("at", offset), ml)] -> (data, the block's sequences)"""
    z = S(salt, literals)
    z.runs(runs)
    for ll, how, ml in spec:
        if how == "rep":
            z.rep(ll, ml)
        elif how == "rep0":
            z.rep0(ml)
        elif isinstance(how, tuple):
            z.seq(ll, how[1], ml)
        else:
            z.coded(ll, how, ml)
    return z.done(tail), z.want


_cases = None


def cases():
    """[(name, data, expect)], built once"""
    global _cases
    if _cases is None:
        out = []
        for build in (_frame_cases, _block_and_reuse_cases, _sequence_cases, _literal_cases, _window_cases, _gain_and_table_cases):
            build(lambda name, data, expect: out.append((name, bytes(data), expect)))
        _cases = out
    return _cases


def emulator_cases(variant=None, limit=20000):
    """the cases an emulator run takes: everything up to `limit` bytes but some that repeat a neighbour's path at another size, and the larger ones that
    are runs and filler (few sequences).  variant: 0 and 2 emit every sequence from one lane and leave out the three cases of thousands of sequences,
    whose edges lie in the entropy stage (the default variant 3 and variant 1 take them)."""
    import re
    return [c for c in cases() if ((len(c[1]) <= limit and not re.match(EMULATOR_SKIP, c[0]) and c[0] not in _highest_of_a_code) or c[0] in EMULATOR_LARGE)
            and not (variant in (0, 2) and c[0] in EMULATOR_MANY_SEQUENCES)]


_highest_of_a_code = set()  # (filled by the catalog: a code's highest length or offset takes the path of its lowest with other extra bits)
EMULATOR_SKIP = r"sequences/count=(4|5|37|62|63|67|73|125|131|19[123]|25[567])$|frame/size=(3|4|5|10|12|15|17|24|31|33|127|129|511|513|2047|2049|8191|8193)$"
# (seconds each on the emulator: long matches and long literal runs are cheap there; what costs is a sequence)
EMULATOR_MANY_SEQUENCES = {"literals/rle/4095", "literals/rle/4096", "sequences/count=2100"}
EMULATOR_LARGE = {"blocks/last-block-of-6/raw", "literals/rle/64", "literals/rle/4095", "frame/size=262145/search-length-5", "literals/huffman/two-symbols", "literals/reuse/refused/a-symbol-has-no-code",
                  "literals/huffman/depth-limited/overpaid/one-over/a-leaf-of-rank-1-exists", "literals/huffman/depth-limited/overpaid/three-over/no-leaf-of-rank-1", "blocks/raw-in-the-middle/repeat-offsets-kept,table-reused", "literals/rle/4096",
                  "literals/reuse/by-estimate/1025/reused", "literals/reuse/by-preference/1024/the-old-table-gains-nothing", "literals/reuse/by-estimate/1025/new-table-wins",
                  "literals/huffman/weights-all-equal/direct", "literals/huffman/weights-all-different/direct", "sequences/ll-code=35/ll=65536",
                  "sequences/ml-code=52/ml=65539", "sequences/count=2100", "frame/window/first-occurrence-at-the-window-base/matched"}


def _fcs_bytes(n):
    return 1 if n < 256 else (2 if n < 65536 + 256 else 4)


def _single(n):
    """the frame header of a single-segment frame of n bytes"""
    return {"single_segment": True, "content_size": n, "content_size_bytes": _fcs_bytes(n), "checksum": True, "window_descriptor": None}


def _frame_cases(add):
    T, T2, single = _t(), _t2(), _single
    # ---- frame and parameters: sizes at which CompressionParameters.compute and the frame header change ----
    for n in (0, 1, 6, 7, 8):
        add("frame/size=%d/raw-block" % n, T[:n], {"frame": single(n), "types": ["raw"]})
    for n in (2, 3, 4, 5, 9, 10, 12, 15, 16, 17, 24, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 511, 512, 513, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 8191, 8192, 8193, 32768, 32769, 65791, 65792):
        add("frame/size=%d" % n, _compressible(n, salt=n % 7), dict({"frame": single(n), "types": ["compressed" if n >= 64 else "raw"]}, **({"min_count": 1} if n > 1000 else {"count": 0})))
    # the four rows of the level's table differ in the search length: a second occurrence of exactly four bytes is a match at 4, none at 5
    for n, found in ((16384, True), (16385, False), (131072, False), (131073, True), (262144, True), (262145, False)):
        z = Z(n % 5, T)
        z.fill(120)
        z.again(40, 4)
        z.fill(30)
        head = bytes(z.d)
        data = _compressible(n, salt=1, head=head)
        e = {"frame": single(n), "types": ["compressed"] * (n // BLOCK) + (["raw"] if n % BLOCK == 1 else ["compressed"] * (n % BLOCK > 0))}
        e["has" if found else "none"] = [[(120, 83, 4)]] if found else [(None, None, 4)]
        add("frame/size=%d/search-length-%d" % (n, 4 if found else 5), data, e)

    # ---- literals: raw below 64, RLE, the shortcut, Huffman in every header form ----
    for n in (63, 64):
        add("literals/%d/%s" % (n, "raw" if n == 63 else "huffman"), *_one(T2, n, {"literals.kind": "raw" if n == 63 else "compressed", "literals.regenerated": n}))
    for n in (64, 4095, 4096):  # an RLE literals section: n equal bytes that no match covers -- they stand between matches, one a sequence
        add("literals/rle/%d" % n, *_rle_literals(n))
    for n, streams, form in ((255, 1, 0), (256, 4, 1), (257, 4, 1), (258, 4, 1), (259, 4, 1), (1023, 4, 1), (1024, 4, 2), (1025, 4, 2), (16383, 4, 2), (16384, 4, 3)):
        add("literals/huffman/%d/streams=%d,form=%d" % (n, streams, form), *_one(T2 if n < 2000 else T, n, {"literals.kind": "compressed", "literals.regenerated": n, "literals.streams": streams, "literals.form": form}))
    add("literals/huffman/no-sequences", T2[:500], {"types": ["compressed"], "count": 0, "blocks": {0: {"literals.kind": "compressed", "nseq": 0, "count_form": "one byte"}}})


def _one(lits, n, want, tail=0):
    data, seqs = _try(_lits_then_match, lits, n, tail=tail)
    return data, {"types": ["compressed"], "exact": {0: seqs}, "blocks": {0: want}}


_dicts = {}


def _dict_block(text, salt=0):
    """an S whose first block (131072 bytes) is written: literal runs of 240 bytes (sources for the blocks behind it) between short matches, two long
    matches, two sequences that leave the offsets `o1`, `o2`, 24 last literals.  text: literals from the skewed alphabet (the block leaves a Huffman
    table behind) or from the pool of random bytes (raw literals, and far more sources).  A copy per caller."""
    import copy
    if (text, salt) not in _dicts:
        z = S(salt, _t() if text else None)
        for k in range(32 if text else 380):  # (text: fewer runs, a cheaper block for the emulator -- 7.7 KB of literals still give every letter a code)
            z.seq(240, 100 + (k * 37) % 90, 16)
        rest = BLOCK - len(z.d) - 2 * (10 + 20) - 24 - 2 * 8
        z.seq(8, len(z.d) + 8 - 1, rest // 2)
        z.seq(8, len(z.d) + 8 - 13, rest - rest // 2)
        z.coded(10, 16, 20)
        z.coded(10, 16, 20)
        z.fill(24)
        assert len(z.d) == BLOCK
        z.next_block()
        _dicts[(text, salt)] = z
    return copy.deepcopy(_dicts[(text, salt)])


def _rle_literals(n):
    """The literals of a block are an RLE section where every byte that no match covers is the same: the second block repeats the first at the offset its
    last sequence left, but for every tenth byte, which is 0 (the text has none) -- n sequences of one literal and nine bytes at the repeat offset.
    -> (data, expectation)"""
    z = _dict_block(True)
    for i in range(n):
        z.byte(0)
        z.pending += 1
        z.again(len(z.d) - z.o1, 9)
        z._close(1, 9)
    return bytes(z.d), {"types": ["compressed", "compressed"], "exact": {1: z.want},
                        "blocks": {1: {"literals.kind": "rle", "literals.regenerated": n, "literals.header_bytes": 2 if n < 4096 else 3, "last_literals": 0}}}


def _block_and_reuse_cases(add):
    T, single = _t(), _single
    # ---- blocks ----
    # (exactly two blocks, 2 x 131072: frame/size=262144 above; a last block of one byte: frame/size=131073; three blocks: frame/size=262145; last blocks of 2 .. 5 bytes: behind the far offsets and the most sequences)
    add("blocks/1-blocks/size=%d" % BLOCK, _compressible(BLOCK, salt=2), {"frame": single(BLOCK), "types": ["compressed"]})
    for k in (6, 7):  # (below 7 bytes compressBlock does not try; at 7 it tries and gains nothing)
        add("blocks/last-block-of-%d/raw" % k, _compressible(BLOCK + k, salt=k), {"frame": single(BLOCK + k), "types": ["compressed", "raw"], "blocks": {1: {"size": k, "last": True}}})
    # an incompressible block between compressible ones: its match finder runs and finds a match, its offsets and its table are not committed
    z = _dict_block(True)
    o1, o2 = z.o1, z.o2
    z.src, z.at = None, 0
    z.fill(BLOCK - 60)
    z.seq(0, 50000, 40)  # (a match in the raw block: the finder's own offsets move on)
    z.fill(20)
    assert len(z.d) == 2 * BLOCK
    z.next_block()
    z.o1, z.o2 = o1, o2
    z.src, z.at = T, 30000
    z.rep(1, 20)
    z.rep0(20)
    for i in range(6):
        z.coded(100, 17, 30)
    add("blocks/raw-in-the-middle/repeat-offsets-kept,table-reused", z.done(5),
        {"types": ["compressed", "raw", "compressed"], "exact": {0: z.blocks[0], 2: z.want}, "rep": [(1, True), (1, False)],
         "blocks": {0: {"literals.kind": "compressed"}, 2: {"literals.kind": "treeless", "literals.regenerated": 606, "literals.form": 1}}})
    # ---- table reuse ----
    tail = _stream("tail", {180 + i: 1.0 + i % 3 for i in range(60)}, n=3000, seed=5, avoid=T)
    # (reuse by preference, a valid table and at most 1024 literals: the third block of blocks/raw-in-the-middle)
    for name, n, lits, kind in (("by-estimate/1025/reused", 1025, T[30000:], "treeless"),
                                # letters that are rare in the first block: its table codes them, a table of their own would do better -- at 1024 the old one is preferred all the same, gains nothing, and the literals stay raw
                                ("by-preference/1024/the-old-table-gains-nothing", 1024, tail, "raw"), ("by-estimate/1025/new-table-wins", 1025, tail, "compressed"),
                                ("refused/a-symbol-has-no-code", 900, bytes(T[30000:30500]) + b"\x05" + bytes(T[30500:31000]), "compressed")):
        z = _dict_block(True)
        z.src, z.at = lits, 0
        z.coded(n, 17, 60)
        add("literals/reuse/" + name, z.done(), {"types": ["compressed", "compressed"], "exact": {1: z.want}, "blocks": {1: {"literals.kind": kind, "literals.regenerated": n}}})



def expected_mode(codes, default_log, allowed=True):
    """SequenceEncoder.selectEncodingType as the Java states it (strategy DFAST), for a case's own codes: what its name promises"""
    n, largest = len(codes), max(codes.count(c) for c in set(codes))
    if largest == n:
        return "predefined" if allowed and n <= 2 else "rle"
    if allowed and (n < ((1 << default_log) * 9) >> 3 or largest < n >> (default_log - 1)):
        return "predefined"
    return "fse"


def expected_modes(seqs):
    ll = [zc.ll_code(s[0]) for s in seqs]
    of = [s[1].bit_length() - 1 for s in seqs]
    ml = [zc.ml_code(s[2]) for s in seqs]
    return (expected_mode(ll, 6), expected_mode(of, 5, max(of) < 28), expected_mode(ml, 6))


def _own(salt, triples, first=(30, 22, 12), tail=9, literals=None):
    """sequences whose sources lie in their own literals (offset <= ll): [(ll, offset, ml)] behind a first one"""
    z = S(salt, literals)
    z.seq(*first)
    for ll, off, ml in triples:
        assert off <= ll
        z.seq(ll, off, ml)
    return z.done(tail), z.want


def _far(salt, offset, ml=24, last=0):
    """one sequence at exactly this offset: literal runs (the sources), long matches to get away from them, each block ending in eight literals -- and, with
    `last`, the rest of its block as one more long match and a last block of `last` bytes.  -> (the builder, the index of the sequence's block, that block's sequences)"""
    z = S(salt)
    z.runs(6, 240)
    p = next(q for q in z.spots if q > 300 and q + offset > len(z.d))
    target = p + offset  # where the match begins
    sources = iter(range(1, 230, 12))  # (the long matches' sources: positions of the first literal run, each used once)

    def long_match(end):
        z.seq(8, len(z.d) + 8 - next(sources), end - len(z.d) - 8)

    def end_block():
        long_match((len(z.d) // BLOCK + 1) * BLOCK - 8)
        z.fill(8)
        z.next_block()

    while target > (len(z.d) // BLOCK + 1) * BLOCK:
        end_block()
    if target - 12 - len(z.d) - 8 >= 40:
        long_match(target - 12)
    z.seq(target - len(z.d), offset, ml)
    at = len(getattr(z, "blocks", []))
    if not last:
        z.fill(9)
        return z, at, z.want
    end_block()
    z.fill(last)
    return z, at, z.blocks[at]


def _sequence_cases(add):
    kinds = {"ll": {"same": lambda i: 34, "varied": lambda i: (34, 34, 34, 36, 40, 50, 64)[i % 7]},
             "of": {"same": lambda i: (14, 17, 20, 25)[i % 4], "varied": lambda i: (6, 9, 9, 14, 14, 14, 30, 3)[i % 8]},
             "ml": {"same": lambda i: 9, "varied": lambda i: (8, 8, 8, 9, 12, 20, 40)[i % 7]}}
    for n in (20, 40, 80):
        for a in ("same", "varied"):
            for b in ("same", "varied"):
                for c in ("same", "varied"):
                    data, want = _try(_own, [(kinds["ll"][a](i), kinds["of"][b](i), kinds["ml"][c](i)) for i in range(n - 1)], first=(34, 14, 9))
                    m = expected_modes(want)
                    add("seq-modes/n=%d,codes-%s-%s-%s/ll=%s,of=%s,ml=%s" % (n, a, b, c, m[0], m[1], m[2]), data, {"types": ["compressed"], "exact": {0: want}, "blocks": {0: {"modes": m}}})
    # one code each, twice and three times: `sequenceCount <= 2` keeps the predefined tables, a third sequence makes them RLE
    for n in (2, 3):
        data, want = _try(_own, [(34, 17, 9), (34, 20, 9)][:n - 1], first=(34, 14, 9))
        m = expected_modes(want)
        assert m == (("predefined",) * 3 if n == 2 else ("rle",) * 3)
        add("seq-modes/n=%d,one-code-each/ll=%s,of=%s,ml=%s" % (n, m[0], m[1], m[2]), data, {"types": ["compressed"], "exact": {0: want}, "blocks": {0: {"modes": m}}})
    # match-length codes spread flat over 168 sequences: the predefined table beside two FSE tables; one code more often: FSE
    for flat in (True, False):
        mls = [zc.ML_BASE[1 + i % 42] for i in range(168)]  # (42 codes, four times each: 4 < 168 >> 5)
        if not flat:
            mls[50] = mls[9]
        data, want = _try(_own, [((34, 36, 40, 50)[i % 4], (6, 9, 14, 30, 14)[i % 5], ml) for i, ml in enumerate(mls[1:])], first=(34, 14, mls[0]))
        m = expected_modes(want)
        assert m == ("fse", "fse", "predefined" if flat else "fse"), m
        add("seq-modes/n=168/ml-codes-flat=%s/ml=%s" % (flat, m[2]), data, {"types": ["compressed"], "exact": {0: want}, "blocks": {0: {"modes": m}}})
    # counts: the one-byte form ends at 126; minNumberOfSequences 36 (offsets) and 72; the groups of 64 of the lane-parallel encoder
    for n in (1, 2, 3, 35, 36, 37, 63, 64, 65, 66, 71, 72, 73, 4, 5, 62, 67, 125, 126, 127, 128, 129, 130, 131, 191, 192, 193, 255, 256, 257, 600, 2100):  # (600: the FSE table logs come from the count alone, between their floor and their maximum)
        lean = n >= 600  # (short sequences: the emulator takes this one too)
        data, want = _try(_own, [((12, 13, 16, 20, 34)[i % 5] if not lean else (9, 10, 12)[i % 3], (6, 9, 11, 12)[i % 4] if not lean else (6, 9, 7, 8)[i % 4],
                                  (8, 9, 10, 12, 16, 33)[i % 6] if not lean else (8, 9)[i % 2]) for i in range(n - 1)], first=(34, 14, 9 if n > 3 else 30))
        add("sequences/count=%d" % n, data, {"types": ["compressed"], "exact": {0: want}, "count": n,
                                             "blocks": {0: {"nseq": n, "count_form": "one byte" if n < 127 else "two bytes", "modes": expected_modes(want)}}})
    # literal-length codes 16 .. 35, the lowest and the highest length of each
    for c in range(16, 36):
        for ll in sorted({zc.LL_BASE[c], zc.LL_BASE[c] + (1 << zc.LL_BITS[c]) - 1 if c < 35 else 70000}):
            z = _try(lambda salt: S(salt).seq(ll, ll - 8, ll // 30 + 40))
            _highest_of_a_code.update({"sequences/ll-code=%d/ll=%d" % (c, ll)} if ll != zc.LL_BASE[c] else ())
            add("sequences/ll-code=%d/ll=%d" % (c, ll), z.done(), {"types": ["compressed"], "exact": {0: z.want}, "codes": {"ll": [c]}})
    # match-length codes 32 .. 52
    for c in range(32, 53):
        for ml in sorted({zc.ML_BASE[c], zc.ML_BASE[c] + (1 << zc.ML_BITS[c]) - 1 if c < 52 else BLOCK - 60}):
            z = _try(lambda salt: S(salt).seq(40, 30, ml))
            _highest_of_a_code.update({"sequences/ml-code=%d/ml=%d" % (c, ml)} if ml != zc.ML_BASE[c] else ())
            add("sequences/ml-code=%d/ml=%d" % (c, ml), z.done(9 if ml < 60000 else 0), {"types": ["compressed"], "exact": {0: z.want}, "codes": {"ml": [c]}})
    # offset codes: 0 is the repeat offset; 1 (values 2 and 3) is never written: the finder knows two offsets and writes the second as value 1 with no
    # literals; 2 .. 19 the lowest and (up to 15) the highest offset of each.  20 is out of reach: the window is 2^20, a candidate lies beyond the window base
    # (the block's end - 2^20) and the finder stops eight bytes before the block's end, so an offset stays below 2^20 - 8 and offset + 3 below 2^20.
    # The cases of 17, 18 and 19 end in a last block of 4, 2 and 3 bytes, stored raw (1: frame/size=131073; 5: the most sequences; 6, 7: blocks/last-block-of).
    for c in range(2, 20):
        for off in sorted({(1 << c) - 3, (2 << c) - 4 if c < 16 else (1 << c) - 3}):
            last = {17: 4, 18: 2, 19: 3}.get(c, 0)
            name = "sequences/of-code=%d/offset=%d" % (c, off) + (",last-block-of-%d" % last if last else "")
            if off <= 30:
                z = _try(lambda salt: S(salt).seq(34, 14 if off != 14 else 20, 9).seq(34, off, 12))
                z.fill(9)
                at, want = 0, z.want
            else:
                z, at, want = _try(_far, off, last=last)
            if off != (1 << c) - 3:
                _highest_of_a_code.add(name)
            e = {"exact": {at: want}, "codes": {"of": [c]}, "has": [[(None, off + 3, None)]], "none": [(None, 2, None), (None, 3, None)]}
            if last:
                e.update({"types": ["compressed"] * (at + 1) + ["raw"], "blocks": {at + 1: {"size": last, "last": True}}})
            add(name, z.done(), e)
    z = _try(lambda salt: S(salt).seq(34, 14, 9).rep(1, 5).rep(3, 4).seq(20, 17, 9).rep0(6).rep0(4).rep(1, 7))
    add("sequences/repeat-offsets/value=1-with-and-without-literals", z.done(9), {"exact": {0: z.want}, "rep": [(1, True), (1, False)], "none": [(None, 2, None), (None, 3, None)], "codes": {"of": [0]}})


def _exact(key, counts, seed=1):
    return _stream(("exact", key), counts, seed=seed)


def _chosen_literals(lits, text=True):
    """a second block whose literals are exactly `lits`: it repeats the first block at the offset the first block's last sequence left, but for every tenth
    byte, which is the next of `lits` (bytes the first block does not have) -- one literal and nine bytes at the repeat offset per sequence"""
    z = _dict_block(text)
    for v in lits:
        z.byte(v)
        z.pending += 1
        z.again(len(z.d) - z.o1, 9)
        z._close(1, 9)
    return z


def _literal_cases(add):
    # the shortcut `largestCount <= (n >> 7) + 4`, both sides, at 64 literals (threshold 4) and at 1000 (11)
    for n, counts, kind in ((64, {97 + i: 4 for i in range(16)}, "raw"), (64, {97 + i: 4 for i in range(14)} | {111: 5, 112: 3}, "compressed"),
                            (1000, {60 + i: 10 + (i < 45) for i in range(95)} | {200: 5}, "raw"), (1000, {60 + i: 10 + (i < 32) for i in range(95)} | {200: 12, 201: 6}, "compressed")):
        assert sum(counts.values()) == n
        largest = max(counts.values())
        lits = _exact((n, largest), counts)
        add("literals/shortcut/%d-literals,largest-count=%d/%s" % (n, largest, kind), *_one(lits + lits[:40], n, {"literals.kind": kind, "literals.regenerated": n, "largest_count": largest}))
    # past the shortcut, a table is built and written, the streams are sized -- and the section does not gain: raw after all
    counts = {i: 4 for i in range(1, 248)} | {250: 12}
    lits = _exact("no-gain", counts)
    add("literals/gain-fallback/table-written-then-raw", *_one(lits + lits[:40], 1000, {"literals.kind": "raw", "literals.regenerated": 1000, "largest_count": 12}))
    # a tree deeper than 11: Fibonacci counts (every merge takes the two smallest) among letters that keep the 4-grams apart
    # (the limit is HuffmanCompressor's optimalNumberOfBits: highest_bit(n - 1) - 1 below 4097 literals, 11 from there on)
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    for name, counts, limit in (("fibonacci-15/limit-10", {65 + i: c for i, c in enumerate(fib[:15])} | {120 + i: 11 for i in range(110)}, 10),
                                ("fibonacci-15-two-tails/limit-10", {65 + i: c for i, c in enumerate(fib[:15])} | {90 + i: c for i, c in enumerate(fib[:12])} | {120 + i: 13 for i in range(110)}, 10),
                                ("fibonacci-17/limit-11", {65 + i: c for i, c in enumerate(fib)} | {90 + i: 60 for i in range(160)}, 11)):
        lits = _exact(name, counts)
        n = len(lits)
        add("literals/huffman/depth-limited/" + name, *_one(lits + lits[:40], n, {"literals.kind": "compressed", "literals.regenerated": n, "huffman_depth_over": limit, "max_bits": limit}))
    # setMaxHeight pays more than the cut cost (limit 10 at 2049 .. 4096 literals), literals chosen byte by byte.  First: one leaf of 11 bits, none of 9:
    # the step is taken from a leaf of 8 bits and pays 2 for a debt of 1; a bit goes back to the leaf behind the one just lengthened.  Second: code lengths
    # 1 .. 7 and a tail at 10 and 11, no leaf of 9 or 8 bits: the step from 7 bits pays 4 for 1, and the first bit goes back with no leaf of 9 bits to start from.
    for name, counts in (("one-over/a-leaf-of-rank-1-exists", (1030, 512, 256, 128, 64, 32, 16, 8, 2, 2, 2, 1, 1)),
                         ("three-over/no-leaf-of-rank-1", (1030, 516, 258, 130, 66, 34, 18, 2, 2, 2, 2, 2, 2, 2, 1, 1))):
        lits = [v for v, c in enumerate(counts) for _ in range(c)]
        n = len(lits)
        stride = next(k for k in range(n // 3, n) if np.gcd(k, n) == 1)
        z = _chosen_literals([lits[(i * stride) % n] for i in range(n)])
        add("literals/huffman/depth-limited/overpaid/" + name, z.done(), {"types": ["compressed", "compressed"], "exact": {1: z.want},
            "blocks": {1: {"literals.kind": "compressed", "literals.regenerated": n, "symbols": len(counts), "huffman_depth_over": 10, "max_bits": 10, "literals.weights.form": "direct"}}})
    # weights all equal: the bytes 0 .. 15 as often as each other (the table writer counts the weights of every symbol from 0 on), literals chosen byte by byte
    z = _chosen_literals([(i * 7) % 16 for i in range(256)])
    add("literals/huffman/weights-all-equal/direct", z.done(), {"types": ["compressed", "compressed"], "exact": {1: z.want},
                                                               "blocks": {1: {"literals.kind": "compressed", "weights_equal": True, "literals.weights.form": "direct", "symbols": 16, "max_bits": 4}}})
    lits = _stream("all-256", {i: (i + 1.0) ** -0.8 for i in range(256)}, n=9000, seed=4)
    add("literals/huffman/256-symbols", *_one(lits, 8000, {"literals.kind": "compressed", "symbols": 256, "literals.weights.form": "fse", "literals.weights.count": 255}))
    # two symbols; weights that are all different (no FSE table: direct) -- literals chosen byte by byte, in the second block
    z = _chosen_literals([0] * 45 + [1] * 19)  # (64 literals of two symbols: the table log comes out at its floor of 5)
    add("literals/huffman/two-symbols", z.done(), {"types": ["compressed", "compressed"], "exact": {1: z.want}, "blocks": {1: {"literals.kind": "compressed", "symbols": 2, "literals.regenerated": 64,
                                                                                                                       "literals.weights.form": "direct", "literals.streams": 1}}})
    lits = [v for v, c in enumerate((128, 64, 32, 16, 8, 4, 4)) for _ in range(c)]  # (code lengths 1 .. 6 and 6: no deeper than 256 literals allow)
    z = _chosen_literals([lits[(i * 37) % 256] for i in range(256)])
    add("literals/huffman/weights-all-different/direct", z.done(), {"types": ["compressed", "compressed"], "exact": {1: z.want},
                                                                    "blocks": {1: {"literals.kind": "compressed", "symbols": 7, "literals.weights.form": "direct", "literals.weights.weights": [6, 5, 4, 3, 2, 1], "literals.streams": 4}}})


def _window_cases(add):
    """Beyond 1 MiB the frame has a window descriptor and the match finder a window base (blockEnd - 2^20, set per block): 4096 bytes of filler early in the
    input, once more 20 000 bytes before the end -- with the first occurrence's first byte at the last block's window base (a candidate must lie beyond the
    base; the step backwards from the byte behind it reaches the base itself), and one byte before the base, where the match begins a byte later.  The rest is a period of 1000 bytes: a few long matches per block."""
    pool = ec._filler_pool()
    piece, period = pool[100000:104096], pool[200000:201000]
    n = (1 << 20) + 65536
    q = n - 20000
    base = n - (1 << 20)
    for name, p0, seq in (("at-the-window-base/matched", base, (0, q - base + 3, 4096)), ("one-before-the-window-base/not-matched", base - 1, (1, q - base + 1 + 3, 4095))):
        d = bytearray((period * (n // 1000 + 1))[:n])
        d[p0:p0 + 4096] = piece
        d[q:q + 4096] = piece
        add("frame/window/first-occurrence-%s" % name, d, {"frame": {"single_segment": False, "window_descriptor": 0x50, "window_log": 20, "content_size": n, "content_size_bytes": 4},
                                                         "nblocks": 9, "has": [[seq]], "offset": seq[1] - 3})


def _gain_and_table_cases(add):
    # compressBlock's gain test `compressedSize > n - (n >> 6) - 2`: raw literals and one match, a byte of match more or less
    for ll, ml, kind in ((100, 10, "raw"), (100, 11, "compressed"), (1000, 26, "raw"), (1000, 27, "compressed")):
        z = _try(lambda salt: S(salt).seq(ll, ll - 8, ml))
        n = ll + ml
        e = {"types": [kind]}
        if kind == "compressed":
            e.update({"exact": {0: z.want}, "blocks": {0: {"size": n - (n >> 6) - 2, "literals.kind": "raw"}}})  # (exactly the most a compressed block may take)
        add("blocks/gain/%d-literals,match-of-%d/%s" % (ll, ml, kind), z.done(), e)
    # no sequences: Huffman literals that gain (a table is built and written), a block that does not -- and four bytes of text more, where it just does
    pool = ec._filler_pool()
    for a, kind in ((324, "raw"), (328, "compressed")):
        e = {"types": [kind]}
        if kind == "compressed":
            e["blocks"] = {0: {"size": 1000 - (1000 >> 6) - 2, "literals.kind": "compressed", "nseq": 0}}
        add("blocks/gain/no-sequences,%d-of-1000-bytes-text/%s" % (a, "table-built-then-dropped" if kind == "raw" else kind), _t2()[:a] + pool[5000:5000 + 1000 - a], e)
    # FSE table descriptions: runs of zero counts of 1 .. 2, of 3 and more, of 24 and more (match-length codes 1 and 28 only)
    data, want = _try(_own, [(34, (6, 9, 14, 30, 14)[i % 5], (4, 31, 31)[i % 3]) for i in range(79)], first=(34, 14, 31))
    add("seq-tables/zero-run-of-24-and-more/ml-codes-1-and-28", data, {"exact": {0: want}, "blocks": {0: {"modes": ("rle", "fse", "fse"), "tables.ml.zero_runs": [(24, 99)], "tables.of.zero_runs": [(1, 2)]}}})
    data, want = _try(_own, [((12, 13, 20, 34)[i % 4], (6, 9, 11, 12)[i % 4], (8, 9, 15, 16)[i % 4]) for i in range(79)], first=(34, 14, 9))
    add("seq-tables/zero-runs-of-1-2-and-3-and-more", data, {"exact": {0: want}, "blocks": {0: {"modes": ("fse", "fse", "fse"), "tables.ml.zero_runs": [(3, 23)], "tables.ll.zero_runs": [(1, 2), (3, 23)]}}})
    # the last sequence's codes occur once: buildCompressionTable does not take one off their counts
    data, want = _try(_own, [((12, 13, 20, 34)[i % 4], (6, 9, 11, 12)[i % 4], (8, 9, 15, 16)[i % 4]) for i in range(78)] + [(70, 40, 60)], first=(34, 14, 9))
    add("seq-tables/last-codes-occur-once", data, {"exact": {0: want}, "blocks": {0: {"modes": ("fse", "fse", "fse")}}})
    # as many sequences as a block was made to hold: one literal and four bytes at the repeat offset, 26 213 times (the three-byte count begins at 32 512)
    z = _dict_block(False)
    for i in range((BLOCK - 7) // 5):  # (the finder stops eight bytes before the block's end)
        z.byte((z.d[len(z.d) - z.o1] + 1 + i % 3) & 255)
        z.pending += 1
        z.again(len(z.d) - z.o1, 4)
        z._close(1, 4)
    add("sequences/count=26213/the-most-in-one-block,last-block-of-5", z.done(7 + 5), {"types": ["compressed", "compressed", "raw"], "exact": {1: z.want}, "blocks": {1: {"nseq": 26213, "count_form": "two bytes", "modes": ("rle", "rle", "rle")}}})
