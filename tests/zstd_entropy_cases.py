"""Hand-built Zstd frames with real entropy coding, aimed at the decoder's entropy stages (zstd_dec_common.h: read_fse_table, fse_build, huf_read_table,
fse_decompress_weights, huf_decode_stream; zstd_decompress_pipe.hip: parse_block, the literal stage, the sequence stage, the zstd_mb_* stages; and the one-kernel
decoder zstd_decompress.hip).  The counterpart of tests/zstd_frame_cases.py, which aims at the execute stage.  Imports numpy and the standard library only.

Everything here is written from RFC 8878, not from the kernels and not from the oracle:
  * fse_description(): a normalized count vector (positive counts, -1, zeros) and a table log -> the bits of 4.1.1 (short and long values around the threshold,
    the two-bit zero-run repeats, padding to a byte);
  * fse_decode_table(): the decoding table of 4.1.1 by the serial spread walk; FseCoder turns it round: the one state of a symbol from which a given next state
    can be reached, which is all an encoder needs -- a stream is laid out from its LAST symbol, whose state is free to choose, back to its first;
  * sequences_stream(): three interleaved states plus extra bits (3.1.1.3.2.1), weights_stream(): two interleaved states (4.2.1.2);
  * huffman: a chosen weight vector (the last weight implied) -> canonical codes (4.2.1), the table description in both forms, one or four streams;
  * write_frame(): frames of raw, RLE and compressed blocks, each compressed block with its own literals kind and its own mode per sequence table.
The expected plaintext comes from executing the chosen sequences here, with the repeat offsets carried from block to block.  The writers record which states
of which table every stream visits.

entropy_catalog() returns the cases; the CPU suite (tests/test_zstd_entropy_cases.py) recounts the edges from the BYTES with the reader at the end of this
module, and compares every case with the oracle (the contract: the Java decoder) and with libzstd.  profiles/zstd_entropy_edges.md is the account of it."""
import numpy as np

from tests.zstd_frame_cases import LL_BASE, LL_BITS, ML_BASE, ML_BITS, MAX_BLOCK, Case, ll_code, ml_code, xxh64, read_frame_header, read_block_header, \
    read_literals_header, read_sequence_count
from tests import zstd_frame_cases as zc

LL, OF, ML = 0, 1, 2
TABLES = {}  # {table key: (kind or "W", norm, log)}: every described table a stream was coded with
KINDS = ("LL", "OF", "ML")
MAX_SYMBOL = (35, 28, 52)
MAX_LOG = (9, 8, 9)
# RFC 8878 3.1.1.3.2.2
PREDEFINED = (([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6),
              ([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1], 5),
              ([1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1], 6))
OF_USABLE = 18  # the largest offset code a frame of at most ~400 KiB of output can use


# ---------------------------------------------------------------- bits ----------------------------------------------------------------
def backward_stream(fields, pad_bits=0):
    """fields [(value, width)] in the order the decoder READS them -> the bytes of a backward bit stream (the first field right under the end mark)"""
    s = "1" + "".join(format(v, "0%db" % w) for v, w in fields if w)
    assert all(0 <= v < (1 << w) for v, w in fields if w) and all(v == 0 for v, w in fields if not w)
    s += "0" * pad_bits  # (never in a valid stream: bits in front of the first byte's)
    n = (len(s) + 7) // 8
    return int(s, 2).to_bytes(n, "little")


class ForwardBits:
    def __init__(self):
        self.acc = self.n = 0

    def put(self, v, w):
        assert 0 <= v < (1 << w), (v, w)
        self.acc |= v << self.n
        self.n += w

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


# ---------------------------------------------------------------- FSE ----------------------------------------------------------------
def fse_description(norm, log, runs=None):
    """the table description of 4.1.1 for the counts `norm` (symbol 0 first; the last one given is the last one written).  Returns (bytes, record): record
    lists what the writer did -- ("short" | "long-low" | "long-high", value), ("run", extra zeros) -- for its own cross-check with the reader below."""
    w = ForwardBits()
    w.put(log - 5, 4)
    remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
    rec = []
    i = 0
    while i < len(norm):
        assert remaining > 1 or runs is not None, "counts behind the one that completes the table"
        c = norm[i]
        v = c + 1
        mx = 2 * threshold - 1 - remaining
        if v < mx:
            w.put(v, nbits - 1)
            rec.append(("short", v))
        elif v < threshold:
            w.put(v, nbits)
            rec.append(("long-low", v))
        else:
            w.put(v + mx, nbits)
            rec.append(("long-high", v))
        remaining -= abs(c)
        i += 1
        halvings = 0
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
            halvings += 1
        rec.append(("halvings", halvings))
        if c == 0:
            extra = 0
            while i + extra < len(norm) and norm[i + extra] == 0:
                extra += 1
            if runs is not None:  # (a malformed run: more zeros announced than symbols given)
                extra = runs.pop(0)
            rec.append(("run", extra))
            i += extra
            while extra >= 3:
                w.put(3, 2)
                extra -= 3
            w.put(extra, 2)
    rec.append(("remaining", remaining))
    return w.bytes(), rec


def fse_decode_table(norm, log):
    """[(symbol, number of bits, baseline)] per state: the spread walk and the state numbering of 4.1.1, serially"""
    size = 1 << log
    sym = [None] * size
    high = size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
    pos, step, mask = 0, (size >> 1) + (size >> 3) + 3, size - 1
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & mask
            while pos > high:
                pos = (pos + step) & mask
    assert pos == 0 and None not in sym
    nxt = [1 if c == -1 else c for c in norm]
    table = []
    for u in range(size):
        s = sym[u]
        ns = nxt[s]
        nxt[s] += 1
        nb = log - (ns.bit_length() - 1)
        table.append((s, nb, (ns << nb) - size))
    return table


class FseCoder:
    """a decoding table turned round.  pred(symbol, next) -> (state, value, width): the state of `symbol` whose baseline range holds `next`"""

    def __init__(self, table, log, key):
        self.table, self.log, self.key = table, log, key  # key: what the visited-state records are filed under
        self.by_symbol = {}
        for u, (s, nb, base) in enumerate(table):
            self.by_symbol.setdefault(s, []).append(u)
        self.owner = {}
        for s, states in self.by_symbol.items():
            row = [None] * len(table)
            for u in states:
                _, nb, base = table[u]
                for y in range(base, base + (1 << nb)):
                    assert row[y] is None
                    row[y] = u
            assert len(table) == 1 or None not in row
            self.owner[s] = row

    def pred(self, symbol, nxt):
        u = self.owner[symbol][nxt]
        _, nb, base = self.table[u]
        return u, nxt - base, nb

    def chain(self, symbols, final=None):
        """the states of `symbols` (decode order) ending in state `final` (default: the symbol's first), and the update fields between them"""
        n = len(symbols)
        final = self.by_symbol[symbols[-1]][0] if final is None else final
        assert self.table[final][0] == symbols[-1]
        states = [None] * n
        upd = [None] * n
        states[-1] = final
        for i in range(n - 2, -1, -1):
            states[i], v, nb = self.pred(symbols[i], states[i + 1])
            upd[i] = (v, nb)
        return states, upd


def rle_coder(symbol, key):
    return FseCoder([(symbol, 0, 0)], 0, key)


def sequences_stream(seqs, coders, finals=(None, None, None), visited=None):
    """the bit stream of 3.1.1.3.2.1 for seqs [(ll, ml, offset value)]: offset value 1 .. 3 the repeat offsets, above that offset + 3"""
    codes = [[ll_code(s[0]) for s in seqs], [s[2].bit_length() - 1 for s in seqs], [ml_code(s[1]) for s in seqs]]
    st, up = zip(*(coders[k].chain(codes[k], finals[k]) for k in range(3)))
    if visited is not None:
        for k in range(3):
            visited.setdefault(coders[k].key, set()).update(st[k])
    fields = [(st[k][0], coders[k].log) for k in (LL, OF, ML)]
    for i, (ll, ml, ov) in enumerate(seqs):
        cl, co, cm = codes[LL][i], codes[OF][i], codes[ML][i]
        fields += [(ov - (1 << co), co), (ml - ML_BASE[cm], ML_BITS[cm]), (ll - LL_BASE[cl], LL_BITS[cl])]
        if i < len(seqs) - 1:
            fields += [up[LL][i], up[ML][i], up[OF][i]]
    return fields


def weights_stream(weights, coder, finals=(None, None), visited=None):
    """4.2.1.2: two interleaved states, the even weights from the first, the odd ones from the second; the stream ends with both states' last symbols"""
    assert len(weights) >= 2
    a, b = weights[0::2], weights[1::2]
    sa, ua = coder.chain(a, finals[0])
    sb, ub = coder.chain(b, finals[1])
    if visited is not None:
        visited.setdefault(coder.key, set()).update(sa + sb)
    fields = [(sa[0], coder.log), (sb[0], coder.log)]
    for i in range(len(weights) - 2):
        fields.append((ua if i % 2 == 0 else ub)[i // 2])
    return fields


# ---------------------------------------------------------------- Huffman ----------------------------------------------------------------
def huffman_last_weight(weights):
    """(table log, the implied last weight) for the weights given, or None where 4.2.1 has none"""
    total = sum((1 << w) >> 1 for w in weights)
    if total == 0:
        return None
    log = total.bit_length()
    rest = (1 << log) - total
    if rest & (rest - 1):
        return None
    return log, rest.bit_length()


def huffman_codes(full):
    """{symbol: (code, bits)} for the full weight vector: weight 1 symbols first, in symbol order, then weight 2, ... (4.2.1)"""
    total = sum((1 << w) >> 1 for w in full)
    log = total.bit_length() - 1
    assert 1 << log == total
    codes = {}
    pos = 0
    for w in range(1, log + 1):
        for s, x in enumerate(full):
            if x == w:
                codes[s] = (pos >> (w - 1), log + 1 - w)
                pos += 1 << (w - 1)
    assert pos == total
    return codes, log


def huffman_stream(data, codes):
    return backward_stream([codes[b] for b in data])


class Huf:
    """a Huffman literals section: weights (without the implied last one), how the table is described -- "direct", or ("fse", norm, log) with the weights' own FSE
    table --, 1 or 4 streams, the size format (None: the smallest)"""

    def __init__(self, data, weights=None, desc="direct", streams=1, form=None, treeless=False, tamper=None, w_finals=(None, None)):
        self.data, self.weights, self.desc, self.streams, self.form, self.treeless, self.tamper, self.w_finals = bytes(data), weights, desc, streams, form, treeless, tamper, w_finals


def write_huffman_table(h, visited, key):
    if h.desc == "direct":
        n = len(h.weights)
        ws = list(h.weights) + [0]
        return bytes([127 + n]) + bytes((ws[i] << 4) | ws[i + 1] for i in range(0, n, 2))
    _, norm, log = h.desc
    body, _ = fse_description(norm, log)
    TABLES[key] = ("W", list(norm), log)
    body += backward_stream(weights_stream(h.weights, FseCoder(fse_decode_table(norm, log), log, key), h.w_finals, visited))
    assert len(body) < 128, len(body)
    return bytes([len(body)]) + body


def write_literals(lit, state, visited, key):
    """the literals section for `lit`: bytes -> raw; ("rle", byte, n); Huf.  state: the frame's writer state (the Huffman codes in force)"""
    if isinstance(lit, (bytes, bytearray)) or (isinstance(lit, tuple) and lit[0] in ("raw", "rle")):
        if isinstance(lit, tuple):
            kind, data, form = (0, lit[1], lit[2]) if lit[0] == "raw" else (1, bytes([lit[1]]) * lit[2], lit[3] if len(lit) > 3 else None)
        else:
            kind, data, form = 0, bytes(lit), None
        n = len(data)
        if form is None:
            form = 0 if n < 32 else (1 if n < 4096 else 3)
        head = bytes([(n << 3) | (form << 2) | kind]) if form in (0, 2) else ((n << 4) | (form << 2) | kind).to_bytes(2 if form == 1 else 3, "little")
        return head + (data if kind == 0 else data[:1]), data
    h = lit
    table = b""
    if not h.treeless:
        lw = huffman_last_weight(h.weights)
        table = write_huffman_table(h, visited, key)
        if lw is not None and lw[1] <= 12 and lw[0] <= 12:
            state["huf"] = huffman_codes(list(h.weights) + [lw[1]])[0]
        else:
            state["huf"] = None  # (a table no decoder takes: the streams are whatever fits)
    codes = state.get("huf") or {b: (0, 1) for b in range(256)}
    n = len(h.data)
    if h.streams == 1:
        streams = huffman_stream(h.data, codes)
    else:
        seg = (n + 3) // 4
        parts = [huffman_stream(h.data[i * seg:(i + 1) * seg], codes) for i in range(3)] + [huffman_stream(h.data[3 * seg:], codes)]
        jump = [len(p) for p in parts[:3]]
        if h.tamper and "jump" in h.tamper:
            jump = h.tamper["jump"](jump)
        streams = b"".join(j.to_bytes(2, "little") for j in jump) + b"".join(parts)
    if h.tamper and "streams" in h.tamper:
        streams = h.tamper["streams"](streams)
    if h.tamper and "table" in h.tamper:
        table = h.tamper["table"](table)
    comp = len(table) + len(streams)
    regen = n + (h.tamper.get("regen", 0) if h.tamper else 0)
    form = h.form
    if form is None:
        form = (0 if h.streams == 1 else 1) if max(regen, comp) < 1024 else (2 if max(regen, comp) < 16384 else 3)
    assert (form == 0) == (h.streams == 1), "one stream has one size format"
    bits = 10 if form < 2 else (14 if form == 2 else 18)
    assert regen < (1 << bits) and comp < (1 << bits)
    head = ((3 if h.treeless else 2) | (form << 2) | (regen << 4) | (comp << (4 + bits))).to_bytes(3 if form < 2 else form + 2, "little")
    return head + table + streams, h.data[:regen]


# ---------------------------------------------------------------- blocks and frames ----------------------------------------------------------------
class Tab:
    """a sequence table's mode: Tab("predefined"), Tab("rle"), Tab("fse", norm, log), Tab("repeat"); raw: description bytes written as they are"""

    def __init__(self, mode, norm=None, log=None, raw=None, key=None):
        self.mode, self.norm, self.log, self.raw, self.key = mode, norm, log, raw, key


def execute_block(out, rep, literals, seqs):
    """appends the block's plaintext to `out` (the frame's output so far), updating rep; False where a sequence is malformed.  3.1.1.4, 3.1.1.5"""
    lp = 0
    for ll, ml, ov in seqs:
        if lp + ll > len(literals):
            return False
        out += literals[lp:lp + ll]
        lp += ll
        if ov > 3:
            o = ov - 3
            rep[:] = [o, rep[0], rep[1]]
        else:
            idx = ov - 1 + (1 if ll == 0 else 0)
            if idx == 0:
                o = rep[0]
            else:
                o = rep[0] - 1 if idx == 3 else rep[idx]
                if o == 0:
                    return False  # (3.1.1.5: a value of 0 is corrupt; the Java decoder takes 1 -- such a sequence is not written here)
                if idx != 1:
                    rep[2] = rep[1]
                rep[1] = rep[0]
                rep[0] = o
        if o > len(out):
            return False
        for _ in range(0, ml, o) if o < ml else (0,):
            take = min(o, ml - _)
            out += out[len(out) - o:len(out) - o + take]
    out += literals[lp:]
    return True


def write_block(spec, state, visited, name):
    """spec: ("raw", bytes) | ("rle", byte, n) | ("c", literals, seqs, (Tab, Tab, Tab), options).  Returns (kind, body, announced size); executes it into state["out"]"""
    if spec[0] == "raw":
        state["out"] += spec[1]
        return 0, spec[1], len(spec[1])
    if spec[0] == "rle":
        state["out"] += bytes([spec[1]]) * spec[2]
        return 1, bytes([spec[1]]), spec[2]
    _, lit, seqs, tabs, opt = (spec + ({},))[:5]
    body, literals = write_literals(lit, state, visited, name + "/W")
    ns = len(seqs)
    form = opt.get("count_form", 0 if ns < 128 else (1 if ns < 0x7F00 else 2))
    body += bytes([ns]) if form == 0 else (bytes([128 + (ns >> 8), ns & 255]) if form == 1 else b"\xff" + (ns - 0x7F00).to_bytes(2, "little"))
    if ns or form:
        modes = 0
        descs = b""
        coders = [None] * 3
        for k, t in enumerate(tabs):
            mode = ("predefined", "rle", "fse", "repeat").index(t.mode)
            modes |= mode << (6 - 2 * k)
            key = t.key or "%s/%s" % (name, KINDS[k])
            if t.mode == "predefined":
                coders[k] = FseCoder(fse_decode_table(*PREDEFINED[k]), PREDEFINED[k][1], "predefined/" + KINDS[k])
            elif t.mode == "rle":
                sym = t.norm if t.norm is not None else ((ll_code, lambda v: v.bit_length() - 1, ml_code)[k]((seqs[0][0], seqs[0][2], seqs[0][1])[k]) if ns else 0)
                descs += bytes([sym])
                coders[k] = rle_coder(sym, key)
            elif t.mode == "fse":
                if t.raw is not None:
                    descs += t.raw
                else:
                    descs += fse_description(t.norm, t.log)[0]
                coders[k] = FseCoder(fse_decode_table(t.norm, t.log), t.log, key) if t.norm is not None and t.log <= MAX_LOG[k] + 3 else None
                if t.norm is not None and t.raw is None:
                    TABLES[key] = (k, list(t.norm), t.log)
            else:
                coders[k] = state["fse"][k]
            if coders[k] is None:  # (malformed on purpose: nothing to code with; the stream is a stand-in)
                coders[k] = rle_coder(0, key)
                opt = dict(opt, stream=b"\x01")
        state["fse"] = list(coders)
        body += bytes([modes]) + descs
        if "stream" in opt:
            body += opt["stream"]
        elif ns:
            body += backward_stream(sequences_stream(seqs, coders, opt.get("finals", (None, None, None)), visited), opt.get("pad_bits", 0))
        else:
            body += b"\x01"
    if opt.get("cut"):
        body = body[:-opt["cut"]]
    body += opt.get("append", b"")
    state["ok"] = execute_block(state["out"], state["rep"], literals, seqs) and state["ok"]
    return 2, body, len(body)


def write_frame(blocks, *, checksum=False, single_segment=True, window_log=None, fcs_bytes=None, visited=None, name="", block_within_window=True):
    """(frame, plaintext or None where a sequence is malformed).  single_segment: the content size stands for the window; otherwise a window descriptor of
    window_log (default: enough for the plaintext) and a content size only where fcs_bytes says so.  A block may not be larger than the window (3.1.1.2.3:
    Block_Maximum_Size); a single-segment frame whose content is smaller than one of its blocks is written with a window descriptor instead, unless
    block_within_window is False (libzstd refuses such a frame, the Java decoder reads it)"""
    state = {"out": bytearray(), "rep": [1, 4, 8], "ok": True, "fse": [None] * 3, "huf": None}
    body = b""
    largest = 0
    for i, spec in enumerate(blocks):
        kind, data, size = write_block(spec, state, visited, "%s#%d" % (name, i))
        assert size < (1 << 21) and len(data) <= MAX_BLOCK, (name, len(data))
        body += ((size << 3) | (kind << 1) | (1 if i == len(blocks) - 1 else 0)).to_bytes(3, "little") + data
        largest = max(largest, len(data))
    plain = bytes(state["out"])
    n = len(plain)
    if single_segment and block_within_window and largest > n:
        single_segment = False
    if single_segment:
        nb = fcs_bytes or (1 if n < 256 else (2 if n < 65536 + 256 else 4))
        flag = {1: 0, 2: 1, 4: 2, 8: 3}[nb]
        head = bytes([0x20 | (flag << 6) | (4 if checksum else 0)]) + (n - 256 if nb == 2 else n).to_bytes(nb, "little")
    else:
        wl = window_log or max(10, (max(n, 1) - 1).bit_length())
        flag = {None: 0, 0: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
        head = bytes([(flag << 6) | (4 if checksum else 0), (wl - 10) << 3]) + ((n - 256 if fcs_bytes == 2 else n).to_bytes(fcs_bytes, "little") if fcs_bytes else b"")
    frame = b"\x28\xb5\x2f\xfd" + head + body
    if checksum:
        frame += (xxh64(plain) & 0xFFFFFFFF).to_bytes(4, "little")
    return frame, (plain if state["ok"] else None)


# ---------------------------------------------------------------- the catalog ----------------------------------------------------------------
class ECase(Case):
    """a catalog entry (tests/zstd_frame_cases.Case) with: fallback -- a valid frame the pipeline hands to the one-kernel decoder by design, and why;
    visited -- {table key: states} of every table its streams ran through; group -- the table group it counts for; differs -- a note where the RFC model and the
    Java decoder part (the expectation is the Java decoder's: see profiles/zstd_entropy_edges.md)"""

    def __init__(self, name, frame, plain, malformed=False, tags=(), fallback=None, visited=None, group=None, differs=None, cap=None):
        cap = cap if cap is not None else (len(plain) if plain is not None else 4096)
        super().__init__(name, frame, plain, cap, 0, malformed=malformed, tags=tags, checksum=bool(frame[4] & 4))
        self.fallback, self.visited, self.group, self.differs = fallback, visited or {}, group, differs
        self.model_plain = plain  # what the Python model decodes the frame to (add() keeps it for the cases the Java decoder refuses)


def history_blocks(rng, n, period=251):
    """blocks that lay down n bytes of history with period `period`: a raw block of random bytes, then matches at offset `period` (RLE tables: no entropy coding)"""
    seed = rng.integers(0, 256, period, dtype=np.uint8).tobytes()
    blocks = [("raw", seed)]
    left = n - period
    while left > 0:
        take = []
        room = 120000
        while left > 0 and room > 0 and len(take) < 2:
            ml = max(min(left, 60000, room), 3)
            take.append((0, ml, period + 3))
            left -= ml
            room -= ml
        # (the sequences of a block share their codes: one block per match-length code)
        for s in take:
            blocks.append(("c", b"", [s], (Tab("rle"), Tab("rle"), Tab("rle"))))
    return blocks


def usable(kind, symbol):
    return symbol <= OF_USABLE if kind == OF else True


def symbol_cost(kind, s):
    return LL_BASE[s] if kind == LL else (ML_BASE[s] if kind == ML else 0)


def cover_walks(rng, coder, kind, visited, budget=100000, max_len=1500, max_walks=60, extra_steps=40):
    """symbol lists (decode order, each with its final state) whose chains visit every state of `coder` whose symbol a frame here can use; greedy, backwards"""
    walks = []
    want = {u for u, (s, _, _) in enumerate(coder.table) if usable(kind, s)}
    seen = set(visited)
    while want - seen and len(walks) < max_walks:
        left = budget
        final = min(want - seen, key=lambda u: (-symbol_cost(kind, coder.table[u][0]), u))  # (the dearest first: it has the block's whole budget)
        syms = [coder.table[final][0]]
        left -= symbol_cost(kind, syms[0])
        seen.add(final)
        y = final
        idle = 0
        while len(syms) < max_len:
            cands = [(s,) + coder.pred(s, y) for s in coder.by_symbol if usable(kind, s) and symbol_cost(kind, s) <= left]
            fresh = [c for c in cands if c[1] not in seen]
            if not cands or (not fresh and idle >= extra_steps):
                break
            idle = 0 if fresh else idle + 1
            if not fresh:  # look one step further: a visited state from which a fresh one can be reached
                ahead = [c for c in cands if any(coder.pred(s2, c[1])[0] not in seen for s2 in coder.by_symbol if usable(kind, s2) and symbol_cost(kind, s2) <= left - symbol_cost(kind, c[0]))]
                cands = ahead or cands
            pool = fresh or cands
            c = pool[int(rng.integers(0, len(pool)))]
            syms.append(c[0])
            left -= symbol_cost(kind, c[0])
            seen.add(c[1])
            y = c[1]
        walks.append((syms[::-1], final))
    return walks


def seqs_for(rng, kind, syms, history, extra="random"):
    """sequences whose `kind` codes are `syms`; the other two fields small and fixed-code (their tables are RLE or predefined): ll 1 / ml 4 / a small offset.
    history: bytes of output in front of the block"""
    seqs = []
    out = history
    for s in syms:
        pick = (lambda bits: int(rng.integers(0, 1 << bits)) if extra == "random" and bits else 0)
        ll, ml, ov = 1, 4, 5
        if kind == LL:
            ll = LL_BASE[s] + (pick(LL_BITS[s]) if LL_BITS[s] < 6 else 0)
        elif kind == ML:
            ml = ML_BASE[s] + (pick(ML_BITS[s]) if ML_BITS[s] < 7 else 0)
        else:
            lo, hi = 1 << s, min((2 << s) - 1, out + ll + 3)
            assert lo <= hi or s < 2, (s, out)
            ov = int(rng.integers(lo, hi + 1)) if s >= 2 else (1 if s == 0 else int(rng.integers(2, 4)))
        seqs.append((ll, ml, ov))
        out += ll + ml
    return seqs


_catalog = None


def entropy_catalog():
    global _catalog
    if _catalog is None:
        _catalog = _build_catalog()
    return _catalog


def _norm_sum_ok(norm, log):
    return sum(abs(c) for c in norm) == 1 << log


def random_norm(rng, kind, log=None, nsym=None):
    """a random valid count vector: random support, some -1, zero runs, the rest spread"""
    top = MAX_SYMBOL[kind] + 1
    log = log or int(rng.integers(5, MAX_LOG[kind] + 1))
    size = 1 << log
    n = nsym or int(rng.integers(2, top + 1))
    present = np.sort(rng.choice(n, int(rng.integers(2, min(n, size) + 1)), replace=False))
    if n - 1 not in present:
        present = np.append(present[:-1], n - 1)
    norm = [0] * n
    for s in present:
        norm[s] = -1 if rng.random() < 0.3 else 1
    left = size - len(present)
    hot = [int(s) for s in present if norm[s] == 1]
    if not hot:
        norm[int(present[0])] = 1
        hot = [int(present[0])]
    cuts = np.sort(rng.integers(0, left + 1, len(hot) - 1)) if len(hot) > 1 else np.array([], dtype=int)
    parts = np.diff(np.concatenate(([0], cuts, [left])))
    if rng.random() < 0.4:  # (one symbol takes nearly everything)
        parts = np.zeros(len(hot), dtype=int)
        parts[int(rng.integers(0, len(hot)))] = left
    for s, p in zip(hot, parts):
        norm[s] += int(p)
    assert _norm_sum_ok(norm, log)
    return norm, log


def named_tables():
    """{kind: [(name, norm, log, tags)]}: the table descriptions the issue names.  Symbols a small frame cannot use often (LL >= 25, ML >= 43) get -1 or small counts;
    offset codes above OF_USABLE stay out of the tables whose every state must be visited and come in the tables marked "unusable" """
    T = {LL: [], OF: [], ML: []}

    def fill(n, log, spec, default=0):
        norm = [default] * n
        for s, c in spec.items():
            norm[s] = c
        return norm

    for kind in (LL, OF, ML):
        nmax = MAX_SYMBOL[kind] + 1
        nuse = min(nmax, OF_USABLE + 1) if kind == OF else nmax
        mlog = MAX_LOG[kind]
        big = 1 << mlog
        # log 5, all 32 symbols "less than one" (OF: 19 usable symbols cannot fill 32 states with -1 alone -- its all--1 table has unusable symbols)
        if kind != OF:
            T[kind].append(("all-low-32", [-1] * 32, 5, {"log=5", "all-low", "size=32"}))
        else:
            T[kind].append(("all-low-29+3", [-1] * 28 + [4], 5, {"log=5", "all-low", "size=32", "unusable-symbols"}))
        # size - 1 states beside a single -1, beside a count of 1; at the maximum log (a symbol of 300+ states: 511 / 255)
        T[kind].append(("max-log-one-low", fill(2, mlog, {0: big - 1, 1: -1}), mlog, {"log=max", "one-low", "low-last", "size-1+low", "states>=128", "states>=65"} | ({"states>=300"} if kind != OF else set())))
        T[kind].append(("max-log-beside-1", fill(3, mlog, {0: 1, 2: big - 1}), mlog, {"log=max", "size-1+one", "run=0", "long-high"}))
        T[kind].append(("low-first", fill(4, 6, {0: -1, 1: 30, 2: 3, 3: 30}), 6, {"low-first", "size=64", "log=6"}))
        # -1s interleaved with large counts; 65 and 128 states
        T[kind].append(("interleaved", fill(9, 8, {0: 65, 1: -1, 2: 128, 3: -1, 4: 40, 5: -1, 6: 10, 7: -1, 8: 9}), 8, {"interleaved-low", "states>=65", "states>=128", "low-last"}))
        # zero runs (extra zeros behind the first): 1, 2, 3, 4, 6, 7 and a run up to the last symbol
        for part, run_set in enumerate(((1, 2, 3),) if kind == OF else (((1, 2, 3, 4), (6, 7)) if kind == LL else ((1, 2, 3, 4, 6, 7),))):
            norm = [0] * nuse
            at = 0
            for extra in run_set:
                norm[at] = 3
                at += 1 + 1 + extra  # a count, a zero, `extra` more zeros
            norm[at] = 2
            assert at < nuse - 2
            norm[nuse - 1] = -1  # (... and zeros from at + 1 to the one before the last symbol)
            norm[0] += 64 - sum(abs(c) for c in norm)
            T[kind].append(("zero-runs-%d" % part, norm, 6, {"run=%d" % r for r in run_set}))
        if kind == OF:
            norm = [0] * 19
            for s, c in {0: 20, 6: 3, 14: 3, 18: 6}.items():
                norm[s] = c
            T[kind].append(("zero-runs-b", norm, 5, {"run=4", "run=6"}))
            norm = [0] * 29
            for s, c in {0: 24, 9: 7, 28: 1}.items():
                norm[s] = c
            T[kind].append(("zero-runs-c", norm, 5, {"run=7", "run-to-max-symbol", "unusable-symbols"}))
        # long runs (the 0xFFFF path of the Java reader: 24 extra zeros and more)
        if kind == LL:
            T[kind].append(("run-24", fill(36, 5, {0: 16, 26: 15, 35: -1}), 5, {"run=24", "run-ffff", "run-to-max-symbol"}))
        if kind == ML:
            T[kind].append(("run-24", fill(28, 5, {1: 20, 27: 12}), 5, {"run=24", "run-ffff"}))
            T[kind].append(("run-27", fill(53, 6, {0: 30, 1: 10, 30: 23, 52: -1}), 6, {"run=27", "run-ffff", "run-to-max-symbol"}))
            T[kind].append(("run-48", fill(53, 7, {2: 127, 52: -1}), 7, {"run=48", "run-ffff", "run-to-max-symbol"}))
        # the threshold: short and long values, both sides of max, a count after which the threshold halves more than once
        T[kind].append(("threshold", fill(8, 7, {0: 100, 1: 1, 2: 13, 3: 1, 4: 6, 5: 2, 6: 4, 7: 1}), 7, {"halvings>=2", "short", "long-low", "long-high"}))
        T[kind].append(("exactly-one-low", fill(6, 5, {0: 10, 1: 10, 2: -1, 3: 5, 4: 3, 5: 3}), 5, {"one-low", "log=5"}))
        # every symbol of the alphabet present at the maximum log, the dear ones "less than one"
        dear = (lambda s: s >= 25) if kind == LL else ((lambda s: s >= 43) if kind == ML else (lambda s: s > OF_USABLE))
        norm = [-1 if dear(s) else 1 for s in range(nmax)]
        spare = big - sum(abs(c) for c in norm)
        cheap = [s for s in range(nmax) if not dear(s)]
        for j, s in enumerate(cheap):
            norm[s] += spare // len(cheap) + (1 if j < spare % len(cheap) else 0)
        T[kind].append(("full-alphabet", norm, mlog, {"log=max", "full-alphabet"} | ({"unusable-symbols"} if kind == OF else set())))
    return T


MALFORMED_TABLES = ("log-above-max", "run-past-max-symbol", "symbol-limit-remaining>1")


def _build_catalog():
    rng = np.random.default_rng(8878)
    cases = []

    def add(name, blocks, tags=(), malformed=False, fallback=None, group=None, frame_opts=None, cap=None, java_refuses=None, differs=None):
        visited = {}
        fo = dict(frame_opts or {})
        fo.setdefault("checksum", len(cases) % 2 == 1)
        frame, plain = write_frame(blocks, visited=visited, name=name, **fo)
        assert malformed or plain is not None, name
        if java_refuses:  # valid by RFC 8878, refused by the Java decoder: the contract is the Java decoder
            malformed, differs, tags = True, java_refuses, set(tags) | {"java-differs"}
        assert len(frame) <= 200000, (name, len(frame))
        c = ECase(name, frame, None if malformed else plain, malformed=malformed, tags=set(tags), fallback=fallback, visited=visited, group=group,
                  cap=cap if cap is not None else (len(plain) if plain is not None else 4096), differs=differs)
        c.model_plain = plain
        cases.append(c)
        return c

    def tabs_for(kind, tab, others="rle"):
        t = [Tab(others), Tab(others), Tab(others)]
        t[kind] = tab
        return tuple(t)

    # ---- 1. FSE table descriptions: one table at a time in compressed mode (the other two RLE, then predefined), every usable state visited ----
    HIST = 300000
    for kind, tables in named_tables().items():
        for tname, norm, log, tags in tables:
            assert _norm_sum_ok(norm, log), (KINDS[kind], tname)
            key = "%s/%s" % (KINDS[kind], tname)
            coder = FseCoder(fse_decode_table(norm, log), log, key)
            seen = set()
            walks = cover_walks(rng, coder, kind, seen, budget=110000 if kind != OF else 30000)
            tags = set(tags) | {"table=" + KINDS[kind], "desc-log=%d" % log}
            for j, (syms, final) in enumerate(walks):
                finals = [None] * 3
                finals[kind] = final
                heavy = sum(symbol_cost(kind, s) for s in syms) > 4000
                nlit = lambda seqs: sum(s[0] for s in seqs)
                # (a) a frame of several blocks: history in front (offset codes up to 18 need 2^18 bytes of it), the table described in the first compressed block
                need = min(HIST, (2 << max(syms)) + 1000) if kind == OF else 600
                hist = history_blocks(rng, need)
                seqs = seqs_for(rng, kind, syms, need)
                lit = ("rle", 0x41 + j % 26, nlit(seqs) + 3) if heavy else rng.integers(0, 256, nlit(seqs) + 3, dtype=np.uint8).tobytes()
                others = "rle" if j % 2 == 0 else "predefined"
                blk = ("c", lit, seqs, tabs_for(kind, Tab("fse", norm, log, key=key), others), {"finals": tuple(finals)})
                add("%s-%s-w%d-mb" % (KINDS[kind], tname, j), hist + [blk], tags=tags | {"others=" + others, "multi-block"}, group=key,
                        frame_opts={"single_segment": j % 3 != 0})
                # (b) the same block as a single-block frame (the pipeline's other instantiation), where it stands on its own: no history needed
                if kind != OF:
                    seqs1 = [(max(seqs[0][0], 2),) + seqs[0][1:]] + seqs[1:]
                    if ll_code(seqs1[0][0]) == ll_code(seqs[0][0]):
                        lit1 = ("rle", 0x61 + j % 26, nlit(seqs1) + 1) if heavy else rng.integers(0, 256, nlit(seqs1) + 1, dtype=np.uint8).tobytes()
                        blk1 = ("c", lit1, seqs1, tabs_for(kind, Tab("fse", norm, log, key=key), others), {"finals": tuple(finals)})
                        add("%s-%s-w%d-single" % (KINDS[kind], tname, j), [blk1], tags=tags | {"others=" + others, "single-block"}, group=key)

    # ---- 2. the random family: at least 40 valid count vectors per kind, one block each; all three tables compressed together ----
    for kind in (LL, OF, ML):
        for r in range(44):
            norm, log = random_norm(rng, kind, nsym=None if kind != OF or r % 4 else int(rng.integers(20, 30)))
            if kind == OF and not any(usable(OF, s) and c for s, c in enumerate(norm)):
                continue
            key = "random/%s/%d" % (KINDS[kind], r)
            coder = FseCoder(fse_decode_table(norm, log), log, key)
            walks = cover_walks(rng, coder, kind, set(), budget=20000, max_len=300, max_walks=2)
            need = min(HIST, (2 << max(max(sy) for sy, _ in walks)) + 1000) if kind == OF else 300
            blocks = history_blocks(rng, need)
            for j, (syms, final) in enumerate(walks):
                finals = [None] * 3
                finals[kind] = final
                seqs = seqs_for(rng, kind, syms, need)
                n = sum(s[0] for s in seqs) + 2
                lit = ("rle", 0x30 + r % 10, n) if n > 3000 else rng.integers(0, 256, n, dtype=np.uint8).tobytes()
                blocks.append(("c", lit, seqs, tabs_for(kind, Tab("fse", norm, log, key=key) if j == 0 else Tab("repeat"), "predefined" if r % 2 else "rle"), {"finals": tuple(finals)}))
            add("random-%s-%d" % (KINDS[kind], r), blocks, tags={"random-table", "table=" + KINDS[kind], "desc-log=%d" % log}, group="random/" + KINDS[kind],
                frame_opts={"single_segment": r % 2 == 0})
    for r in range(12):  # all three compressed together: triples drawn at random, each table's chain ending where it likes
        tabs = []
        norms = []
        for kind in (LL, OF, ML):
            norm, log = random_norm(rng, kind, nsym=int(rng.integers(8, 19)) if kind == OF else None)
            norms.append((norm, log))
            tabs.append(Tab("fse", norm, log, key="together/%d/%s" % (r, KINDS[kind])))
        syms = [[s for s, c in enumerate(n) if c and (k != LL or s < 25) and (k != ML or s < 43)] or [max(s for s, c in enumerate(n) if c)] for k, (n, _) in enumerate(norms)]
        seqs = []
        out = HIST
        for i in range(int(rng.integers(1, 120))):
            a, b, cc = (int(rng.choice(s)) for s in syms)
            ll = LL_BASE[a] + int(rng.integers(0, 1 << min(LL_BITS[a], 4)))
            ml = ML_BASE[cc] + int(rng.integers(0, 1 << min(ML_BITS[cc], 4)))
            ov = int(rng.integers(1 << b, 2 << b)) if b >= 2 else (1 if b == 0 else int(rng.integers(2, 4)))
            ov = 2 if (ll == 0 and ov == 3) else ov
            seqs.append((ll, ml, ov))
            out += ll + ml
            if out - HIST > 100000:
                break
        n = sum(s[0] for s in seqs) + 5
        lit = ("rle", 0x21 + r, n) if n > 3000 else rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        add("together-%d" % r, history_blocks(rng, HIST) + [("c", lit, seqs, tuple(tabs))], tags={"three-compressed"}, group="together", frame_opts={"single_segment": r % 2 == 1})

    # ---- 3. malformed table descriptions ----
    lit8 = b"literals"
    for kind in (LL, OF, ML):
        K = KINDS[kind]
        mlog = MAX_LOG[kind]
        # one above the maximum log: the description's first nibble
        norm = [(2 << mlog) - 1, -1]
        raw = fse_description(norm, mlog + 1)[0]
        add("bad-%s-log-above-max" % K, [("c", lit8, [(1, 4, 5)], tabs_for(kind, Tab("fse", norm, mlog + 1, raw=raw)), {"stream": b"\x01\x00\x00\x01"})], malformed=True,
            tags={"bad-table", "log-above-max", "table=" + K})
        # a zero run that passes the maximum symbol
        n = MAX_SYMBOL[kind] + 1
        norm = [31, 0]
        raw = fse_description(norm, 5, runs=[n])[0]
        add("bad-%s-run-past-max-symbol" % K, [("c", lit8, [(1, 4, 5)], tabs_for(kind, Tab("fse", None, 5, raw=raw + b"\x00\x00")), {"stream": b"\x01\x00\x00\x01"})], malformed=True,
            tags={"bad-table", "run-past-max-symbol", "table=" + K})
        # the symbol limit ends the table with counts still to come (remaining > 1)
        norm = [1] * n
        size_log = 6 if n > 32 else 5
        norm[0] = (1 << size_log) - n  # one state short of the table
        raw, rec = fse_description(norm, size_log)
        assert rec[-1] == ("remaining", 2)
        add("bad-%s-symbol-limit" % K, [("c", lit8, [(1, 4, 5)], tabs_for(kind, Tab("fse", None, size_log, raw=raw)), {"stream": b"\x01\x00\x00\x01"})], malformed=True,
            tags={"bad-table", "symbol-limit-remaining>1", "table=" + K})

    # ---- 4. description tails: the match-length table (the last one described) ends 0, 1, 2, 3 bytes before the block's end ----
    for tail in (0, 1, 2, 3):
        for tname, norm, log in (("two", [16, 16], 5), ("low", [20, -1, 0, 0, 5, -1, 5], 5), ("wide", [1] * 30 + [-1] * 2 + [0, 0, 0, 30, 2], 6)):
            coder = FseCoder(fse_decode_table(norm, log), log, "tail")
            # the shortest streams: `tail` bytes -- the match-length state's `log` bits, no extra bits (symbols below 32), the mark; longer ones are padded with
            # sequences of no extra bits
            syms = [s for s, c in enumerate(norm) if c]
            want_bits = 8 * tail - 1
            seqs = None
            if tail:
                for tries in range(400):
                    k = int(rng.integers(1, 5))
                    cand = [(2, ML_BASE[int(rng.choice(syms))], 5) for _ in range(k)]
                    fields = sequences_stream(cand, [rle_coder(2, "x"), rle_coder(2, "x"), coder])
                    nbits = sum(w for _, w in fields)
                    if want_bits - 7 <= nbits <= want_bits:
                        seqs = cand
                        break
                if seqs is None and tail == 1 and log > 5:
                    continue  # (six bits of state, two of offset and the mark do not fit a byte)
                assert seqs, (tail, tname)
                blk = ("c", b"abcdefgh", seqs, (Tab("rle"), Tab("rle"), Tab("fse", norm, log, key="tail/%s" % tname)))
                short = len(fse_description(norm, log)[0]) + tail < 4
                add("tail-%d-%s" % (tail, tname), [blk], tags={"tail=%d" % tail, "table=ML"}, group="tail/%s" % tname,
                    java_refuses="a table description with fewer than 4 bytes from its start to the block's end (FseTableReader.readFseTable)" if short else None)
            else:
                blk = ("c", b"abcdefgh", [(1, 3, 5)], (Tab("rle"), Tab("rle"), Tab("fse", norm, log)), {"stream": b""})
                add("tail-0-%s" % tname, [blk], malformed=True, tags={"tail=0", "table=ML"})

    # ---- 5. the sequence stream ----
    # extra bits plus three state updates beyond 64 bits: LL code 35 (16 bits), ML code 52 (16), OF code 17 (17) at logs 9 / 8 / 9, every state update full width
    nLL = [1] * 35 + [-1]
    nLL[0] = 512 - 35
    nOF = [1] * 17 + [-1]
    nOF[2] = 256 - 17
    nML = [1] * 52 + [-1]
    nML[1] = 512 - 52
    wide = (Tab("fse", nLL, 9, key="wide/LL"), Tab("fse", nOF, 8, key="wide/OF"), Tab("fse", nML, 9, key="wide/ML"))
    for llc, tag, note in ((35, "wide-sequence-ll35", "block-above-128KiB"), (34, "wide-sequence-ll34", None)):
        first = (LL_BASE[llc] + 77, ML_BASE[52] + 1 if llc == 34 else ML_BASE[52], (1 << 17) + 12345)
        n = first[0] + 2 + 1
        add(tag, history_blocks(rng, 200000) + [("c", ("rle", 0x5A, n), [first, (2, 3, 5), (1, 4, 4)], wide)], tags={"wide-sequence", tag} | ({note} if note else set()), group="wide",
            frame_opts={"single_segment": False, "window_log": 19})
    # runs of sequences without extra bits; counts 1, 2, 3; each count form
    pre3 = (Tab("predefined"), Tab("predefined"), Tab("predefined"))
    for n in (1, 2, 3, 127, 128, 300):
        seqs = [(1 + i % 15, 3 + i % 29, 1 if i % 3 else 4 + i % 4) for i in range(n)]
        seqs[0] = (4, 5, 5)
        lit = rng.integers(0, 256, sum(s[0] for s in seqs), dtype=np.uint8).tobytes()
        add("no-extra-bits-%d" % n, [("c", lit, seqs, pre3)], tags={"nseq=%d" % n, "no-extra-bits", "count-form=%d" % (1 if n < 128 else 2)}, group="predefined")
    seqs = [(1, 3, 4)] * (0x7F00 + 5)
    add("count-form-3", [("c", ("rle", 0x33, len(seqs)), seqs, pre3)], tags={"count-form=3"}, group="predefined")
    seqs = [(1, 3, 4)] * 20
    add("count-form-2-small", [("c", ("rle", 0x34, 20), seqs, pre3, {"count_form": 1})], tags={"count-form=2"}, group="predefined")
    # end marks: the stream's last byte 0x01 (eight bits of payload below the mark's byte), 0x80 (the first seven bits read are zero), 0x00 (malformed)
    found = set()
    pcoders = [FseCoder(fse_decode_table(*PREDEFINED[k]), PREDEFINED[k][1], "predefined/" + KINDS[k]) for k in range(3)]
    for fl in range(64):  # one sequence behind a raw block: its three states are free to choose
        for fo in range(32):
            for fm in range(0, 64, 7):
                cl, co, cm = pcoders[LL].table[fl][0], pcoders[OF].table[fo][0], pcoders[ML].table[fm][0]
                if cl > 20 or not 2 <= co <= 6 or cm > 40:
                    continue
                seq = (LL_BASE[cl], ML_BASE[cm], (1 << co) + (5 if co > 2 else 1))
                stream = backward_stream(sequences_stream([seq], pcoders, (fl, fo, fm)))
                if stream[-1] in (0x01, 0x80) and stream[-1] not in found:
                    found.add(stream[-1])
                    lit = rng.integers(0, 256, seq[0] + 1, dtype=np.uint8).tobytes()
                    add("seq-end-mark-%02x" % stream[-1], [("raw", rng.integers(0, 256, 100, dtype=np.uint8).tobytes()), ("c", lit, [seq], pre3, {"finals": (fl, fo, fm)})],
                        tags={"seq-end-mark=%02x" % stream[-1]}, group="predefined")
    assert len(found) == 2
    add("bad-seq-end-mark-00", [("c", b"abcd", [(1, 3, 4)], pre3, {"append": b"\x00"})], malformed=True, tags={"seq-end-mark=00"})

    # ---- 6. Huffman tables ----
    def data_for(full, n, every=True):
        syms = [s for s, w in enumerate(full) if w]
        p = np.array([float(1 << full[s]) for s in syms])
        d = rng.choice(syms, n, p=p / p.sum()).astype(np.uint8)
        if every and n >= len(syms):
            d[rng.choice(n, len(syms), replace=False)] = syms
        return d.tobytes()

    def huf_block(h, extra_seqs=True):
        # the literals, and behind them two sequences that copy from them (predefined tables)
        n = len(h.data)
        seqs = [(min(n, 3), 4, 4 + min(n, 3) - 1)] if n >= 1 and extra_seqs else []
        return ("c", h, seqs, pre3)

    def full_of(weights):
        lw = huffman_last_weight(weights)
        return list(weights) + [lw[1]], lw[0]

    def chain_weights(L):  # 1, 1, 2, 3, ... L: the last one (L) implied -- the maximally skewed code of log L
        return [1, 1] + list(range(2, L)) if L > 1 else [1]

    def add_huf(name, weights, n, tags, desc="direct", streams=1, fallback=None, malformed=False, data=None, group=None, frame_opts=None, java_refuses=None, differs=None, **kw):
        lw = huffman_last_weight(weights)
        if data is None:
            full = (list(weights) + [lw[1]]) if lw else [1] * 256
            data = data_for(full, n)
        h = Huf(data, weights, desc=desc, streams=streams, **kw)
        t = set(tags) | {"huf"}
        if lw and not malformed:
            t |= {"huf-log=%d" % lw[0], "huf-weights=%d" % len(weights), "huf-desc=" + (desc if desc == "direct" else "fse"), "huf-streams=%d" % streams}
        return add(name, [huf_block(h)], tags=t, malformed=malformed, fallback=fallback, group=group, frame_opts=frame_opts, java_refuses=java_refuses, differs=differs)

    def skew_for(n_weights, zeros=()):
        """n_weights weights with every symbol present (but those in `zeros`): weight 1 and 2 interleaved so that the implied last weight is 1"""
        n = n_weights + 1 - len(zeros)
        L = max((n - 1).bit_length(), 1)
        b, a = (1 << L) - n, 2 * n - (1 << L)
        assert a >= 2 and b >= 0
        ws = []
        twos = b
        live = [s for s in range(n_weights + 1) if s not in zeros]
        for j, s in enumerate(live[:-1]):
            if twos and j % 2 == 0:
                ws.append((s, 2))
                twos -= 1
            else:
                ws.append((s, 1))
        if twos:  # (more twos than every second place: from the front)
            for j, (s, w) in enumerate(ws):
                if w == 1 and twos:
                    ws[j] = (s, 2)
                    twos -= 1
        full = [0] * n_weights
        for s, w in ws:
            full[s] = w
        return full

    # direct form: 1, 2, 127, 128 weights; odd and even counts
    add_huf("huf-direct-1", [1], 40, {"huf-direct-odd", "huf-all-equal", "last-weight=1"})
    add_huf("huf-direct-2", [1, 1], 40, {"huf-direct-even", "last-weight=log"})
    add_huf("huf-direct-127", skew_for(127), 600, {"huf-direct-odd", ">64-of-one-weight"}, streams=4)
    add_huf("huf-direct-128", skew_for(128), 700, {"huf-direct-even", ">64-of-one-weight"}, streams=4)
    # table logs 1 .. 12 by the maximally skewed chain 1, 1, 2, 3, ...; log 12 is the one-kernel decoder's
    for L in range(1, 13):
        w = chain_weights(L)
        add_huf("huf-log-%d" % L, w, 300 + 50 * L, {"huf-chain", "last-weight=log"}, streams=1 if L % 2 else 4, fallback="huffman log 12" if L == 12 else None)
    add_huf("huf-log-11-max-codes", chain_weights(11), 0, {"huf-max-length-run"}, data=bytes([0, 1] * 40 + [11, 0, 0, 0, 1, 1, 1]))
    # zeros between used symbols; the last weight 1; all equal over more than 64 symbols
    zs = [0] * 200
    for s, w in {3: 3, 70: 1, 71: 1, 130: 2, 199: 3}.items():
        zs[s] = w
    add_huf("huf-zeros-between", zs[:200], 500, {"huf-zero-weights"}, desc=("fse", [40, 6, 6, 12], 6), group="W/zeros")
    # FSE-compressed weights: 65, 129, 193, 254, 255 weights with every byte value present; the weights' table at log 5 and log 6
    for nw, wl in ((65, 5), (129, 6), (193, 5), (252, 6), (253, 5), (254, 6), (255, 5)):
        w = skew_for(nw)
        ones, twos = w.count(1), w.count(2)
        size = 1 << wl
        c2 = max(1, min(size - 2, round(size * twos / (ones + twos)))) if twos else 0
        norm = [0, size - c2, c2] if c2 else [0, size - 1, -1]
        if not twos:
            norm = [-1, size - 1]
        add_huf("huf-fse-%d" % nw, w, 1200, {"huf-fse-weights=%d" % nw, "weights-log=%d" % wl, "weights-mod4=%d" % (nw % 4), ">64-of-one-weight", "every-byte" if nw == 255 else "huf-wide",
                                             "huf-all-equal" if not twos else "huf-mixed"},
                desc=("fse", norm, wl), streams=4, group="W/%d" % nw)
    # ... and short weight streams that leave the four-at-a-time loop with each remainder
    for nw in (4, 5, 6, 7, 9, 14, 19, 32):
        w = skew_for(nw)
        add_huf("huf-fse-short-%d" % nw, w, 100, {"weights-mod4=%d" % (nw % 4), "weights-log=5"}, desc=("fse", [0, 16, 16] if w.count(2) else [-1, 31], 5), group="W/short",
                java_refuses="fewer than six FSE-compressed weights: FiniteStateEntropy.decompress emits four symbols before it looks at the stream's end" if nw < 6 else None)
    # a weights table with every weight 0 .. 11 in it, every state visited: the chain of log 11 in FSE form, repeated symbols
    wnorm = [6, 20, 4, 4, 4, 4, 4, 4, 4, 4, 3, 3]
    w = [1, 1, 2, 3, 0, 4, 0, 0, 5, 6, 7, 8, 0, 9, 10]
    add_huf("huf-fse-all-weights", w, 900, {"weights-log=6", "huf-zero-weights"}, desc=("fse", wnorm, 6), group="W/all")
    # 252 .. 255 weights of three values in a stream of some fifty bytes: the four-at-a-time loop runs up to its output limit
    for nw in (252, 253, 254, 255):
        n = nw + 1
        c3 = next(c for c in (64, 65) if (512 - n - 3 * c) >= 0 and (n - c - (512 - n - 3 * c)) % 2 == 0)
        c2 = 512 - n - 3 * c3
        c1 = n - c2 - c3
        assert c1 + 2 * c2 + 4 * c3 == 512 and c1 >= 2 and c1 % 2 == 0
        w = [3] * c3 + [2] * c2 + [1] * (c1 - 1)
        w = [int(x) for x in rng.permutation(w)]
        add_huf("huf-fse-%d-long" % nw, w, 1500, {"huf-fse-weights=%d" % nw, "weights-long-stream", "weights-log=6", ">64-of-one-weight"}, desc=("fse", [0, 32, 16, 16], 6), streams=4, group="W/long")
    # a weights table of 67 symbols: one "less than one" symbol in the first 64, three behind them (never used: they are no weights), 60 zeros between in one run
    wn = [-1, 30, 30] + [0] * 61 + [-1, -1, -1]
    w = [1, 2] * 9 + [0] + [2, 1] * 8 + [1]
    add_huf("huf-fse-weights-table-67-symbols-short", w, 400, {"weights-table>64-symbols", "weights-log=6"}, desc=("fse", wn, 6),
            java_refuses="a zero run of 24 and more within five bytes of the description's limit: the 32-bit window of FseTableReader.readFseTable runs dry (libzstd refuses it too)")
    add_huf("huf-fse-weights-table-67-symbols", skew_for(120, zeros=(37,)), 600, {"weights-table>64-symbols", "weights-log=6", "huf-zero-weights"}, desc=("fse", wn, 6), group="W/67",
            differs="a weights table that names symbols above 12 (never used): read by the Java decoder, refused by libzstd")
    # malformed tables
    # (weights whose total is a power of two cannot hold an odd number of weight-1 symbols but for none at all: that is the table the check refuses)
    add_huf("bad-huf-odd-weight-1", [2, 2], 50, {"bad-huf", "odd-weight-1"}, malformed=True, data=bytes(50))
    add_huf("bad-huf-rest-not-power-of-two", [2, 2, 1], 50, {"bad-huf", "rest-not-power-of-two"}, malformed=True, data=bytes(50))  # 5 -> rest 3
    add_huf("bad-huf-weight-13", [13, 1, 1], 50, {"bad-huf", "weight-13"}, malformed=True, data=bytes(50))
    add_huf("bad-huf-all-zero", [0, 0, 0, 0], 50, {"bad-huf", "all-zero"}, malformed=True, data=bytes(50))
    add_huf("bad-huf-256-weights", skew_for(255) + [1], 50, {"bad-huf", "256-weights"}, malformed=True, data=bytes(50), desc=("fse", [-1, 31], 5))
    add_huf("bad-huf-table-past-section", skew_for(127), 50, {"bad-huf", "table-past-section"}, malformed=True, data=bytes(50), streams=1,
            frame_opts={"checksum": False})
    cases[-1].frame = _cut_literals_section(cases[-1].frame, 40)

    # ---- 7. Huffman streams ----
    w6 = [1, 1, 2, 3, 4, 5]  # log 6, seven symbols
    full6 = full_of(w6)[0]
    for n in (1, 2, 3, 4):
        add_huf("huf-one-stream-%d" % n, w6, n, {"huf-size=%d" % n}, data=data_for(full6, n, every=False))
    for n in (4, 5, 6, 7, 8, 9, 10):  # four streams: the sizes at which the fourth stream has a byte to decode, and those at which it has none (or less)
        seg = (n + 3) // 4
        bad = n - 3 * seg < 0
        empty = n - 3 * seg == 0  # (a fourth stream of the mark alone: no symbol to decode)
        add_huf("huf-four-streams-%d" % n, w6, n, {"huf-size=%d" % n, "huf-four-smallest" if n == 4 else "huf-four-small"} | ({"huf-four-empty-fourth"} if empty else set()), streams=4,
                data=data_for(full6, n, every=False), malformed=bad, differs="four Huffman streams for fewer than 6 bytes: read by the Java decoder, refused by libzstd" if n == 4 else None)
    for n in (1, 2, 5):  # the first three segments cover more than the literals: the Java decoder decodes them all the same and wants the fourth stream empty
        seg = (n + 3) // 4
        h = Huf(data_for(full6, 3 * seg, every=False), w6, streams=4, tamper={"regen": n - 3 * seg})
        add("huf-four-streams-%d-overlap" % n, [("c", h, [], pre3)], tags={"huf", "huf-four-overlap"}, fallback="four streams whose first three segments cover more than the literals",
            differs="four Huffman streams for 1, 2 or 5 literals, the first three decoding beyond them: read by the Java decoder, refused by libzstd")
    for around in (256, 1024, 16384):
        for d in (0, 1, 3):
            n = around + d
            add_huf("huf-four-streams-%d" % n, skew_for(40), n, {"huf-size=4k+%d" % d, "huf-around=%d" % around}, streams=4)
    for n in (1023, 1024):  # (each header size in use: the size format follows the sizes)
        add_huf("huf-one-stream-%d" % n, [1, 1], n, {"huf-size-format"}, streams=1 if n < 1024 else 4)
    for tail in (0, 1, 2, 3):
        add_huf("huf-tail-%d" % tail, w6, 20 + tail, {"huf-stream-tail=%d" % tail}, data=data_for(full6, 20 + tail, every=False))
    found = set()
    for tries in range(2000):
        d = data_for(full6, int(rng.integers(5, 30)), every=False)
        last = huffman_stream(d, huffman_codes(full6)[0])[-1]
        if last in (0x01, 0x80) and last not in found:
            found.add(last)
            add_huf("huf-end-mark-%02x" % last, w6, len(d), {"huf-end-mark=%02x" % last}, data=d)
    assert len(found) == 2
    add_huf("bad-huf-jump-table", w6, 40, {"bad-huf-stream", "jump-past-section"}, streams=4, malformed=True, tamper={"jump": lambda j: [j[0], j[1], j[2] + 200]}, data=data_for(full6, 40))
    add_huf("bad-huf-stream-short", w6, 40, {"bad-huf-stream", "stream-decodes-short"}, malformed=True, tamper={"regen": -1}, data=data_for(full6, 40))
    add_huf("bad-huf-stream-long", w6, 40, {"bad-huf-stream", "stream-decodes-long"}, malformed=True, tamper={"regen": 1}, data=data_for(full6, 40))

    # ---- 8. across blocks: treeless literals, repeat-mode tables ----
    def hb(n, treeless=False, streams=1, w=None):
        w = w or w6
        full = full_of(w)[0]
        return huf_block(Huf(data_for(full, n, every=False), None if treeless else w, treeless=treeless, streams=streams))

    rawlit = lambda: ("c", rng.integers(0, 256, 9, dtype=np.uint8).tobytes(), [(4, 5, 5)], pre3)
    add("treeless-next", [hb(60), hb(33, True)], tags={"treeless", "treeless-direct"}, group="across")
    add("treeless-after-raw-literals", [hb(60), rawlit(), hb(44, True, 4)], tags={"treeless", "treeless-after-raw-literals"}, group="across")
    add("treeless-after-raw-block", [hb(60), ("raw", b"raw block bytes"), hb(29, True)], tags={"treeless", "treeless-after-raw-block"}, group="across")
    add("treeless-after-rle-block", [hb(60), ("rle", 0x77, 1000), hb(31, True)], tags={"treeless", "treeless-after-rle-block"}, group="across")
    add("treeless-chain", [hb(300, w=chain_weights(11)), hb(40, True), hb(50, True, 4), hb(61, True)], tags={"treeless", "treeless-chain"}, group="across")
    add("bad-treeless-first", [hb(30, True)], malformed=True, tags={"treeless-first-block"})
    rep_tables = {LL: Tab("fse", [10, 10, 6, 3, 2, -1], 5, key="rep/LL"), OF: Tab("fse", [0, 0, 20, 8, 4], 5, key="rep/OF"), ML: Tab("fse", [16, 8, 4, 2, 1, -1], 5, key="rep/ML")}

    def rep_block(tabs, n=12):
        seqs = [(1 + i % 5, 3 + (i * 3) % 6, 4 + i % 28) for i in range(n)]
        seqs[0] = (4, 3, 4)
        return ("c", rng.integers(0, 256, sum(s[0] for s in seqs) + 2, dtype=np.uint8).tobytes(), seqs, tabs)

    R = Tab("repeat")
    for kind in (LL, OF, ML):
        first = tabs_for(kind, rep_tables[kind], "predefined")
        add("repeat-%s-alone" % KINDS[kind], [rep_block(first), rep_block(tabs_for(kind, R, "predefined"))], tags={"repeat", "repeat=" + KINDS[kind], "repeat-compressed"}, group="across")
    all3 = (rep_tables[LL], rep_tables[OF], rep_tables[ML])
    add("repeat-all-three", [rep_block(all3), rep_block((R, R, R))], tags={"repeat", "repeat-all", "repeat-compressed"}, group="across")
    add("repeat-chain", [rep_block(all3), rep_block((R, R, R)), ("rle", 0x20, 50), rep_block((R, R, R), 30)], tags={"repeat", "repeat-chain"}, group="across")
    rl = (Tab("rle", 16), Tab("rle", 5), Tab("rle", 32))
    lit51 = lambda: rng.integers(0, 256, 51, dtype=np.uint8).tobytes()
    raw64 = ("raw", rng.integers(0, 256, 64, dtype=np.uint8).tobytes())
    add("repeat-rle", [raw64, ("c", lit51(), [(16, 35, 40), (17, 36, 63)], rl), ("c", lit51(), [(17, 35, 32), (16, 36, 50), (17, 36, 44)], (R, R, R))], tags={"repeat", "repeat-rle"}, group="across")
    rl = (Tab("rle", 3), Tab("rle", 2), Tab("rle", 1))
    add("repeat-rle-short", [("c", b"0123456789abcdef", [(3, 4, 5), (3, 4, 6)], rl), ("c", b"0123456789abcdef", [(3, 4, 7), (3, 4, 4), (3, 4, 5)], (R, R, R))], tags={"repeat", "sequences-section<4"},
        java_refuses="fewer than 4 bytes behind the sequence count (ZstdFrameDecompressor.decompressSequences)")
    add("block-above-window", [("c", b"abcd", [(4, 5, 5)], pre3)], tags={"block-above-window"}, frame_opts={"block_within_window": False, "single_segment": True},
        differs="a compressed block larger than the frame's window (a single-segment frame of less content than the block has bytes): read by the Java decoder, refused by libzstd")
    add("repeat-predefined", [rep_block(pre3), rep_block((R, R, R))], tags={"repeat", "repeat-predefined"}, group="across")
    add("bad-repeat-first", [rep_block((R, rep_tables[OF], rep_tables[ML]))], malformed=True, tags={"repeat-first-block"})
    # two frames in one item: tables do not cross frames
    good, plain_good = write_frame([hb(60), hb(20, True)], name="x")
    f2, _ = write_frame([hb(30, True)], name="x")
    cases.append(ECase("bad-two-frames-treeless", good + f2, None, malformed=True, tags={"two-frames-treeless"}, cap=4096))
    g1, p1 = write_frame([rep_block(all3)], name="x")
    g2, _ = write_frame([rep_block((R, R, R))], name="x")
    cases.append(ECase("bad-two-frames-repeat", g1 + g2, None, malformed=True, tags={"two-frames-repeat"}, cap=4096))
    g3, p3 = write_frame([hb(25)], name="x", checksum=True)
    cases.append(ECase("two-frames", good + g3 + g1, plain_good + p3 + p1, tags={"two-frames"}, fallback="more than one frame in the item", group="across"))
    assert len({c.name for c in cases}) == len(cases)
    return cases


def _cut_literals_section(frame, keep):
    """the single compressed block of `frame` with its literals section's compressed size set to `keep`, and the block cut right behind it: the table runs past"""
    h = read_frame_header(frame)
    pos = h["end"]
    lit = read_literals_header(frame, pos + 3)
    assert lit["kind"] == 2 and lit["header_bytes"] == 3
    hh = int.from_bytes(frame[pos + 3:pos + 6], "little")
    hh = (hh & ((1 << 14) - 1)) | (keep << 14)
    body = hh.to_bytes(3, "little") + frame[pos + 6:pos + 6 + keep] + b"\x00"
    out = frame[:pos] + ((len(body) << 3) | 5).to_bytes(3, "little") + body
    return out + (b"\x00\x00\x00\x00" if h["checksum"] else b"")


# ---------------------------------------------------------------- an independent reader: the edges, recounted from the bytes ----------------------------------------------------------------
class _Fwd:
    def __init__(self, buf, pos):
        self.v = int.from_bytes(buf[pos:], "little")
        self.n = 0

    def get(self, w):
        x = (self.v >> self.n) & ((1 << w) - 1)
        self.n += w
        return x


def read_fse_description(buf, pos, max_symbol):
    """reads a table description by RFC 8878 4.1.1 -> {"log", "norm", "bytes", "runs": [extra zeros], "forms": {"short", "long-low", "long-high"}, "halvings": max}, or None
    where it is malformed (zero run past max_symbol; the symbols run out with states left).  The bytes are assumed to be there."""
    r = _Fwd(buf, pos)
    log = r.get(4) + 5
    remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
    norm, runs, forms, halv = [], [], set(), 0
    while remaining > 1 and len(norm) <= max_symbol:
        mx = 2 * threshold - 1 - remaining
        low = (r.v >> r.n) & (threshold - 1)
        if low < mx:
            v = r.get(nbits - 1)
            forms.add("short")
        else:
            v = r.get(nbits)
            if v >= threshold:
                v -= mx
                forms.add("long-high")
            else:
                forms.add("long-low")
        c = v - 1
        norm.append(c)
        remaining -= abs(c)
        h = 0
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
            h += 1
        halv = max(halv, h)
        if c == 0:
            extra = 0
            while True:
                f = r.get(2)
                extra += f
                if f != 3:
                    break
            runs.append(extra)
            if len(norm) + extra > max_symbol:
                return None
            norm += [0] * extra
    if remaining != 1:
        return None
    return {"log": log, "norm": norm, "bytes": (r.n + 7) // 8, "runs": runs, "forms": forms, "halvings": halv}


def scan_item(item):
    """Reads the structure of a VALID item (one or more frames) from its bytes and returns the set of edge tags found there: table descriptions per kind
    (log, -1 patterns, counts, zero runs, value forms), modes, literals kinds, Huffman descriptions, stream end marks, block kinds."""
    tags = set()
    pos = 0
    nframes = 0
    while pos < len(item):
        fh = read_frame_header(item, pos)
        nframes += 1
        tags.add("single-segment" if fh["single_segment"] else "windowed")
        tags.add("checksum" if fh["checksum"] else "no-checksum")
        pos = fh["end"]
        nblocks = 0
        prev = None
        while True:
            last, kind, size = read_block_header(item, pos)
            pos += 3
            nblocks += 1
            tags.add(("raw-block", "rle-block", "compressed-block")[kind])
            if kind == 2:
                end = pos + size
                lit = read_literals_header(item, pos)
                tags.add("literals=" + zc.LITERAL_KINDS[lit["kind"]])
                tags.add("literals-header=%d" % lit["header_bytes"])
                if lit["kind"] >= 2:
                    tags.add("huf-streams=%d" % lit["streams"])
                    tags.add("huf-regen=%d" % lit["regenerated"])
                if lit["kind"] == 3:
                    tags.add("treeless-after-" + {None: "nothing", 0: "raw-block", 1: "rle-block", 2: "compressed"}[prev])
                if lit["kind"] == 2:
                    at = pos + lit["header_bytes"]
                    hb = item[at]
                    if hb >= 128:
                        tags.add("huf-direct=%d" % (hb - 127))
                    else:
                        d = read_fse_description(item, at + 1, 255)
                        tags.add("weights-log=%d" % d["log"])
                        tags.add("huf-fse-bytes=%d" % hb)
                        tags.add("weights-end-mark=%02x" % item[at + hb])
                sp = lit["end"]
                n, form, sp = read_sequence_count(item, sp)
                tags.add("count-form=%d" % (form + 1))
                if n or form:
                    tags.add("nseq=%d" % n)
                    modes = item[sp]
                    sp += 1
                    names = ("predefined", "rle", "compressed", "repeat")
                    three = [(modes >> (6 - 2 * k)) & 3 for k in range(3)]
                    if three == [2, 2, 2]:
                        tags.add("three-compressed")
                    for k, m in enumerate(three):
                        tags.add("%s-mode=%s" % (KINDS[k], names[m]))
                        if m == 1:
                            sp += 1
                        elif m == 2:
                            d = read_fse_description(item, sp, MAX_SYMBOL[k])
                            sp += d["bytes"]
                            K = KINDS[k]
                            norm, log = d["norm"], d["log"]
                            size_ = 1 << log
                            tags.add("%s-log=%d" % (K, log))
                            if log == MAX_LOG[k]:
                                tags.add("%s-log=max" % K)
                            lows = [s for s, c in enumerate(norm) if c == -1]
                            if lows:
                                tags.add("%s-low=%s" % (K, "all" if len(lows) == len([c for c in norm if c]) and len(lows) >= 28 else ("one" if len(lows) == 1 else "some")))
                                if 0 in lows:
                                    tags.add("%s-low-first" % K)
                                if len(norm) - 1 in lows:
                                    tags.add("%s-low-last" % K)
                                if any(norm[s - 1] >= 10 and s + 1 < len(norm) and norm[s + 1] >= 10 for s in lows if s > 0):
                                    tags.add("%s-low-interleaved" % K)
                            big = max(norm)
                            if big == size_ - 1 and lows:
                                tags.add("%s-size-1+low" % K)
                            if big == size_ - 1 and 1 in norm:
                                tags.add("%s-size-1+one" % K)
                            for lim in (65, 128, 300):
                                if big >= lim:
                                    tags.add("%s-states>=%d" % (K, lim))
                            for rr in d["runs"]:
                                tags.add("%s-run=%d" % (K, rr))
                                if rr >= 24:
                                    tags.add("%s-run-ffff" % K)
                            if len(norm) == MAX_SYMBOL[k] + 1 and len(norm) >= 2 and norm[-2] == 0:
                                tags.add("%s-run-to-max-symbol" % K)
                            for f in d["forms"]:
                                tags.add("%s-%s" % (K, f))
                            if d["halvings"] >= 2:
                                tags.add("%s-halvings>=2" % K)
                            if k == 2:
                                tags.add("tail=%d" % min(end - sp, 4))
                    tags.add("seq-end-mark=%02x" % item[end - 1])
                if lit["kind"] >= 2:
                    tags.add("huf-end-mark=%02x" % item[lit["end"] - 1])
                pos = end
            else:
                pos += 1 if kind == 1 else size
            prev = kind
            if last:
                break
        tags.add("blocks=%d" % min(nblocks, 4))
        pos += 4 if fh["checksum"] else 0
    tags.add("frames=%d" % min(nframes, 2))
    return tags


# what scan_item() must find among the VALID cases (each entry: every tag of it in one case).  Per kind where the issue says so.
def required_scan_tags():
    need = []
    for K, k in (("LL", LL), ("OF", OF), ("ML", ML)):
        need += ["%s-log=5" % K, "%s-log=max" % K, "%s-low=one" % K, "%s-low-first" % K, "%s-low-last" % K, "%s-low-interleaved" % K, "%s-size-1+low" % K,
                 "%s-size-1+one" % K, "%s-states>=65" % K, "%s-states>=128" % K, "%s-log=6" % K, "%s-short" % K, "%s-long-low" % K, "%s-long-high" % K, "%s-halvings>=2" % K,
                 "%s-run-to-max-symbol" % K, "%s-mode=predefined" % K, "%s-mode=rle" % K, "%s-mode=compressed" % K, "%s-mode=repeat" % K]
        need += ["%s-run=%d" % (K, r) for r in (1, 2, 3, 4, 6, 7)]
    need += ["LL-low=all", "ML-low=all", "LL-states>=300", "ML-states>=300", "LL-run=24", "LL-run-ffff", "ML-run=24", "ML-run=27", "ML-run=48", "ML-run-ffff", "three-compressed"]
    need += ["tail=1", "tail=2", "tail=3", "nseq=1", "nseq=2", "nseq=3", "count-form=1", "count-form=2", "count-form=3", "seq-end-mark=01", "seq-end-mark=80"]
    need += ["huf-direct=1", "huf-direct=2", "huf-direct=127", "huf-direct=128", "weights-log=5", "weights-log=6", "huf-streams=1", "huf-streams=4", "literals-header=3", "literals-header=4",
             "literals-header=5", "huf-end-mark=01", "huf-end-mark=80", "literals=raw", "literals=rle", "literals=compressed", "literals=treeless", "treeless-after-compressed",
             "treeless-after-raw-block", "treeless-after-rle-block", "raw-block", "rle-block", "single-segment", "windowed", "checksum", "no-checksum", "frames=2"]
    need += ["huf-regen=%d" % n for n in (1, 2, 3, 4, 7, 256, 257, 259, 1024, 1025, 1027, 16384, 16385, 16387)]
    return need


# ... and what the generator's own records must show (tags the bytes alone do not name: which case is which)
def required_case_tags():
    need = ["huf-log=%d" % L for L in range(1, 13)] + ["huf-fse-weights=%d" % n for n in (65, 129, 193, 254, 255)] + ["weights-mod4=%d" % r for r in range(4)]
    need += ["huf-all-equal", "huf-chain", "huf-zero-weights", "last-weight=1", "last-weight=log", ">64-of-one-weight", "huf-direct-odd", "huf-direct-even", "huf-max-length-run",
             "huf-four-smallest", "wide-sequence", "no-extra-bits", "random-table", "treeless-direct", "treeless-after-raw-literals", "treeless-chain", "repeat=LL", "repeat=OF",
             "repeat=ML", "repeat-all", "repeat-compressed", "repeat-rle", "repeat-predefined", "repeat-chain", "two-frames"]
    need += ["huf-stream-tail=%d" % t for t in range(4)] + ["huf-size=4k+%d" % d for d in (0, 1, 3)] + ["huf-around=%d" % a for a in (256, 1024, 16384)]
    return need


REQUIRED_MALFORMED = ["log-above-max", "run-past-max-symbol", "symbol-limit-remaining>1", "tail=0", "seq-end-mark=00", "odd-weight-1", "rest-not-power-of-two", "weight-13", "all-zero",
                      "256-weights", "table-past-section", "jump-past-section", "stream-decodes-short", "stream-decodes-long", "treeless-first-block", "repeat-first-block",
                      "two-frames-treeless", "two-frames-repeat"]


def state_coverage(cases):
    """{table key: (states visited, states a frame here can visit, states)} for every described table the catalog's streams were coded with; a state counts as one a
    frame can visit unless its symbol is an offset code above OF_USABLE"""
    seen = {}
    for c in cases:
        for key, states in c.visited.items():
            seen.setdefault(key, set()).update(states)
    cov = {}
    for key, (kind, norm, log) in TABLES.items():
        table = fse_decode_table(norm, log)
        can = {u for u, (sym, _, _) in enumerate(table) if kind == "W" or usable(kind, sym)}
        cov[key] = (len(seen.get(key, set()) & can), len(can), len(table))
    return cov


# the cases on which the RFC model, libzstd and the Java decoder do not agree (each carries its note in `differs`; the expectation is always the Java decoder's)
KNOWN_DIFFERENCES = ("tail-1-two", "huf-fse-short-4", "huf-fse-short-5", "huf-fse-weights-table-67-symbols-short", "huf-fse-weights-table-67-symbols", "huf-four-streams-4",
                     "huf-four-streams-1-overlap", "huf-four-streams-2-overlap", "huf-four-streams-5-overlap", "repeat-rle-short", "block-above-window")
