"""A catalog of constructed LZ4 and Snappy streams for the LDS-ring decoders (achip_rings.h under lz4_decode_body.h / snappy_decode_body.h): every stream
is written sequence by sequence -- (literal length, match length, offset) -- so that one named edge of one ring instantiation is met: the near / far cut
(LDS_REACH), the copy_small cut (4 * GS), CHUNK and its multiples, the destination head of copy_dwords_rt, ring wraps inside a move, length bytes across a
refill, the block's end.  Pure Python, deterministic, no oracle and no decoder involved: the plaintext comes from the builders' own byte-sequential model.

    CONFIGS                     (lanes, ring class) -> the ring instantiation the product launches for it
    lz4_stream / snappy_stream  sequence list -> (plaintext, stream)
    cases(codec, config)        valid cases: targeted ones (one edge each, behind a warm-up literal run that wraps the output ring) and grammar ones
                                (sequences drawn by a seeded generator from the same pools)
    malformed(codec, config)    the valid streams damaged at the same edges: (name, condition, stream, capacity)
    labels(case, codec, config) which edges a case reaches under a configuration (a walk of its sequence list)
    label_names(codec, config)  every label there is; UNREACHABLE: the (config, label) cells nothing can reach, with the reason
"""
import collections

import numpy as np

Config = collections.namedtuple("Config", "GS GPL IN_RING OUT_RING phased CHUNK LDS_REACH")


def _cfg(gs, gpl, in_ring, out_ring, phased=0):
    chunk = 16 * gs * gpl
    return Config(gs, gpl, in_ring, out_ring, phased, chunk, out_ring - chunk - 16)


# (lanes per block, ring class) as the context options name them; (4, 3) is the latency class: a wavefront (64 lanes) and 128 KiB of history per block.
# (4, 0) is the phased default (its PHASED template argument: 4 for LZ4, 1 for Snappy); (4, 2) the compact rings kept for comparison.
def _configs(phased):
    return {
        (1, 0): _cfg(1, 2, 64, 128), (1, 1): _cfg(1, 4, 128, 256),
        (2, 0): _cfg(2, 1, 64, 128), (2, 1): _cfg(2, 2, 128, 256),
        (4, 0): _cfg(4, 1, 256, 256, phased), (4, 1): _cfg(4, 1, 256, 512), (4, 2): _cfg(4, 1, 128, 256),
        (8, 0): _cfg(8, 1, 256, 512), (8, 1): _cfg(8, 1, 512, 1024),
        (16, 0): _cfg(16, 1, 512, 1024), (16, 1): _cfg(16, 1, 1024, 2048),
        (32, 0): _cfg(32, 1, 1024, 2048), (32, 1): _cfg(32, 1, 2048, 4096),
        (64, 0): _cfg(64, 1, 2048, 4096), (64, 1): _cfg(64, 1, 4096, 8192),
        (4, 3): _cfg(64, 1, 4096, 131072),
    }


CONFIGS = {"lz4": _configs(4), "snappy": _configs(1)}
LATENCY = (4, 3)
# the (source, destination) misalignments every check runs the catalog at: inBase / outBase of the rings
SHIFTS = ((0, 0), (3, 13), (15, 1), (8, 5))

Case = collections.namedtuple("Case", "name kind seqs tail plain stream")

_POOL = None


def _filler(cursor, n):
    """n bytes of non-repeating filler (random, never 0) from position `cursor` of one fixed pool"""
    global _POOL
    if _POOL is None:
        _POOL = np.random.default_rng(20261019).integers(1, 256, 1 << 19, dtype=np.uint8).tobytes()
    cursor %= len(_POOL)
    out = _POOL[cursor:cursor + n]
    while len(out) < n:
        out += _POOL[:n - len(out)]
    return out


def _extend(plain, off, ml):
    """the byte-sequential model of a back-reference"""
    if off >= ml:
        plain += plain[len(plain) - off:len(plain) - off + ml]
    else:
        seg = bytes(plain[len(plain) - off:])
        plain += (seg * (ml // off + 1))[:ml]


def _lz4_len(n):
    out = bytearray()
    n -= 15
    while n >= 255:
        out.append(255)
        n -= 255
    out.append(n)
    return out


def lz4_stream(seqs, tail, strict=True, trace=None):
    """An LZ4 block of the sequences (literal length, match length >= 4, offset) and a final run of `tail` literals.  strict: the reference's end rules hold
    (the last match ends at least 12 bytes before the end, so every non-final literal run has 8 input bytes behind it) and every offset is inside the output.
    Not strict: whatever is asked for is written; the plaintext is None where the model cannot follow.  trace: gets (ip of the token, op at the literals)."""
    plain, s, cur = bytearray(), bytearray(), 0
    for lit, ml, off in seqs:
        if trace is not None:
            trace.append((len(s), len(plain) if plain is not None else -1))
        assert ml >= 4 and lit >= 0
        s.append((min(lit, 15) << 4) | min(ml - 4, 15))
        if lit >= 15:
            s += _lz4_len(lit)
        f = _filler(cur, lit)
        cur += lit
        s += f
        s += (off & 0xFFFF).to_bytes(2, "little")
        if ml - 4 >= 15:
            s += _lz4_len(ml - 4)
        if plain is not None:
            plain += f
            if 1 <= off <= len(plain) and off <= 65535:
                _extend(plain, off, ml)
            else:
                assert not strict, (lit, ml, off, len(plain))
                plain = None
    assert not strict or not seqs or tail >= 12, tail
    if trace is not None:
        trace.append((len(s), len(plain) if plain is not None else -1))
    s.append(min(tail, 15) << 4)
    if tail >= 15:
        s += _lz4_len(tail)
    f = _filler(cur, tail)
    s += f
    if plain is not None:
        plain += f
    return (bytes(plain) if plain is not None else None), bytes(s)


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _snappy_literal(n, nbytes):
    """header of a literal element: its length in the tag (nbytes 0, n <= 60) or in 1 .. 4 bytes behind it"""
    if nbytes == 0:
        assert 1 <= n <= 60
        return bytes([(n - 1) << 2])
    assert n - 1 < 1 << (8 * nbytes)
    return bytes([(59 + nbytes) << 2]) + (n - 1).to_bytes(nbytes, "little")


def _snappy_copy(n, off, kind):
    if kind == 1:
        assert 4 <= n <= 11 and 0 <= off < 2048
        return bytes([1 | ((n - 4) << 2) | ((off >> 8) << 5), off & 0xFF])
    assert 1 <= n <= 64
    if kind == 2:
        return bytes([2 | ((n - 1) << 2)]) + (off & 0xFFFF).to_bytes(2, "little")
    return bytes([3 | ((n - 1) << 2)]) + (off & 0xFFFFFFFF).to_bytes(4, "little")


def _literal_bytes(n, form):
    """the length bytes behind a literal's tag: what the form asks for (0: in the tag), or the fewest that hold the length if that is more"""
    need = 0 if n <= 60 else (1 if n <= 256 else (2 if n <= 65536 else 3))
    nb = form.get("lit", need)
    return need if (nb == 0 or nb < need) else nb


def snappy_pieces(ml, off, form):
    """how a match of ml bytes is cut into copy elements: [(length, tag kind)].  form: "cut" 64 (64 + 64 + .. + rest) or 60; "copy" a tag kind or a list of
    kinds taken in turn -- a kind the piece cannot have (1-byte offsets: 4 .. 11 bytes from below 2048; 2-byte offsets: below 65536) gives way to the next larger"""
    cut = form.get("cut", 64)
    kinds = form.get("copy", 0)
    kinds = kinds if isinstance(kinds, (list, tuple)) else [kinds]
    out = []
    while ml > 0:
        n = min(ml, cut)
        k = kinds[len(out) % len(kinds)]
        if k == 0:
            k = 1
        if k == 1 and not (4 <= n <= 11 and off < 2048):
            k = 2
        if k == 2 and off >= 65536:
            k = 4
        out.append((n, k))
        ml -= n
    return out


def snappy_stream(elements, strict=True, trace=None, expected=None):
    """A raw Snappy stream of the elements (literal length, match length, offset[, form]): a literal element if the first is not 0, then the copy elements of
    the match if the second is not 0.  form (a dict): "lit": the literal's length in the tag (0) or in 1 .. 4 trailing bytes; "cut" / "copy": snappy_pieces.
    expected: the length the preamble claims, if not the plaintext's.  trace: gets (ip of the first element behind the preamble, op) per entry."""
    plain, s, cur = bytearray(), bytearray(), 0
    for e in elements:
        lit, ml, off = e[:3]
        form = e[3] if len(e) > 3 else {}
        if trace is not None:
            trace.append((len(s), len(plain) if plain is not None else -1))
        if lit > 0:
            nb = _literal_bytes(lit, form)
            f = _filler(cur, lit)
            cur += lit
            s += _snappy_literal(lit, nb) + f
            if plain is not None:
                plain += f
        if ml > 0:
            for n, k in snappy_pieces(ml, off, form):
                s += _snappy_copy(n, off, k)
            if plain is not None:
                if 1 <= off <= len(plain):
                    _extend(plain, off, ml)
                else:
                    assert not strict, (lit, ml, off, len(plain))
                    plain = None
    if trace is not None:
        trace.append((len(s), len(plain) if plain is not None else -1))
    n = expected if expected is not None else len(plain)
    return (bytes(plain) if plain is not None else None), varint(n) + bytes(s)


def build(codec, seqs, tail, strict=True, trace=None):
    if codec == "lz4":
        return lz4_stream(seqs, tail, strict, trace)
    return snappy_stream(list(seqs) + [(tail, 0, 0)], strict, trace)


# ---- the edge values of a configuration ----

def _uniq(values, lo=None, hi=None):
    return sorted({v for v in values if (lo is None or v >= lo) and (hi is None or v <= hi)})


def band(cfg):
    """the offsets around the near / far cut"""
    return list(range(cfg.LDS_REACH - 3, cfg.OUT_RING - cfg.CHUNK + 21))


def offset_values(cfg):
    c, r, g4 = cfg.CHUNK, cfg.OUT_RING, 4 * cfg.GS
    named = {"off:4GS-1": g4 - 1, "off:4GS": g4, "off:4GS+1": g4 + 1, "off:CHUNK/2": c // 2, "off:CHUNK-1": c - 1, "off:CHUNK": c, "off:CHUNK+1": c + 1,
             "off:2CHUNK-1": 2 * c - 1, "off:2CHUNK+1": 2 * c + 1, "off:65535": 65535}
    for v in list(range(1, 10)) + [15, 16, 17]:
        named["off:%d" % v] = v
    for v in band(cfg):
        named["off:REACH%+d" % (v - cfg.LDS_REACH)] = v
    for v in range(r - 17, r + 2):
        named["off:RING%+d" % (v - r)] = v
    return named


def match_values(cfg, codec):
    c, g4 = cfg.CHUNK, 4 * cfg.GS
    named = {"ml:4": 4, "ml:4GS-1": g4 - 1, "ml:4GS": g4, "ml:4GS+1": g4 + 1, "ml:CHUNK-1": c - 1, "ml:CHUNK": c, "ml:CHUNK+1": c + 1, "ml:2CHUNK-1": 2 * c - 1,
            "ml:2CHUNK+1": 2 * c + 1, "ml:3CHUNK+5": 3 * c + 5}
    return {k: v for k, v in named.items() if v >= (4 if codec == "lz4" else 1)}  # (an LZ4 match has 4 bytes at least)


def literal_values(cfg):
    c, g4 = cfg.CHUNK, 4 * cfg.GS
    named = {"lit:4GS-1": g4 - 1, "lit:4GS": g4, "lit:4GS+1": g4 + 1, "lit:2CHUNK-1": 2 * c - 1, "lit:2CHUNK+1": 2 * c + 1}
    for v in (0, 1, 2, 3, 4, 14, 15, 16, 17):
        named["lit:%d" % v] = v
    for v in range(c - 4, c + 2):
        named["lit:CHUNK%+d" % (v - c)] = v
    return named


LZ4_LIT_CHAINS = (269, 270, 271, 524, 525, 526)   # 15 + 254 / 255 / 255 + 0, 15 + 255 + 254 / 255 + 255 / 255 + 255 + 0
LZ4_ML_CHAINS = (273, 274, 528, 529)              # 4 + 15 + 254 / 255 + 0, 4 + 15 + 255 + 254 / 255 + 255 + 0
PERIODIC = (1, 2, 3, 5)                           # and CHUNK - 1
HEADS = ("band-after:dwords-head0", "band-after:dwords-head1", "band-after:dwords-head2", "band-after:dwords-head3", "band-after:small")
SNAPPY_FORMS = ("sn:lit-tag", "sn:lit-1b", "sn:lit-2b", "sn:lit-3b", "sn:lit-4b", "sn:copy1", "sn:copy2", "sn:copy4", "sn:cut64", "sn:cut60", "sn:merge-mixed-tags",
                "sn:nomerge-other-offset", "sn:nomerge-short-piece", "sn:merge>4096")


def label_names(codec, config):
    """every label of a codec and configuration: the list of the module's docstring, written out once"""
    cfg = CONFIGS[codec][config]
    names = list(offset_values(cfg)) + list(literal_values(cfg)) + list(HEADS)
    names += ["%s/%s" % (m, p) for m in match_values(cfg, codec) for p in ("periodic", "plain")]
    names += ["op%%16=%d" % r for r in range(16)] + ["op%CHUNK=0", "op%CHUNK=1", "op%CHUNK=CHUNK-1"]
    names += ["wrap:src", "wrap:dst", "wrap:both", "wrap:in-ring-literal", "end%16=0", "end%16=1", "end%16=15", "short-block"]
    if codec == "lz4":
        names += ["lz4:lit%d" % v for v in LZ4_LIT_CHAINS] + ["lz4:ml%d" % v for v in LZ4_ML_CHAINS] + ["lz4:lit-chain-straddles-refill", "lz4:ml-chain-straddles-refill"]
    else:
        names += list(SNAPPY_FORMS)
    return names


# (config, label) cells nothing within the size limits reaches, each with its reason
def _unreachable():
    out = {}
    for codec in ("lz4", "snappy"):
        cfg = CONFIGS[codec][LATENCY]
        why = ("the latency class keeps 128 KiB of history: its near / far cut (LDS_REACH = %d) and its ring size lie beyond every offset an LZ4 block can hold and "
               "beyond the 65 535 the catalog's blocks of at most 160 KiB go up to" % cfg.LDS_REACH)
        for name, v in offset_values(cfg).items():
            if v > 65535:
                out[(codec, LATENCY, name)] = why
        for name in HEADS:
            out[(codec, LATENCY, name)] = why
        out[(codec, LATENCY, "wrap:both")] = "a move that wraps the 128 KiB ring at its source and at its destination ends beyond 256 KiB: the catalog's blocks end at 160 KiB"
    return out


UNREACHABLE = _unreachable()


# ---- labels: a walk of the sequence list ----

def _last_move(cfg, op, off, n):
    """what the last move of copy_match(op, off, n) is, with its destination head (output base 0): ("small", 0), ("dwords", head) or ("other", 0)"""
    g4 = 4 * cfg.GS
    if n <= g4 and off >= n:
        return ("small", 0)
    if cfg.GS == 4 and cfg.GPL == 1:  # the unified form (with its staging area): every move is a copy_dwords of c <= min(CHUNK, distance) bytes
        dist = off
        while True:
            c = min(n, cfg.CHUNK, dist)
            if n == c:
                return ("dwords", (4 - (op & 3)) & 3)
            op += c
            n -= c
            if dist < cfg.CHUNK:
                dist += dist
    c = (n - 1) % cfg.CHUNK + 1
    c0 = op + n - c
    if off <= cfg.LDS_REACH and off >= c and c > max(cfg.GS, 4):
        return ("dwords", (4 - (c0 & 3)) & 3)
    return ("other", 0)


def labels(case, codec, config):
    """the labels a case reaches under a configuration"""
    cfg = CONFIGS[codec][config]
    c, r = cfg.CHUNK, cfg.OUT_RING
    offs_all, lits_all, mls_all = ({} for _ in range(3))  # value -> its names (two names may be one value: 4 * GS - 1 is 15 at four lanes)
    for names, table in ((offs_all, offset_values(cfg)), (lits_all, literal_values(cfg)), (mls_all, match_values(cfg, codec))):
        for k, v in table.items():
            names.setdefault(v, []).append(k)
    trace = []
    plain, _ = build(codec, case.seqs, case.tail, strict=False, trace=trace)
    got = set()
    in_band = set(band(cfg))
    prev = None  # (op of the match, offset, length) of the sequence before
    for (lit, ml, off, *rest), (ip, op) in zip(case.seqs, trace):
        form = rest[0] if rest else {}
        if codec == "lz4" or lit > 0 or prev is not None:
            got.update(lits_all.get(lit, ()))
        if codec == "lz4":
            if lit in LZ4_LIT_CHAINS:
                got.add("lz4:lit%d" % lit)
            if ml in LZ4_ML_CHAINS:
                got.add("lz4:ml%d" % ml)
            nl = len(_lz4_len(lit)) if lit >= 15 else 0
            nm = len(_lz4_len(ml - 4)) if ml - 4 >= 15 else 0
            for base, _ in SHIFTS:
                if nl >= 2 and (ip + 1 + base) // c != (ip + nl + base) // c:
                    got.add("lz4:lit-chain-straddles-refill")
                m0 = ip + 1 + nl + lit + 2
                if nm >= 2 and (m0 + base) // c != (m0 + nm - 1 + base) // c:
                    got.add("lz4:ml-chain-straddles-refill")
            ipl = ip + 1 + nl
        else:
            nb = _literal_bytes(lit, form)
            if lit > 0:
                got.add("sn:lit-tag" if nb == 0 else "sn:lit-%db" % nb)
            ipl = ip + 1 + nb
        if lit > 0 and ipl // cfg.IN_RING != (ipl + lit - 1) // cfg.IN_RING:
            got.add("wrap:in-ring-literal")
        om = op + lit
        if ml > 0:
            got.update(offs_all.get(off, ()))
            for k in mls_all.get(ml, ()):
                got.add("%s/%s" % (k, "periodic" if off < ml else "plain"))
            got.add("op%%16=%d" % (om % 16))
            if om % c in (0, 1, c - 1):
                got.add("op%%CHUNK=%s" % {0: "0", 1: "1", c - 1: "CHUNK-1"}[om % c])
            src = om - off
            wd = om // r != (om + ml - 1) // r
            ws = src >= 0 and src // r != (src + min(ml, off) - 1) // r
            if wd or ws:
                got.add("wrap:both" if wd and ws else ("wrap:dst" if wd else "wrap:src"))
            if off in in_band and lit == 0 and prev is not None:
                kind, head = _last_move(cfg, *prev[:3])
                if kind == "small":
                    got.add("band-after:small")
                elif kind == "dwords":
                    got.add("band-after:dwords-head%d" % head)
            if codec == "snappy":
                pieces = snappy_pieces(ml, off, form)
                for n, k in pieces:
                    got.add("sn:copy%d" % k)
                if len(pieces) > 1:
                    if pieces[0][0] in (60, 64):
                        got.add("sn:cut%d" % pieces[0][0])
                    if len({k for _, k in pieces}) > 1:
                        got.add("sn:merge-mixed-tags")
                    if ml > 4096 and pieces[0][0] >= 60:
                        got.add("sn:merge>4096")
                if prev is not None and lit == 0 and prev[2] >= 60 and snappy_pieces(prev[2], prev[1], prev[3])[-1][0] >= 60:
                    got.add("sn:nomerge-other-offset" if prev[1] != off else "sn:merge-mixed-tags")
                if prev is not None and lit == 0 and prev[2] > 64 and prev[1] == off and snappy_pieces(prev[2], prev[1], prev[3])[-1][0] < 60:
                    got.add("sn:nomerge-short-piece")
            prev = (om, off, ml, form)
        else:
            prev = None
    n = len(plain) if plain is not None else 0
    if n % 16 in (0, 1, 15):
        got.add("end%%16=%d" % (n % 16))
    if n < 16:
        got.add("short-block")
    return got


# ---- the cases ----

def size_limit(cfg):
    return 65536 if cfg.OUT_RING <= 1024 else min(8 * cfg.OUT_RING, 163840)


def _targeted(codec, config):
    cfg = CONFIGS[codec][config]
    c, r, g4, reach = cfg.CHUNK, cfg.OUT_RING, 4 * cfg.GS, cfg.LDS_REACH
    lat = config == LATENCY
    if lat:  # the latency class runs the cases of the 64-lane large rings (the same CHUNK), and its own ring's wraps and far offsets below
        out = [(n, s, t) for n, s, t in _targeted(codec, (64, 1)) if "after every predecessor" not in n and not n.startswith(("wrap:", "off:65535"))]
        r_small = CONFIGS[codec][(64, 1)].OUT_RING
    else:
        out = []
        r_small = r
    w = r_small + 24  # the warm-up literal run: the output ring has wrapped where the edge sits
    w -= w % 16

    def add(name, seqs, tail=13):
        out.append((name, seqs, tail))

    if not lat:
        mid = g4 + 5
        for name, off in offset_values(cfg).items():
            if off == 65535:
                continue
            ww = max(w, off + (-off) % 16)
            add(name, [(ww, mid, off)])
            if off in (reach - 1, reach, reach + 1, reach + 2, r - c - 1, r - c, r - c + 1, r - c + 4, r - c + 5):
                add(name + ",ml4", [(ww + 5, 4, off)])
                add(name + ",mlCHUNK+7", [(ww + 10, c + 7, off)])
        # the near / far band behind every kind of predecessor move: a full-extent copy_dwords with destination head 0 .. 3, a copy_small
        unified = cfg.GS == 4 and cfg.GPL == 1
        # (one stream per offset, so that the large rings' catalogs stay within their size: the five predecessors follow each other, a few literals between them)
        for off in band(cfg):
            op = max(w, off + (-off) % 16) + 16
            seqs = []
            for head in range(4):
                if unified:  # the shortest copy_dwords there is: a periodic match ends in a move of one byte
                    pre = (16 + (1 - head - op) % 4, 4, 3)  # moves of 3 and 1 bytes; the last at op + 3
                else:        # max(GS, 4) + 1 bytes behind whole chunks
                    pre = (16 + (-head - c - op) % 4, c + max(cfg.GS, 4) + 1, c + 3)
                if not seqs:
                    pre = (op + pre[0] - 16,) + pre[1:]
                    op = 0
                assert _last_move(cfg, op + pre[0], pre[2], pre[1]) == ("dwords", head), (config, pre)
                seqs += [pre, (0, mid, off)]
                op += pre[0] + pre[1] + mid
            seqs += [(7, 4, 9), (0, mid, off)]
            add("REACH%+d after every predecessor move" % (off - reach), seqs)
        for name, ml in match_values(cfg, codec).items():
            for p in PERIODIC + (c - 1,):
                if p < ml:
                    add("%s/periodic off %d" % (name, p), [(w + 3, ml, p)])
            add("%s/plain" % name, [(max(w, ml) + 6, ml, ml)])
            if max(ml, r - 5) <= max(w, ml) + 9:
                add("%s/plain far" % name, [(max(w, ml) + 9, ml, max(ml, r - 5))])
        for name, lit in literal_values(cfg).items():
            add(name, [(w, 9, 11), (lit, mid, c + 9)])
        if codec == "lz4":
            # the 255 chains, placed so that the chain's bytes straddle a CHUNK boundary of the input at each of the four input bases
            for base, _ in SHIFTS:
                for lit in LZ4_LIT_CHAINS:
                    # token of the second sequence at ip0: 1 + len(ext(w1)) + w1 + 2 bytes of the first sequence in front of it
                    for w1 in range(w, w + 2 * c + 1):
                        ip0 = 1 + len(_lz4_len(w1)) + w1 + 2
                        if (ip0 + 2 + base) % c == 0:
                            break
                    add("lz4:lit%d chain over a refill, input base %d" % (lit, base), [(w1, 8, 13), (lit, mid, 21)])
                for ml in LZ4_ML_CHAINS:
                    for w1 in range(w, w + 2 * c + 1):
                        m0 = 1 + len(_lz4_len(w1)) + w1 + 2
                        if (m0 + 1 + base) % c == 0:
                            break
                    add("lz4:ml%d chain over a refill, input base %d" % (ml, base), [(w1, ml, 21)])
                # (the decoder reads the token's and the offset's 4-byte windows ahead: only a chain's byte beyond the window is fetched by the chain's own
                #  loop -- chains of five bytes, the first byte outside the window on the far side of the boundary)
                for w1 in range(w, w + 2 * c + 1):
                    if (1 + len(_lz4_len(w1)) + w1 + 2 + 4 + base) % c == 0:
                        break
                add("lz4:lit1042 chain, a refill inside its loop, input base %d" % base, [(w1, 8, 13), (15 + 4 * 255 + 7, mid, 21)])
                for w1 in range(w, w + 2 * c + 1):
                    if (1 + len(_lz4_len(w1)) + w1 + 2 + 2 + base) % c == 0:
                        break
                add("lz4:ml1046 chain, a refill inside its loop, input base %d" % base, [(w1, 4 + 15 + 4 * 255 + 7, 21)])
                # the offset read ahead of a literal run of just under a chunk (lit + 3 <= CHUNK): the run and the 3 bytes behind it end 1 byte past a
                # refill boundary -- one more byte of reach would cost the input ring the run's first bytes where it holds two chunks
                for lit in (c - 3, c - 1, c):
                    for w1 in range(w, w + 2 * c + 1):
                        start = 1 + len(_lz4_len(w1)) + w1 + 2 + 1 + (len(_lz4_len(lit)) if lit >= 15 else 0)
                        if (start + lit + 3 + base) % c == 1:
                            break
                    add("lz4:lit CHUNK%+d and the offset behind it end 1 past a refill, input base %d" % (lit - c, base), [(w1, 8, 13), (lit, mid, 21)])
        for res in range(16):
            add("op%%16=%d" % res, [(w + res, mid, c + 9)])
        for res, what in ((0, "0"), (1, "1"), (c - 1, "CHUNK-1")):
            add("op%%CHUNK=%s" % what, [(r_small + c + res, c + 3, 2 * c + 1)])
            add("op%%CHUNK=%s, ends on the flush boundary" % what, [(r_small + c + res, 2 * c - res, c + 9)])
    # moves that wrap the output ring at their source, their destination, both; a literal run that wraps the input ring
    k = min(c // 2, 40)
    e = r if lat else 2 * r
    add("wrap:dst", [(e - k, 3 * k, 4 * k + 1)])
    add("wrap:src", [(e + k, 3 * k, 2 * k)])
    if r <= 65535:
        add("wrap:both", [(2 * r - k, 3 * k, r)])
    add("wrap:dst periodic", [(e - k, 3 * k, 3)])
    if lat:
        add("off:65535", [(65536 + 48, 4 * 64 + 5, 65535)])
        add("off:65535 long", [(65536 + 51, 3 * c + 5, 65535), (3, 70, 65535 - c)])
    else:
        add("wrap:in-ring-literal", [(w, 9, 11), (cfg.IN_RING, g4 + 5, c + 9)])
        add("off:65535", [(65536 + 48, g4 + 5, 65535)])
        # the block's end at 0, 1 and 15 mod 16; blocks shorter than 16 bytes (flush_all's byte paths)
        for res in (0, 1, 15):
            add("end%%16=%d" % res, [(w, g4 + 5, 9)], 16 + (res - (w + g4 + 5)) % 16)
        for n in (1, 2, 15):
            out.append(("short-block %d" % n, [], n))
        if codec == "snappy":
            add("short-block with a copy", [(3, 7, 2)], 2)
            for nb in (1, 2, 3, 4):
                add("sn:lit-%db" % nb, [(w, 9, 11, {"lit": max(nb, 2)}), (61, mid, c + 9, {"lit": nb})])
            add("sn:lit-tag 60", [(w, 9, 11), (60, mid, c + 9, {"lit": 0})])
            for kind in (1, 2, 4):
                add("sn:copy%d" % kind, [(w, 9, 11, {"copy": kind}), (3, 11, min(2047, w), {"copy": kind}), (0, 4, 1, {"copy": kind})])
            add("sn:copy4 beyond 65535", [(65536 + 40, 70, 65536 + 30)])
            for cut in (64, 60):
                add("sn:cut%d" % cut, [(w, 64 + 37, c + 9, {"cut": cut}), (5, 3 * 64 + 11, 7, {"cut": cut})])
            add("sn:merge-mixed-tags", [(w, 64 * 3 + 7, 2 * c + 1, {"copy": [2, 4, 2, 1]}), (0, 64, 2 * c + 1, {"copy": 4})])
            add("sn:nomerge-other-offset", [(w, 64, c + 9), (0, 64, c + 10), (0, 60, c + 10, {"cut": 60}), (0, 30, c + 11)])
            add("sn:nomerge-short-piece", [(w, 64 + 59, c + 9), (0, 64, c + 9)])
            add("sn:merge>4096", [(w, 4096 + 64 * 2 + 9, reach)])
            add("sn:merge reaches 4096", [(w, 4096, 5)])
            add("sn:merge to the last element", [(w, 64 * 3, c + 9)], 0)
            add("sn:trailer at the end", [(w, 64, c + 9), (0, 7, 9, {"copy": 4})], 0)
    return out


class _Turns:
    """values taken in turn from shuffled pools, across the grammar streams of one configuration: a value that does not fit where it is asked for
    waits for the next call, so a few streams of a few dozen sequences meet every value"""

    def __init__(self, rng, pools):
        self.pools = {k: [v[i] for i in rng.permutation(len(v))] for k, v in pools.items()}
        self.left = {k: list(v) for k, v in self.pools.items()}
        self.rounds = {k: 0 for k in pools}

    def take(self, what, ok=lambda v: True):
        for source in (self.left[what], self.pools[what]):
            for i, v in enumerate(source):
                if ok(v):
                    if source is self.left[what]:
                        del source[i]
                        if not source:
                            self.left[what] = list(self.pools[what])
                            self.rounds[what] += 1
                    return int(v)
        return None


PRODUCTIONS = ("plain", "ring-edge", "band", "position", "chain", "periodic", "long-plain", "plain", "merge", "plain")


def _grammar(codec, config, index, rng, turns, far, long_ring):
    """one stream of sequences drawn from the pools of edge values: the productions in turn, their values from `turns`"""
    cfg = CONFIGS[codec][config]
    c, r, g4 = cfg.CHUNK, cfg.OUT_RING, 4 * cfg.GS
    max_off = 65535 if codec == "lz4" else 1 << 30
    bnd = band(cfg)
    if far:          # a stream that starts beyond 64 KiB, so that offset 65535 is met
        w, limit = 65536 + 16 + index % 16, 65536 + max(4 * r, 4096) if r <= 8192 else 65536 + 16 * c
    elif long_ring:  # the latency class: a stream that passes the end of its ring of 128 KiB
        w, limit = r - 3 * c - index % 16, r + 8 * c
    else:
        w, limit = min(r, 8192) + 16 + index % 16, min(size_limit(cfg), 16 * r + 8192) - 6 * c - (1200 if codec == "lz4" else 4500)
    seqs = [(w, turns.take("ml", lambda v: v <= c + 1), 65535 if far else turns.take("off", lambda v: v <= w))]
    op = w + seqs[0][1]

    def form(lit):
        if codec == "lz4":
            return ()
        return ({"lit": int(rng.integers(0, 5)), "copy": [(1, 2, 4)[int(rng.integers(0, 3))] for _ in range(3)], "cut": 60 if rng.integers(0, 3) == 0 else 64},)

    k = index
    while op < limit:
        prod = PRODUCTIONS[k % len(PRODUCTIONS)]
        k += 1
        nxt = (op // r + 1) * r
        lit = turns.take("lit")
        if nxt - op < 3 * c and prod in ("plain", "ring-edge", "position"):
            # the ring's edge ahead: a move that wraps at its destination, at both ends, or (just behind the edge) at its source
            n = int(rng.integers(1, min(c, 48)))
            which = turns.take("wrap") if config != LATENCY else (0, 2)[index % 2]  # (both ends of the 128 KiB ring at once: UNREACHABLE)
            lit = nxt - op - n if which < 2 else nxt - op + n
            off = (4 * n + 1 if which == 0 else r) if which < 2 else 2 * n
            if lit >= 0 and off <= min(op + lit, max_off):
                seqs.append((lit, 3 * n + 4, off) + form(lit))
                op += lit + 3 * n + 4
                continue
            lit = turns.take("lit")
        if prod == "band" and op > bnd[-1] + 4 * c and bnd[-1] <= max_off and config != LATENCY:
            # a predecessor move (a copy_small, or a full-extent copy_dwords with each destination head), then an offset of the near / far band
            which = turns.take("pred")
            if which == 4:
                pre = (lit, 4, 9)
            else:
                pre = (lit, 4, 3) if cfg.GS == 4 and cfg.GPL == 1 else (lit, c + max(cfg.GS, 4) + 1, c + 3)
                while _last_move(cfg, op + pre[0], pre[2], pre[1]) != ("dwords", which):
                    pre = (pre[0] + 1,) + pre[1:]
            seqs += [pre + form(pre[0]), (0, g4 + 5, turns.take("band"))]
            op += pre[0] + pre[1] + g4 + 5
            continue
        if prod == "position":  # the next match starts at 0, 1 or CHUNK - 1 past a CHUNK boundary
            lit = (-op) % c + (0, 1, c - 1)[turns.take("pos")]
        if prod == "chain" and codec == "lz4":
            # a chain of length bytes over a CHUNK boundary of the input (at one of the four input bases): the literal run in front of it is found by trying
            ip = len(build(codec, seqs, 13)[1]) - 14
            which = turns.take("chain")
            for pad in range(0, 2 * c):
                at = ip + 1 + (len(_lz4_len(pad)) if pad >= 15 else 0) + pad + 2 + (2 if which in LZ4_LIT_CHAINS else 4)
                if any((at + b) % c == 0 for b, _ in SHIFTS):
                    break
            seqs.append((pad, 4, turns.take("off", lambda v: v <= op + pad)))
            seqs.append((which, 4, 1) if which in LZ4_LIT_CHAINS else (0, which, 21))
            op += pad + 4 + seqs[-1][0] + seqs[-1][1]
            continue
        if prod == "periodic":
            ml = turns.take("mlp")
            off = turns.take("per", lambda v: v < ml)
        elif prod == "long-plain":
            ml = turns.take("mlq")
            off = turns.take("off", lambda v: ml <= v <= op + lit) or (ml if ml <= op + lit else None)
        else:
            ml = turns.take("ml") if k % 4 == 0 else turns.take("ml", lambda v: v <= c + 1)  # (mostly short matches: more sequences in a stream of limited size)
            off = turns.take("off", lambda v: v <= op + lit)
        if off is None:
            ml, off = 4, 1
        seqs.append((lit, ml, off) + form(lit))
        op += lit + ml
        if codec == "snappy" and ml >= 64 and prod != "periodic":  # a copy directly behind a full piece: the same offset in another tag, or another offset
            same = k % 2 == 0
            seqs.append((0, 64 if same else 30, off if same or off + 1 > op else off + 1, {"copy": 4 if same else 2}))
            op += seqs[-1][1]
        if codec == "snappy" and prod == "merge" and op < limit:  # a match cut into whole pieces that passes 4096 bytes, and a copy with another offset behind it
            off = turns.take("off", lambda v: v <= op)
            seqs += [(0, 4096 + 64 * 3, off, {"cut": 64}), (0, 30, off - 1 if off > 1 else 2)]
            op += 4096 + 64 * 3 + 30
    tail = 16 + ((0, 1, 15)[index % 3] - op) % 16
    return seqs, tail


def _grammar_cases(codec, config):
    """the grammar streams of a configuration: as many as it takes for the pools of offsets and lengths to have gone round twice (once for the large rings, whose streams are the long ones) and the other pools once,
    one in four starting beyond 64 KiB, and two blocks shorter than 16 bytes"""
    cfg = CONFIGS[codec][config]
    c = cfg.CHUNK
    rng = np.random.default_rng([config[0], config[1], int(codec == "snappy")])
    pools = {"off": _uniq((v for v in offset_values(cfg).values() if v != 65535), 1, 65535 if codec == "lz4" or config == LATENCY else None), "ml": _uniq(match_values(cfg, codec).values()) + list(LZ4_ML_CHAINS),
             "lit": _uniq(literal_values(cfg).values()) + (list(LZ4_LIT_CHAINS) if codec == "lz4" else [61, 257]), "band": band(cfg), "pred": [0, 1, 2, 3, 4],
             "wrap": [0, 1, 2], "pos": [0, 1, 2], "chain": list(LZ4_LIT_CHAINS + LZ4_ML_CHAINS), "mlp": _uniq(match_values(cfg, codec).values(), 2), "mlq": _uniq(match_values(cfg, codec).values()),
             "per": list(PERIODIC) + [c - 1]}
    turns = _Turns(rng, pools)  # (offset 65535 is not in the pool: the stream that starts beyond 64 KiB begins with it)
    out = []
    often, rarely = {"off", "ml", "lit"}, {"mlp", "mlq"} | ({"band"} if config != LATENCY else set()) | ({"chain"} if codec == "lz4" else set())
    while (len(out) < (4 if config != LATENCY else 6) or min(turns.rounds[k] for k in often) < (2 if cfg.OUT_RING <= 1024 else 1) or min(turns.rounds[k] for k in rarely) < 1) and len(out) < 40:
        i = len(out)
        out.append(("grammar %d" % i,) + _grammar(codec, config, i, rng, turns, far=(i == 1), long_ring=(config == LATENCY and i in (2, 3))))
    for i in range(2):
        if codec == "lz4":
            out.append(("grammar short %d" % i, [], int(rng.integers(1, 16))))
        else:
            lit = int(rng.integers(1, 5))
            out.append(("grammar short %d" % i, [(lit, int(rng.integers(4, 8)), int(rng.integers(1, lit + 1)))], int(rng.integers(0, 4))))
    return out


_cache = {}


def cases(codec, config):
    """[Case]: the valid cases of a codec and ring configuration -- targeted ones, then grammar ones"""
    key = (codec, config)
    if key not in _cache:
        out = []
        for name, seqs, tail in _targeted(codec, config):
            plain, stream = build(codec, seqs, tail, strict=not name.startswith("short-block"))
            out.append(Case(name, "targeted", seqs, tail, plain, stream))
        for name, seqs, tail in _grammar_cases(codec, config):
            plain, stream = build(codec, seqs, tail, strict=bool(seqs) and codec == "lz4")
            out.append(Case(name, "grammar", seqs, tail, plain, stream))
        assert len({c.name for c in out}) == len(out), [n for n, k in collections.Counter(c.name for c in out).items() if k > 1]
        _cache[key] = out
    return _cache[key]


def malformed(codec, config):
    """[(name, the condition it breaks, stream, capacity)]: valid targeted streams damaged at the same edges, in the order the Java decoders check"""
    cfg = CONFIGS[codec][config]
    c, r, g4 = cfg.CHUNK, cfg.OUT_RING, 4 * cfg.GS
    reach = min(cfg.LDS_REACH, CONFIGS[codec][(64, 1)].LDS_REACH)
    w = reach + 40 - reach % 16
    out = []
    if codec == "lz4":
        mk = lambda seqs, tail=13: lz4_stream(seqs, tail, strict=False)
        plain, good = mk([(w, g4 + 5, reach)])
        n = len(plain)
        out.append(("offset = op + 1", "offset > op", mk([(w, g4 + 5, w + 1)])[1], n))
        out.append(("offset = 0", "offset == 0", mk([(w, g4 + 5, 0)])[1], n))
        out.append(("offset = 0 behind a move", "offset == 0", mk([(w, 4, 3), (0, g4 + 5, 0)])[1], n + 4))
        p4, s4 = mk([(w, g4 + 5, reach)], 4)
        out.append(("match ends inside the last 5 bytes", "matchOutLimit > outLimit - 5", s4, len(p4)))
        p11, s11 = mk([(w, g4 + 5, reach), (3, 4, reach + 1)], 13)
        out.append(("match ends inside the last 12 bytes, a sequence behind it", "literals behind it are the last", s11, len(p11) - 9))
        out.append(("literal run one byte past the capacity", "litOutLimit > outLimit", good, n - 1))
        out.append(("first literal run one byte past the capacity", "litOutLimit > outLimit", mk([], 40)[1], 39))
        out.append(("literal run one byte past the input", "litEnd != inLimit", good[:-1], n))
        out.append(("input not consumed", "litEnd != inLimit", good + b"\x00", n + 8))
        prefix = mk([(w, 4, reach)], 0)[1][:-1]  # one whole sequence, no final token
        for at in (15, 5):
            for d in (-1, 0, 1):
                # a literal-length chain / a match-length chain of 255s whose last byte sits at inLimit - 15 / inLimit - 5 (+-1)
                out.append(("literal length chain ends at inLimit - %d%+d" % (at, d), "the chain's loop stops at inLimit - 15", prefix + bytes([0xF0]) + b"\xff" * 3 + b"\x07" * (at + d), n + 4096))
                out.append(("match length chain ends at inLimit - %d%+d" % (at, d), "ip > inLimit - 5 inside the chain",
                            prefix + bytes([0x0F]) + (9).to_bytes(2, "little") + b"\xff" * 3 + b"\xff" * (at + d), n + 4096))
    else:
        mk = lambda el, **kw: snappy_stream(el, strict=False, **kw)
        plain, good = mk([(w, g4 + 5, reach), (13, 0, 0)])
        n = len(plain)
        out.append(("offset = op + 1", "matchOffset > op", mk([(w, g4 + 5, w + 1), (13, 0, 0)], expected=n)[1], n))
        out.append(("offset = 0", "matchOffset <= 0", mk([(w, g4 + 5, 0, {"copy": 2}), (13, 0, 0)], expected=n)[1], n))
        out.append(("offset = 0 behind a move", "matchOffset <= 0", mk([(w, 4, 3), (0, g4 + 5, 0, {"copy": 4}), (13, 0, 0)], expected=n + 4)[1], n + 4))
        out.append(("copy one byte past the capacity", "op + length > outLimit", mk([(w, g4 + 5, reach)], expected=w + g4 + 4)[1], w + g4 + 4))
        out.append(("literal run one byte past the capacity", "litOutLimit > outLimit", mk([(w, g4 + 5, reach), (13, 0, 0)], expected=n - 1)[1], n - 1))
        out.append(("literal run one byte past the input", "ip + lit > inLimit", good[:-1], n))
        out.append(("trailer cut: ip + 4 == inLimit + 1", "ip + trailerBytes > inLimit", mk([(w, 64, reach), (0, 7, 9, {"copy": 4})])[1][:-1], w + 71))
        out.append(("literal trailer cut", "ip + trailerBytes > inLimit", mk([(w, 9, 11), (300, 0, 0, {"lit": 4})])[1][:-302], w + 309))
        # a continuation element that does not fit: left to the next trip, which fails at it
        out.append(("continuation element past the capacity", "op + total + length2 > outLimit", mk([(w, 64 * 3, reach)], expected=w + 64 * 2 + 10)[1], w + 64 * 2 + 10))
        out.append(("negative 4-byte literal length", "trailer < 0", varint(n) + good[len(varint(n)):len(good) - 14] + bytes([63 << 2, 0xFF, 0xFF, 0xFF, 0xFF]) + b"x" * 13, n))
        out.append(("negative 4-byte offset", "trailer < 0", varint(n) + good[len(varint(n)):len(good) - 14] + bytes([3 | (12 << 2), 0, 0, 0, 0x80]) + b"x" * 13, n))
        out.append(("negative 4-byte offset behind a full piece", "trailer2 < 0 stops the merge",
                    mk([(w, 64, reach)], expected=w + 77)[1] + bytes([3 | (12 << 2), 0, 0, 0, 0x80]) + b"x" * 13, w + 77))
        # a continuation element cut inside its trailer, the missing bytes being zeros of the same offset: merging may not look at an element whose header
        # the loop's `ip + 5 < inLimit` does not cover -- the next trip refuses it (:90-92)
        near = mk([(w, 64, 100)], expected=w + 128)[1]
        out.append(("continuation element cut inside its 2-byte offset", "ip + trailerBytes > inLimit", near + bytes([2 | (63 << 2), 100]), w + 128))
        out.append(("continuation element cut inside its 4-byte offset", "ip + trailerBytes > inLimit", near + bytes([3 | (63 << 2), 100, 0, 0]), w + 128))
        out.append(("length mismatch", "expected != op", mk([(w, g4 + 5, reach), (13, 0, 0)], expected=n + 1)[1], n + 1))
    return out
