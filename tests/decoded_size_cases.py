"""Inputs and rules of the decoded-size checks, shared by tests/test_gpu_decoded_size*.py (the GPU) and tools/hostemu/check_size.py (the same kernels on
the CPU emulator).  The ORACLE is the checker: its encoders write the clean items, its decoders say what an item decodes to.

The rules (include/aircompressor_hip.h, achip_decoded_size_batch):
  R1  an item the op's decoder decodes at exact capacity has status 0 and that length;
  R2  status 0 with outSize N: the decoder at dstCap = N returns N bytes or fails.
"An item decodes at exact capacity" is decided by the oracle alone: with room to spare it decodes to L bytes AND at dstCap = L it decodes to L bytes again.
(The second half matters: an LZ4 block that ends in a match decodes with room to spare and fails at exact room, M/lz4/Lz4RawDecompressor.java:168-171; and the
Zstd decoder returns 0 for ANY input at dstCap = 0, so a capacity of 0 alone proves nothing.)"""
import numpy as np

from tests import common, oracle_lib

# name -> ACHIP_OP_*_DECOMPRESS
OPS = {"lz4": 0, "snappy": 2, "zstd": 4, "lz4frame": 6, "snappyframed": 8, "lz4hadoop": 10, "snappyhadoop": 12}
INT32_MAX = 0x7FFFFFFF


def encode(o, name, data):
    if name.endswith("hadoop"):
        return o.hadoop_compress(name[:-6], data)
    return o.compress(name, data)


def decode(o, name, comp, cap):
    """plaintext bytes, or raises oracle_lib.OracleError"""
    if name.endswith("hadoop"):
        return o.hadoop_decompress(name[:-6], comp, cap)
    return o.decompress(name, comp, cap)


def exact_length(o, name, comp, room):
    """L if the oracle decodes `comp` to L bytes with `room` to spare and again at dstCap = L; else None"""
    try:
        n = len(decode(o, name, comp, room))
        return n if len(decode(o, name, comp, n)) == n else None
    except oracle_lib.OracleError:
        return None


def plains(o, big=True):
    """the plaintexts every op's clean items are written from: (label, bytes)"""
    out = [("empty", b""), ("one byte", b"x")]
    for i, (name, data, _) in enumerate(common.corpus_sample()):
        out.append(("corpus %s" % name, bytes(data[:65536])))
        out.append(("corpus %s odd" % name, bytes(data[:(7919 * (i + 1)) % len(data) | 1])))
    for i, b in enumerate(common.synthetic_blocks(21, 12)):
        out.append(("synthetic %d" % i, bytes(b)))
    for r in (0.1, 0.5, 1.0):
        g = o.random_generator(r, 300000).tobytes()
        out.append(("generator %.1f" % r, g[:65536]))
        out.append(("generator %.1f long" % r, g[1:300000]))  # (several Hadoop chunks / framed chunks)
    rng = np.random.default_rng(3)
    out.append(("noise", rng.integers(0, 256, 70001, dtype=np.uint8).tobytes()))
    if big:
        text = b"".join(bytes(d) for _, d, _ in common.corpus_sample())
        out.append(("4 MiB + 1", (text * ((4 << 20) // len(text) + 2))[:(4 << 20) + 1]))
    return out


def clean_items(o, name, big=True):
    """[(label, compressed, plaintext length)] for op `name`, written by the oracle's encoders"""
    items = [(label, encode(o, name, p), len(p)) for label, p in plains(o, big)]
    if name == "zstd":
        for f in ("with-checksum.zst", "multiple-frames.zst"):
            z = common.golden_zstd(f)
            items.append(("golden %s" % f, z, len(o.decompress("zstd", z, 1 << 20))))
        if big:  # streams from 4 MiB on: no content size, several blocks, a slid window
            text = b"".join(bytes(d) for _, d, _ in common.corpus_sample())
            for n in ((4 << 20) + 12345, (6 << 20) + 1):
                p = (text * (n // len(text) + 1))[:n]
                items.append(("stream of %d" % n, o.zstd_stream_compress(p), n))
        small = [p for _, p in plains(o, False)][2:6]
        items.append(("stream small", o.zstd_stream_compress(small[0]), len(small[0])))
        items.append(("two frames", o.compress("zstd", small[1]) + o.zstd_stream_compress(small[2]), len(small[1]) + len(small[2])))
    if name in ("lz4frame", "snappyframed", "lz4hadoop", "snappyhadoop"):
        a, b = [p for _, p in plains(o, False)][3:5]
        items.append(("two streams", encode(o, name, a) + encode(o, name, b), len(a) + len(b)))
    if name == "lz4frame":
        p = plains(o, False)[4][1]
        skippable = (0x184D2A53).to_bytes(4, "little") + (9).to_bytes(4, "little") + b"skip this"
        items.append(("skippable frame in front", skippable + encode(o, name, p), len(p)))
    return items


# ---- damage ----------------------------------------------------------------------------------------------------------
def _lz4_first_offset_field(comp, at):
    """position of the first sequence's offset field of the LZ4 block that starts at `at`, or None"""
    if at >= len(comp):
        return None
    token = comp[at]
    p = at + 1
    lit = token >> 4
    if lit == 15:
        while p < len(comp):
            v = comp[p]
            p += 1
            lit += v
            if v != 255:
                break
    p += lit
    return p if p + 2 <= len(comp) - 8 else None


def _lz4_payload_start(name, comp):
    if name == "lz4":
        return 0
    if name == "lz4hadoop":
        return 8
    if name == "lz4frame" and len(comp) > 6:
        return 4 + 2 + (8 if comp[4] & 8 else 0) + 1 + 4
    return None


def _lz4_block_span(name, comp):
    """(start, end, length field position, its byte order) of the one LZ4 block of an item that holds exactly one, or None"""
    n = len(comp)
    if name == "lz4":
        return 0, n, None, None
    if name == "lz4hadoop" and n > 8 and 8 + int.from_bytes(comp[4:8], "big") == n:
        return 8, n, 4, "big"
    if name == "lz4frame":
        start = _lz4_payload_start(name, comp)
        if start is not None and start < n:
            size = int.from_bytes(comp[start - 4:start], "little")
            if size < 0x80000000 and start + size + 4 <= n:
                return start, start + size, start - 4, "little"
    return None


def _short_tail(name, comp, rng):
    """The block's last literals cut to fewer than 5 bytes, its lengths mended: a stream every walk accepts and no decoder takes at exact room (the last match ends
    within 5 bytes of the output's end, M/lz4/Lz4RawDecompressor.java:168-171) -- what an encoder that forgot the end-of-block rule would write."""
    span = _lz4_block_span(name, comp)
    if span is None:
        return None
    start, end, field, order = span
    p, token_at, matches = start, None, 0
    while p < end:
        token_at = p
        token = comp[p]
        p += 1
        lit = token >> 4
        if lit == 15:
            while p < end:
                v = comp[p]
                p += 1
                lit += v
                if v != 255:
                    break
        p += lit
        if p >= end:
            break
        p += 2
        if token & 15 == 15:
            while p < end:
                v = comp[p]
                p += 1
                if v != 255:
                    break
        matches += 1
    if p != end or matches == 0 or lit < 5:
        return None
    keep = int(rng.integers(0, 5))
    first_literal = end - lit
    block = bytes(comp[start:token_at]) + bytes([(keep << 4) | (comp[token_at] & 15)]) + bytes(comp[first_literal:first_literal + keep])
    head = bytearray(comp[:start])
    if field is not None:
        head[field:field + 4] = len(block).to_bytes(4, order)
    return bytes(head) + block + bytes(comp[end:])


def damage(name, comp, rng):
    """one damaged copy of `comp` and the kind of damage"""
    b = bytearray(comp)
    n = len(b)
    kind = int(rng.integers(0, 7))
    if kind == 0 and n > 1:
        return bytes(b[:int(rng.integers(0, n if rng.integers(0, 4) else min(n, 4)))]), "truncated"
    if kind == 6:
        d = _short_tail(name, comp, rng)
        if d is not None:
            return d, "short tail"
    if kind == 1 and n > 0:  # a byte of the head: lengths, flags, descriptors
        i = int(rng.integers(0, min(n, 24)))
        b[i] ^= 1 << int(rng.integers(0, 8))
        return bytes(b), "head flip"
    if kind == 2 and n > 0:
        i = int(rng.integers(0, n))
        b[i] = int(rng.integers(0, 256))
        return bytes(b), "byte"
    if kind == 3:
        start = _lz4_payload_start(name, comp)
        at = _lz4_first_offset_field(comp, start) if start is not None else None
        if at is not None:
            b[at:at + 2] = b"\x00\x00" if rng.integers(0, 2) else b"\xff\xff"
            return bytes(b), "lz4 offset"
    if kind == 4 and name in ("zstd", "lz4frame", "snappyframed") and n >= 4:
        b[0:4] = rng.integers(0, 256, 4, dtype=np.uint8).tobytes()
        return bytes(b), "magic"
    if kind == 5 and n > 16:  # a chunk / block length past the end
        if name.endswith("hadoop"):
            b[4:8] = (n * 2 + 5).to_bytes(4, "big")
            return bytes(b), "chunk length"
        if name == "snappyframed":
            b[11:14] = (n * 2 + 5).to_bytes(4, "little")[:3]
            return bytes(b), "chunk length"
        if name == "lz4frame":
            at = _lz4_payload_start(name, comp) - 4
            b[at:at + 4] = (n * 2 + 5).to_bytes(4, "little")
            return bytes(b), "chunk length"
    if n > 0:
        i = int(rng.integers(0, n))
        b[i] ^= 0x80
    return bytes(b), "flip"


def damaged_items(o, name, seed, count):
    """[(kind, damaged bytes, room)]: `count` damaged copies of small clean items; room = a capacity with room to spare for whatever the copy may decode to"""
    rng = np.random.default_rng(seed)
    text = b"".join(bytes(d) for _, d, _ in common.corpus_sample())
    gen = o.random_generator(0.5, 200000).tobytes()
    base = []
    for k in range(24):
        src = text if k % 2 == 0 else gen
        at = int(rng.integers(0, len(src) - 5000))
        base.append(src[at:at + int(rng.integers(20, 5000))])
    base.append(gen[:140000])  # (several chunks of a framed stream)
    comps = [encode(o, name, p) for p in base]
    out = []
    for i in range(count):
        c = comps[i % len(comps)]
        d, kind = damage(name, c, rng)
        out.append((kind, d, 4 * len(base[i % len(comps)]) + 70000))
    return out


# R3's exception, per op: the details (include/aircompressor_hip.h, ACHIP_D_*) of checks that only a decode of the payload can make.  Sizing reads headers
# and lengths; the decoder may meet one of these first, on an earlier byte.  Anything else the decoder stops on, sizing must have stopped on too.
_LZ4_BLOCK = {1, 2, 3, 4, 5, 6, 7}        # ACHIP_D_LZ4_INPUT_EMPTY .. ACHIP_D_LZ4_EMPTY_OUTPUT: the LZ4 block codec
_SNAPPY_BLOCK = {16, 17, 18, 19, 20, 21}  # ACHIP_D_SNAPPY_MALFORMED .. ACHIP_D_SNAPPY_OUTPUT_TOO_SMALL: the Snappy block codec
PAYLOAD_ONLY = {
    "lz4": set(),
    "snappy": set(),
    "zstd": {33, 34, 37},                 # ACHIP_D_ZSTD_OUTPUT_TOO_SMALL, ACHIP_D_ZSTD_CORRUPTED, ACHIP_D_ZSTD_BAD_CHECKSUM
    "lz4frame": _LZ4_BLOCK | {81, 83},    # ... ACHIP_D_LZ4F_BLOCK_CHECKSUM, ACHIP_D_LZ4F_CONTENT_CHECKSUM
    "snappyframed": _SNAPPY_BLOCK | {95},  # ... ACHIP_D_SNF_CHECKSUM
    "lz4hadoop": _LZ4_BLOCK,
    "snappyhadoop": _SNAPPY_BLOCK,
}
# so that the exception cannot hide a regression: of an op's reported faults, at the tests' seeds, at most this share may fall under it (the oracle alone
# gives Zstd 9.9 %, snappyhadoop 3.3 %, snappyframed 0.5 %, the others none)
PAYLOAD_ONLY_MAX_SHARE = 0.15


def payload_share_wrong(name, seen):
    """None, or what is wrong with how many of `name`'s reported faults fell under R3's exception (seen: the categories' counts)"""
    faults = seen["fault"] + seen["payload"]
    if seen["payload"] > PAYLOAD_ONLY_MAX_SHARE * faults:
        return "R3: %s: %d of %d reported faults are excused as payload-only, more than %.0f %%" % (name, seen["payload"], faults, 100 * PAYLOAD_ONLY_MAX_SHARE)
    return None


def judge(o, name, item, room, size, status, err_offset):
    """The verdict for one item given what sizing said: ("exact" | "r2" | "fault" | "payload", None) or (category, "what is wrong").
    R3, a reported fault is the reader's fault: where sizing reports a status, the oracle's decoder with room to spare fails with the same status at the same
    offset ("fault") -- or stopped earlier on a check of PAYLOAD_ONLY[name] ("payload")."""
    length = exact_length(o, name, item, room)
    if length is not None:
        if status != 0 or size != length:
            return "exact", "R1: decodes to %d bytes at exact capacity, sizing said status %d size %d" % (length, status, size)
        return "exact", None
    if status != 0:
        if size != 0:
            return "fault", "a fault leaves outSize 0, got %d" % size
        try:
            got = len(decode(o, name, item, room))
        except oracle_lib.OracleError as e:
            if (e.status, e.offset) == (status, err_offset):
                return "fault", None
            if e.detail in PAYLOAD_ONLY[name]:
                return "payload", None
            return "fault", "R3: sizing said status %d at %d, the decoder with room to spare status %d at %d" % (status, err_offset, e.status, e.offset)
        return "fault", "R3: sizing said status %d at %d, the decoder with room to spare decodes %d bytes" % (status, err_offset, got)
    if 0 <= size <= 1 << 28:  # (a quarter GiB of lazily zeroed pages at most; sizes past INT32_MAX the planner leaves out: no decoder is run on them)
        try:
            got = len(decode(o, name, item, int(size)))
        except oracle_lib.OracleError:
            return "r2", None
        if got != size:
            return "r2", "R2: status 0 size %d, the decoder at that capacity succeeds with %d bytes" % (size, got)
    return "r2", None
