"""The LZ4 frame reader with linked blocks, in Python: the model the kernels are held to (achip_ctx_set_lz4frame_linked_blocks), and writers of such frames.

Reader.  decompress(data, cap, accept_linked) restates Lz4FrameCompression.decompress / decompressFrame / skipFrame (M/lz4/Lz4FrameCompression.java:145-343) and
Lz4RawDecompressor.decompress (M/lz4/Lz4RawDecompressor.java:35-198) check by check, in their order, and reports what the ABI reports: the status
-(class + 16 * detail), the offset of the failure (the block decoder's relative to its block), the bytes.  With accept_linked it adds the one rule of the LZ4
Frame format's "Block Independence flag": in a frame whose FLG has bit 5 clear, a match of a block may begin up to 65 535 bytes in front of the position being
written, in the content of the SAME frame decoded so far -- the offset is compared with the bytes of this frame produced so far instead of the bytes of this
block.  Nothing else moves.  tests/test_lz4_linked_ref.py holds the model to the oracle wherever the oracle has an answer (every frame of independent blocks,
every refusal), so what is new here is that rule alone.

Walk.  walk(data) reads the same bytes without decoding them -- frame flags, block boundaries, every sequence's position, lengths and offset -- for the proofs
that a constructed case holds the edge its label names.

Writers.  frame(...) puts a frame together from blocks given sequence by sequence (literal length, match length, offset), in the manner of
tests/decoder_edge_cases.py: the plaintext comes from the writer's own byte-sequential model, carried across the blocks of a frame.  greedy_blocks(...) is a small
greedy encoder: one hash table over the whole frame content, a 64 KiB window, sequences cut at block boundaries, the end-of-block rules honoured (the last five
bytes are literals, no match starts in the last twelve); linked=False confines its matches to the block, which gives the same content as independent blocks.
Pure Python, deterministic, no oracle and no decoder involved."""
import collections
import struct

from tests import decoder_edge_cases as dec

MAGIC, SKIPPABLE_MAGIC, SKIPPABLE_MASK = 0x184D2204, 0x184D2A50, 0xFFFFFFF0
FLG_VERSION, FLG_INDEPENDENT, FLG_BLOCK_CHECKSUM, FLG_CONTENT_SIZE, FLG_CONTENT_CHECKSUM, FLG_RESERVED, FLG_DICTIONARY = 1 << 6, 1 << 5, 1 << 4, 1 << 3, 1 << 2, 1 << 1, 1
BD_RESERVED = 0x8F
HEADER_SIZE = 7
STORED = 0x80000000
MAX_DISTANCE = 65535

CLASS_MALFORMED, CLASS_OUTPUT_TOO_SMALL = 1, 2
# include/aircompressor_hip.h: ACHIP_D_LZ4_* and ACHIP_D_LZ4F_*
D_LZ4_INPUT_EMPTY, D_LZ4_MALFORMED, D_LZ4_LAST_LITERAL_OUTSIDE, D_LZ4_INPUT_NOT_CONSUMED, D_LZ4_OFFSET_OUTSIDE, D_LZ4_LAST_5_LITERALS, D_LZ4_EMPTY_OUTPUT = 1, 2, 3, 4, 5, 6, 7
(D_TOO_SHORT, D_TRUNC_MAGIC, D_BAD_MAGIC, D_TRUNC_HEADER, D_VERSION_0, D_VERSION_2, D_VERSION_3, D_RESERVED_BITS, D_LINKED_BLOCKS, D_DICTIONARY, D_BLOCK_MAX_SIZE,
 D_HEADER_CHECKSUM, D_MISSING_BLOCK_SIZE, D_BLOCK_PAST_END, D_OUTPUT_TOO_SMALL, D_BLOCK_EXCEEDS_MAX, D_MISSING_BLOCK_CHECKSUM, D_BLOCK_CHECKSUM,
 D_MISSING_CONTENT_CHECKSUM, D_CONTENT_CHECKSUM, D_CONTENT_SIZE, D_TRUNC_SKIP_SIZE, D_TRUNC_SKIP) = range(64, 87)


def mk_status(cls, detail):
    return -(cls + 16 * detail)


def malformed(detail):
    return mk_status(CLASS_MALFORMED, detail)


# ---- XXH32 (the frame format's checksum) ----------------------------------------------------------------------------------------------------------------------
_P1, _P2, _P3, _P4, _P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
_M = 0xFFFFFFFF


def _rotl(v, r):
    return ((v << r) | (v >> (32 - r))) & _M


def xxh32(data, seed=0):
    data = bytes(data)
    n, p = len(data), 0
    if n >= 16:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed & _M, (seed - _P1) & _M]
        words = struct.unpack_from("<%dI" % (n // 16 * 4), data)
        for k, w in enumerate(words):
            v[k & 3] = (_rotl((v[k & 3] + w * _P2) & _M, 13) * _P1) & _M
        p = n // 16 * 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while p + 4 <= n:
        h = (_rotl((h + struct.unpack_from("<I", data, p)[0] * _P3) & _M, 17) * _P4) & _M
        p += 4
    while p < n:
        h = (_rotl((h + data[p] * _P5) & _M, 11) * _P1) & _M
        p += 1
    h ^= h >> 15
    h = (h * _P2) & _M
    h ^= h >> 13
    h = (h * _P3) & _M
    return h ^ (h >> 16)


# ---- the reader -----------------------------------------------------------------------------------------------------------------------------------------------
Result = collections.namedtuple("Result", "status offset out")


class _Fail(Exception):
    def __init__(self, status, offset):
        super().__init__(status, offset)
        self.status, self.offset = status, offset


def block_decode(src, out_limit, window=b""):
    """Lz4RawDecompressor.decompress over one block: -> (status, offset, bytes).  `window`: what lies in front of the block's first byte and may be matched
    (the content of a linked frame so far, its last 65 535 bytes at most); b"" is the reference's decoder."""
    in_limit = len(src)
    if in_limit == 0:  # :48-50
        return malformed(D_LZ4_INPUT_EMPTY), 0, b""
    if out_limit == 0:  # :52-57 (the method returns -1)
        if in_limit == 1 and src[0] == 0:
            return 0, 0, b""
        return mk_status(CLASS_OUTPUT_TOO_SMALL, D_LZ4_EMPTY_OUTPUT), 0, b""
    history = len(window)
    buf = bytearray(window)  # the block's byte k is buf[history + k]
    fast_out_limit = out_limit - 8
    ip = op = 0
    while ip < in_limit:
        token = src[ip]
        ip += 1
        lit = token >> 4  # :62-77
        if lit == 0xF:
            if ip >= in_limit:
                return malformed(D_LZ4_MALFORMED), ip, b""
            v = src[ip]
            ip += 1
            lit += v
            while v == 255 and ip < in_limit - 15:
                v = src[ip]
                ip += 1
                lit += v
        lit_end, lit_out_limit = ip + lit, op + lit
        if lit_out_limit > fast_out_limit - 4 or lit_end > in_limit - 8:  # :82-96 the last literals
            if lit_out_limit > out_limit:
                return malformed(D_LZ4_LAST_LITERAL_OUTSIDE), ip, b""
            if lit_end != in_limit:
                return malformed(D_LZ4_INPUT_NOT_CONSUMED), ip, b""
            buf += src[ip:lit_end]
            op += lit
            break
        buf += src[ip:lit_end]  # :99-109
        op += lit
        ip = lit_end
        offset = src[ip] | (src[ip + 1] << 8)  # :113-119
        ip += 2
        if offset == 0 or offset > op + history:  # (the reference: offset > op)
            return malformed(D_LZ4_OFFSET_OUTSIDE), ip, b""
        ml = token & 0xF  # :122-138
        if ml == 0xF:
            if ip > in_limit - 5:
                return malformed(D_LZ4_MALFORMED), ip, b""
            v = src[ip]
            ip += 1
            ml += v
            while v == 255:
                if ip > in_limit - 5:
                    return malformed(D_LZ4_MALFORMED), ip, b""
                v = src[ip]
                ip += 1
                ml += v
        ml += 4
        match_out_limit = op + ml
        if match_out_limit > fast_out_limit - 4 and match_out_limit > out_limit - 5:  # :168-171
            return malformed(D_LZ4_LAST_5_LITERALS), ip, b""
        dec._extend(buf, offset, ml)  # :146-194, byte-sequential
        op = match_out_limit
    return 0, 0, bytes(buf[history:])


Header = collections.namedtuple("Header", "linked block_max block_checksum content_size content_checksum expected_size first_block descriptor")


def read_frame_header(data, frame_start, accept_linked):
    """decompressFrame :184-241: the frame header behind the magic at frame_start"""
    n = len(data)
    dstart = frame_start + 4
    if dstart + 2 > n:
        raise _Fail(malformed(D_TRUNC_HEADER), dstart)
    flg, bd = data[dstart], data[dstart + 1]
    version = (flg >> 6) & 3
    if version != 1:
        raise _Fail(malformed({0: D_VERSION_0, 2: D_VERSION_2, 3: D_VERSION_3}[version]), dstart)
    if flg & FLG_RESERVED or bd & BD_RESERVED:
        raise _Fail(malformed(D_RESERVED_BITS), dstart)
    linked = not flg & FLG_INDEPENDENT
    if linked and not accept_linked:
        raise _Fail(malformed(D_LINKED_BLOCKS), dstart)
    if flg & FLG_DICTIONARY:
        raise _Fail(malformed(D_DICTIONARY), dstart)
    size_id = (bd >> 4) & 7
    if size_id < 4:
        raise _Fail(malformed(D_BLOCK_MAX_SIZE), dstart + 1)
    has_size = bool(flg & FLG_CONTENT_SIZE)
    p = dstart + 2
    if p + (8 if has_size else 0) + 1 > n:
        raise _Fail(malformed(D_TRUNC_HEADER), p)
    expected = -1
    if has_size:
        expected = struct.unpack_from("<q", data, p)[0]
        p += 8
    if data[p] != (xxh32(data[dstart:p]) >> 8) & 0xFF:
        raise _Fail(malformed(D_HEADER_CHECKSUM), p)
    return Header(linked, 1 << (8 + 2 * size_id), bool(flg & FLG_BLOCK_CHECKSUM), has_size, bool(flg & FLG_CONTENT_CHECKSUM), expected, p + 1, dstart)


def _decompress_frame(data, cap, out, pos, accept_linked):
    """decompressFrame :184-322: appends the frame's content to `out`, -> the position behind the frame"""
    n = len(data)
    out_start = len(out)
    h = read_frame_header(data, pos, accept_linked)
    p = h.first_block
    while True:
        if p + 4 > n:
            raise _Fail(malformed(D_MISSING_BLOCK_SIZE), p)
        header = struct.unpack_from("<I", data, p)[0]
        p += 4
        if header == 0:
            break
        stored, block_len = bool(header & STORED), header & 0x7FFFFFFF
        if block_len > h.block_max or p + block_len > n:
            raise _Fail(malformed(D_BLOCK_PAST_END), p)
        o = len(out)
        if stored:
            if o + block_len > cap:
                raise _Fail(malformed(D_OUTPUT_TOO_SMALL), o)
            out += data[p:p + block_len]
        else:
            window = bytes(out[max(out_start, o - MAX_DISTANCE):]) if h.linked else b""  # THE rule: this frame's content so far, never more
            st, eo, piece = block_decode(data[p:p + block_len], cap - o, window)
            if st == mk_status(CLASS_OUTPUT_TOO_SMALL, D_LZ4_EMPTY_OUTPUT):  # the block codec returned -1 (:275-277)
                raise _Fail(malformed(D_OUTPUT_TOO_SMALL), o)
            if st != 0:
                raise _Fail(st, eo)  # the block codec's exception, its offset relative to the block
            if len(piece) > h.block_max:
                raise _Fail(malformed(D_BLOCK_EXCEEDS_MAX), p)
            out += piece
        if h.block_checksum:
            cpos = p + block_len
            if cpos + 4 > n:
                raise _Fail(malformed(D_MISSING_BLOCK_CHECKSUM), cpos)
            if struct.unpack_from("<I", data, cpos)[0] != xxh32(data[p:p + block_len]):
                raise _Fail(malformed(D_BLOCK_CHECKSUM), cpos)
        p += block_len + (4 if h.block_checksum else 0)
    content = out[out_start:]
    if h.content_checksum:
        if p + 4 > n:
            raise _Fail(malformed(D_MISSING_CONTENT_CHECKSUM), p)
        if struct.unpack_from("<I", data, p)[0] != xxh32(content):
            raise _Fail(malformed(D_CONTENT_CHECKSUM), p)
        p += 4
    if h.content_size and len(content) != h.expected_size:
        raise _Fail(malformed(D_CONTENT_SIZE), p)
    return p


def decompress(data, cap, accept_linked=False):
    """Lz4FrameCompression.decompress :145-177 over an item (concatenated and skippable frames) -> Result(status, offset, bytes); a failure has no bytes"""
    data = bytes(data)
    n = len(data)
    out = bytearray()
    try:
        if n < HEADER_SIZE:
            raise _Fail(malformed(D_TOO_SHORT), 0)
        pos = 0
        while pos < n:
            if pos + 4 > n:
                raise _Fail(malformed(D_TRUNC_MAGIC), pos)
            magic = struct.unpack_from("<I", data, pos)[0]
            if magic == MAGIC:
                pos = _decompress_frame(data, cap, out, pos, accept_linked)
            elif magic & SKIPPABLE_MASK == SKIPPABLE_MAGIC:  # skipFrame :327-343
                spos = pos + 4
                if spos + 4 > n:
                    raise _Fail(malformed(D_TRUNC_SKIP_SIZE), spos)
                frame_end = spos + 4 + struct.unpack_from("<I", data, spos)[0]
                if frame_end > n:
                    raise _Fail(malformed(D_TRUNC_SKIP), spos)
                pos = frame_end
            else:
                raise _Fail(malformed(D_BAD_MAGIC), pos)
    except _Fail as f:
        return Result(f.status, f.offset, b"")
    return Result(0, 0, bytes(out))


# ---- the walk: structure without content ------------------------------------------------------------------------------------------------------------------------
Seq = collections.namedtuple("Seq", "pos lit ml offset ip")  # pos: where the match is written, relative to its block; ip: behind the offset, relative to the block
WalkedBlock = collections.namedtuple("WalkedBlock", "stored at length start size seqs tail tail_ip")  # at: in the item; start: in the frame's content; size: decoded
WalkedFrame = collections.namedtuple("WalkedFrame", "at flg linked block_max blocks content")


def walk_block(src):
    """-> ([Seq], final literal run, ip behind its token and length bytes, decoded size) of a block that is in order"""
    seqs, ip, op, n = [], 0, 0, len(src)
    while True:
        token = src[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                v = src[ip]
                ip += 1
                lit += v
                if v != 255:
                    break
        if ip + lit == n:
            return seqs, lit, ip, op + lit
        ip += lit
        op += lit
        offset = src[ip] | (src[ip + 1] << 8)
        ip += 2
        at = ip
        ml = token & 15
        if ml == 15:
            while True:
                v = src[ip]
                ip += 1
                ml += v
                if v != 255:
                    break
        ml += 4
        seqs.append(Seq(op, lit, ml, offset, at))
        op += ml


def walk(data):
    """-> [WalkedFrame] of an item whose containers are in order (checksums and offsets are not looked at); skippable frames are passed over"""
    data = bytes(data)
    frames, pos = [], 0
    while pos < len(data):
        magic = struct.unpack_from("<I", data, pos)[0]
        if magic & SKIPPABLE_MASK == SKIPPABLE_MAGIC:
            pos += 8 + struct.unpack_from("<I", data, pos + 4)[0]
            continue
        assert magic == MAGIC, hex(magic)
        flg, bd = data[pos + 4], data[pos + 5]
        p = pos + 6 + (8 if flg & FLG_CONTENT_SIZE else 0) + (4 if flg & FLG_DICTIONARY else 0) + 1
        blocks, content = [], 0
        while True:
            header = struct.unpack_from("<I", data, p)[0]
            p += 4
            if header == 0:
                break
            length = header & 0x7FFFFFFF
            if header & STORED:
                blocks.append(WalkedBlock(True, p, length, content, length, [], 0, 0))
                content += length
            else:
                seqs, tail, tail_ip, size = walk_block(data[p:p + length])
                blocks.append(WalkedBlock(False, p, length, content, size, seqs, tail, tail_ip))
                content += size
            p += length + (4 if flg & FLG_BLOCK_CHECKSUM else 0)
        p += 4 if flg & FLG_CONTENT_CHECKSUM else 0
        frames.append(WalkedFrame(pos, flg, not flg & FLG_INDEPENDENT, 1 << (8 + 2 * ((bd >> 4) & 7)), blocks, content))
        pos = p
    return frames


# ---- writers --------------------------------------------------------------------------------------------------------------------------------------------------
def write_block(seqs, tail):
    """An LZ4 block of sequences (literal bytes, match length >= 4, offset) and a final literal run (bytes)"""
    s = bytearray()
    for lit, ml, off in seqs:
        assert ml >= 4 and 0 <= off <= 0xFFFF
        s.append((min(len(lit), 15) << 4) | min(ml - 4, 15))
        if len(lit) >= 15:
            s += dec._lz4_len(len(lit))
        s += lit
        s += off.to_bytes(2, "little")
        if ml - 4 >= 15:
            s += dec._lz4_len(ml - 4)
    s.append(min(len(tail), 15) << 4)
    if len(tail) >= 15:
        s += dec._lz4_len(len(tail))
    s += tail
    return bytes(s)


def skippable(payload, nibble=0):
    return struct.pack("<II", SKIPPABLE_MAGIC | nibble, len(payload)) + payload


Frame = collections.namedtuple("Frame", "data plain")  # plain: None where a sequence asks for bytes that are not there


class _Filler:
    """non-repeating literal bytes: tests/decoder_edge_cases.py's pool, one cursor per frame"""

    def __init__(self, salt):
        self.cur = salt * 7919

    def take(self, n):
        f = dec._filler(self.cur, n)
        self.cur += n
        return f


def frame(blocks, linked=True, size_id=4, block_checksum=False, content_checksum=False, content_size=None, dictionary=False, salt=0, bad_block_checksum=None,
          bad_content_checksum=False):
    """One LZ4 frame.  blocks: ("seqs", [(literal length, match length, offset), ...], final literals) -- written as given, the literals filler; ("stored", n)
    -- n filler bytes, stored; ("raw", [(literal bytes, match length, offset), ...], final literal bytes) -- an encoder's sequences.  An offset may reach into
    the blocks in front (linked frames) -- or past everything there is: the plaintext is then None.  content_size: None = not announced, True = the right one,
    a number = that.  bad_block_checksum: the index of the block whose checksum is written wrong."""
    fill = _Filler(salt)
    plain, ok = bytearray(), True
    body = bytearray()
    for k, b in enumerate(blocks):
        start = len(plain)
        if b[0] == "stored":
            block = fill.take(b[1])
            plain += block
            header = len(block) | STORED
        else:
            seqs = [(fill.take(lit), ml, off) for lit, ml, off in b[1]] if b[0] == "seqs" else b[1]
            tail = fill.take(b[2]) if b[0] == "seqs" else b[2]
            for lit, ml, off in seqs:
                plain += lit
                reach = len(plain) if linked else len(plain) - start
                if ok and 1 <= off <= min(reach, MAX_DISTANCE):
                    dec._extend(plain, off, ml)
                else:
                    ok = False
            plain += tail
            block = write_block(seqs, tail)
            header = len(block)
        assert len(plain) - start <= 1 << (8 + 2 * size_id) and len(block) <= 1 << (8 + 2 * size_id)
        body += struct.pack("<I", header) + block
        if block_checksum:
            body += struct.pack("<I", xxh32(block) ^ (0x5A if bad_block_checksum == k else 0))
    body += struct.pack("<I", 0)
    if content_checksum:
        body += struct.pack("<I", xxh32(plain) ^ (0x5A if bad_content_checksum else 0))
    flg = FLG_VERSION | (0 if linked else FLG_INDEPENDENT) | (FLG_BLOCK_CHECKSUM if block_checksum else 0) | (FLG_CONTENT_CHECKSUM if content_checksum else 0)
    flg |= (FLG_CONTENT_SIZE if content_size is not None else 0) | (FLG_DICTIONARY if dictionary else 0)
    desc = bytearray([flg, size_id << 4])
    if content_size is not None:
        desc += struct.pack("<q", len(plain) if content_size is True else content_size)
    if dictionary:
        desc += struct.pack("<I", 0x12345678)
    head = struct.pack("<I", MAGIC) + desc + bytes([(xxh32(desc) >> 8) & 0xFF])
    return Frame(bytes(head + body), bytes(plain) if ok else None)


def greedy_blocks(content, block_size, linked=True):
    """-> [("raw", sequences, final literals)] for frame(): a greedy LZ4 encoding of `content` in blocks of block_size.  One hash table (4 bytes -> the last
    position that held them) over the whole content; a candidate counts when it is at most 65 535 bytes back and -- linked=False -- not in front of its block."""
    content = bytes(content)
    table, blocks = {}, []
    for start in range(0, len(content), block_size):
        end = min(start + block_size, len(content))
        match_start_limit, match_end_limit = end - 12, end - 5  # no match starts in the last 12 bytes; the last 5 are literals
        seqs, anchor, i = [], start, start
        while i < match_start_limit:
            key = content[i:i + 4]
            cand = table.get(key)
            table[key] = i
            if cand is not None and i - cand <= MAX_DISTANCE and (linked or cand >= start):
                ml = 4
                while i + ml < match_end_limit and content[cand + ml] == content[i + ml]:
                    ml += 1
                seqs.append((content[anchor:i], ml, i - cand))
                i += ml
                anchor = i
            else:
                i += 1
        blocks.append(("raw", seqs, content[anchor:end]))
    return blocks
