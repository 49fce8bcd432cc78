"""LZO1X block codec, restated check by check from the reference's two Java files (pure Python, no ctypes, no numpy in the loops):

    D = M/lzo/LzoRawDecompressor.java     decompress(), decoded_size()
    C = M/lzo/LzoRawCompressor.java       compress(), max_compressed_length()
    (M/ = src/main/java/io/airlift/compress/v3/ of airlift/aircompressor)

The decoder raises Malformed(offset) with the Java `input - inputAddress` of the throw; every failure of that decoder, "output too small"
included, is a MalformedInputException.  The encoder's integer arithmetic is the Java's: the hash multiplies in 64 bits and wraps.
"""

MASK64 = (1 << 64) - 1
INT_MAX = 0x7FFFFFFF


class Malformed(Exception):
    def __init__(self, offset):
        Exception.__init__(self, "Malformed input: offset=%d" % offset)
        self.offset = offset


def _i32(v):
    """a Java int after an addition that may wrap"""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def _walk(data, capacity, out, trace=None):
    """D:41-351.  `out`: a bytearray that receives the plaintext, or None (lengths only); `trace`: a list that receives (match length, match offset,
    literal length) per command and None per end marker.  Returns the decoded length."""
    n = len(data)
    if n == 0:  # D:42-44 nothing compresses to nothing
        return 0
    ip = 0
    op = 0
    while ip < n:  # D:52
        first = True
        last_lit = 0
        while True:
            if ip >= n:  # D:56-58
                raise Malformed(ip)
            command = data[ip]
            ip += 1
            if (command & 0xF0) == 0:
                if last_lit == 0:  # D:73-98 a literal run of 4 or more
                    ml = 0
                    off = 0
                    lit = command & 0xF
                    if lit == 0:
                        lit = 0xF
                        nb = 0
                        while ip < n:  # D:92 (input < inputLimit && (nextByte = ...) == 0)
                            nb = data[ip]
                            ip += 1
                            if nb != 0:
                                break
                            lit = _i32(lit + 0xFF)
                        lit = _i32(lit + nb)
                    lit = _i32(lit + 3)
                elif last_lit <= 3:  # D:99-120 a 2-byte match within 1 KiB
                    ml = 2
                    if ip >= n:  # D:111-113
                        raise Malformed(ip)
                    off = (command & 0xC) >> 2
                    off |= data[ip] << 2
                    ip += 1
                    lit = command & 3
                else:  # D:121-142 a 3-byte match at 2049..3072
                    ml = 3
                    if ip >= n:  # D:132-134
                        raise Malformed(ip)
                    off = (command & 0xC) >> 2
                    off |= data[ip] << 2
                    ip += 1
                    off |= 0x800
                    lit = command & 3
            elif first:  # D:144-149
                ml = 0
                off = 0
                lit = command - 17
            elif (command & 0xF0) == 0x10:  # D:150-189
                ml = command & 7
                if ml == 0:
                    ml = 7
                    nb = 0
                    while ip < n:  # D:160
                        nb = data[ip]
                        ip += 1
                        if nb != 0:
                            break
                        ml = _i32(ml + 0xFF)
                    ml = _i32(ml + nb)
                ml = _i32(ml + 2)
                if ip + 2 > n:  # D:168-170
                    raise Malformed(ip)
                trailer = data[ip] | (data[ip + 1] << 8)
                ip += 2
                off = (command & 8) << 11
                off += trailer >> 2
                if off == 0:  # D:180-183 the end marker (the trailer's low bits are not looked at)
                    if trace is not None:
                        trace.append(None)
                    break
                off += 0x3FFF
                lit = trailer & 3
            elif (command & 0xE0) == 0x20:  # D:190-222
                ml = command & 0x1F
                if ml == 0:
                    ml = 0x1F
                    nb = 0
                    while ip < n:  # D:201
                        nb = data[ip]
                        ip += 1
                        if nb != 0:
                            break
                        ml = _i32(ml + 0xFF)
                    ml = _i32(ml + nb)
                ml = _i32(ml + 2)
                if ip + 2 > n:  # D:209-211
                    raise Malformed(ip)
                trailer = data[ip] | (data[ip + 1] << 8)
                ip += 2
                off = trailer >> 2
                lit = trailer & 3
            else:  # D:223-244 ((command & 0xC0) != 0 holds for every byte that comes here: D:245-248 cannot be reached)
                ml = ((command & 0xE0) >> 5) + 1
                if ip >= n:  # D:235-237
                    raise Malformed(ip)
                off = (command & 0x1C) >> 2
                off |= data[ip] << 3
                ip += 1
                lit = command & 3
            first = False
            if trace is not None:
                trace.append((ml, off + 1 if ml else 0, lit))
            if ml < 0:  # D:251-253
                raise Malformed(ip)
            if ml != 0:  # D:256-320
                off += 1
                if op - off < 0 or op + ml > capacity:  # D:261-263 (and :297-299)
                    raise Malformed(ip)
                if out is not None:
                    start = op - off
                    if off >= ml:
                        out += out[start:start + ml]
                    else:
                        for k in range(ml):
                            out.append(out[start + k])
                op += ml
            if lit < 0:  # D:323-325
                raise Malformed(ip)
            if op + lit > capacity or ip + lit > n:  # D:327-330
                raise Malformed(ip)
            if out is not None:
                out += data[ip:ip + lit]
            ip += lit
            op += lit
            last_lit = lit  # D:348
    return op


def decompress(data, capacity):
    """LzoRawDecompressor.decompress into a buffer of `capacity` bytes: the plaintext, or Malformed(offset)"""
    out = bytearray()
    n = _walk(bytes(data), capacity, out)
    assert n == len(out)
    return bytes(out)


def decoded_size(data):
    """what `data` decodes to with room to spare (capacity INT32_MAX), without the bytes; Malformed(offset) as the decoder"""
    return _walk(bytes(data), INT_MAX, None)


def commands(data):
    """the commands of a valid stream: (match length, match offset, literal length) each, None for an end marker"""
    trace = []
    _walk(bytes(data), INT_MAX, None, trace)
    return trace


# ---- encoder ----
LAST_LITERAL_SIZE = 5
MIN_MATCH = 4
MAX_INPUT_SIZE = 0x7E000000
HASH_LOG = 12
MIN_TABLE_SIZE = 16
MAX_TABLE_SIZE = 1 << HASH_LOG
MATCH_FIND_LIMIT = 8 + MIN_MATCH
MIN_LENGTH = MATCH_FIND_LIMIT + 1
RUN_MASK = 15
MAX_DISTANCE = 0xC000 - 1
SKIP_TRIGGER = 6


def max_compressed_length(n):  # C:65-68 (Java ints: the division truncates toward zero, the sum wraps)
    q = abs(n) // 255
    return _i32(n + (q if n >= 0 else -q) + 16)


def compute_table_size(n):  # C:382-389
    v = (n - 1) & 0xFFFFFFFF
    hob = 0 if v == 0 else 1 << (v.bit_length() - 1)
    target = _i32(hob << 1)
    return max(MIN_TABLE_SIZE, min(target, MAX_TABLE_SIZE))


def _hash(value, mask):  # C:51-63
    return (((value * 889523592379) & MASK64) >> 28) & mask


def _encode_literal_length(first, out, length):  # C:278-309
    if first and length < 0xFF - 17:
        out.append(length + 17)
    elif length < 4:
        out[-2] |= length  # the low bits of the previous command's little-endian trailer
    else:
        length -= 3
        if length > RUN_MASK:
            out.append(0)
            remaining = length - RUN_MASK
            while remaining > 255:
                out.append(0)
                remaining -= 255
            out.append(remaining)
        else:
            out.append(length)


def _emit_last_literal(first, out, data, anchor):  # C:236-255
    _encode_literal_length(first, out, len(data) - anchor)
    out += data[anchor:]
    out += b"\x11\x00\x00"


def _encode_match_length(out, ml, base, command):  # C:360-380
    if ml <= base:
        out.append(command | ml)
    else:
        out.append(command)
        remaining = ml - base
        while remaining > 510:
            out += b"\x00\x00"
            remaining -= 510
        if remaining > 255:
            out.append(0)
            remaining -= 255
        out.append(remaining)


def _emit_copy(out, off, ml):  # C:311-352
    assert 1 <= off <= MAX_DISTANCE, off
    if ml <= 8 and off <= 2048:
        ml -= 1
        off -= 1
        out.append((ml << 5) | ((off & 7) << 2))
        out.append(off >> 3)
        return
    ml -= 2
    if off >= 1 << 15:
        _encode_match_length(out, ml, 7, 0x18)
    elif off > 1 << 14:
        _encode_match_length(out, ml, 7, 0x10)
    else:
        _encode_match_length(out, ml, 31, 0x20)
        off -= 1
    v = (off << 2) & 0xFFFF  # C:354-358 (short)
    out.append(v & 0xFF)
    out.append(v >> 8)


def _count(data, start, match, limit):  # C:203-234: the common prefix, capped at the limit
    cur = start
    while cur < limit and data[match] == data[cur]:
        cur += 1
        match += 1
    return cur - start


class IllegalArgument(Exception):
    pass


def compress(data, max_output=None):
    """LzoRawCompressor.compress: the compressed bytes (max_output: the room; None = max_compressed_length)"""
    data = bytes(data)
    n = len(data)
    if n > MAX_INPUT_SIZE:  # C:84-86
        raise IllegalArgument("Max input length exceeded")
    if max_output is not None and max_output < max_compressed_length(n):  # C:88-90
        raise IllegalArgument("Max output length must be larger than %d" % max_compressed_length(n))
    if n == 0:  # C:93-95
        return b""
    out = bytearray()
    if n < MIN_LENGTH:  # C:104-107
        _emit_last_literal(True, out, data, 0)
        return bytes(out)
    size = compute_table_size(n)
    mask = size - 1
    table = [0] * size
    # 8 bytes at position p (positions the search loads from always have 8 bytes: p <= n - 12 + ...); padded for the last ones
    padded = data + bytes(8)

    def ld8(p):
        return int.from_bytes(padded[p:p + 8], "little")

    def ld4(p):
        return padded[p:p + 4]

    match_find_limit = n - MATCH_FIND_LIMIT
    match_limit = n - LAST_LITERAL_SIZE
    ip = 0
    anchor = 0
    table[_hash(ld8(ip), mask)] = ip  # C:113
    ip += 1
    next_hash = _hash(ld8(ip), mask)
    done = False
    first = True
    while not done:  # C:120-195
        next_ip = ip
        attempts = 1 << SKIP_TRIGGER
        step = 1
        while True:  # C:127-146
            h = next_hash
            ip = next_ip
            next_ip += step
            step = attempts >> SKIP_TRIGGER
            attempts += 1
            if next_ip > match_find_limit:  # C:134-137
                _emit_last_literal(first, out, data, anchor)
                return bytes(out)
            match = table[h]
            next_hash = _hash(ld8(next_ip), mask)
            table[h] = ip
            if ld4(match) == ld4(ip) and match + MAX_DISTANCE >= ip:
                break
        while ip > anchor and match > 0 and data[ip - 1] == data[match - 1]:  # C:149-152
            ip -= 1
            match -= 1
        lit = ip - anchor
        _encode_literal_length(first, out, lit)  # C:156, emitLiteral C:257-276
        out += data[anchor:ip]
        first = False
        while True:  # C:160-193
            off = ip - match
            ip += MIN_MATCH
            ml = _count(data, ip, match + MIN_MATCH, match_limit)
            ip += ml
            _emit_copy(out, off, ml + MIN_MATCH)
            anchor = ip
            if ip > match_find_limit:  # C:173-176
                done = True
                break
            pos = ip - 2
            table[_hash(ld8(pos), mask)] = pos
            h = _hash(ld8(ip), mask)
            match = table[h]
            table[h] = ip
            if match + MAX_DISTANCE < ip or ld4(match) != ld4(ip):  # C:186-190
                ip += 1
                next_hash = _hash(ld8(ip), mask)
                break
    _emit_last_literal(False, out, data, anchor)  # C:198
    return bytes(out)
