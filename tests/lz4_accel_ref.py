"""A pure-Python LZ4 block encoder with the acceleration parameter of Lz4Compressor.create(int), for the tests: the GPU encoders are checked against it at
accelerations the oracle (which restates the Java encoder, acceleration 1 only) does not have.

The definition: M/lz4/Lz4RawCompressor.java:69-192 with ONE line changed -- :115 `int findMatchAttempts = 1 << SKIP_TRIGGER` becomes
`acceleration << SKIP_TRIGGER`, liblz4's rule (LZ4_compress_generic: searchMatchNb = acceleration << LZ4_skipTrigger).  `step` still starts at 1, so a search
that starts at s probes s, s + 1, s + 1 + a, s + 1 + 2a, ...; the advance grows by 1 every 64 probes.  Everything else -- the re-probe behind a match, the
`input - 2` insert, the catch-up, count, the end-of-block rules, maxCompressedLength -- is the Java encoder's.

At acceleration 1 the output is the oracle's, byte for byte (tests/test_lz4_accel_ref.py); the other accelerations are pinned by tests/golden/lz4_accel_vectors.json
(tools/record_lz4_accel_vectors.py).  compress_frame() is Lz4FrameCompression.compress (M/lz4/Lz4FrameCompression.java:96-140) over this encoder.
Hashes and 4-byte words of every position come from numpy, the parse itself is a plain loop: 64 KiB of text take about 0.1 s.
"""
import struct

import numpy as np

HASH_LOG = 12
MIN_TABLE_SIZE = 16
MAX_TABLE_SIZE = 1 << HASH_LOG
MIN_MATCH = 4
LAST_LITERAL_SIZE = 5
MATCH_FIND_LIMIT = 12
MIN_LENGTH = 13
ML_MASK = 15
RUN_MASK = 15
MAX_DISTANCE = 65535
SKIP_TRIGGER = 6
MAX_INPUT_SIZE = 0x7E000000
MIN_ACCELERATION, MAX_ACCELERATION = 1, 65537  # M/lz4/Lz4Native.java:49-50

FRAME_MAGIC = 0x184D2204
FRAME_BLOCK_MAX = 4 << 20
FRAME_UNCOMPRESSED = 0x80000000


def check_acceleration(acceleration):
    if not MIN_ACCELERATION <= acceleration <= MAX_ACCELERATION:
        raise ValueError("LZ4 acceleration should be in the [1, 65537] range but got %d" % acceleration)


def max_compressed_length(n):
    return n + n // 255 + 16


def table_size(n):
    target = 0 if n <= 1 else 1 << (n - 1).bit_length()
    return min(max(target, MIN_TABLE_SIZE), MAX_TABLE_SIZE)


# ---- the probe schedule of one search, in closed form (what the batch-probe kernels compute per lane) --------------------------------------------------------
def scan_advance(k, a):
    """the advance behind probe k of a search: `step` as the loop leaves it after k + 1 passes"""
    return 1 if k == 0 else (64 * a + k - 1) >> 6


def _S(x):
    """sum of t >> 6 over 0 <= t <= x"""
    if x < 0:
        return 0
    q, r = divmod(x + 1, 64)
    return 32 * q * (q - 1) + q * r


def scan_offset(m, a):
    """the distance of probe m from the search's start: the sum of the first m advances"""
    return 0 if m == 0 else 1 + _S(64 * a + m - 2) - _S(64 * a - 1)


def probe_pattern(a):
    """the probes of a search as a mask of the 64 positions from its start on: bit 0, and the bits 1 + j * a (lz4_compress_mw.h: P_a)"""
    p = 1
    for bit in range(1, 64, a):
        p |= 1 << bit
    return p


# ---- the encoder ------------------------------------------------------------------------------------------------------------------------------------------
def _count(data, a, b, limit):
    """bytes data[a:] and data[b:] have in common, a never beyond `limit` (count :240-267)"""
    n = limit - a
    done = 0
    chunk = 16
    while done < n:
        c = min(chunk, n - done)
        if data[a + done:a + done + c] == data[b + done:b + done + c]:
            done += c
            chunk = min(chunk * 4, 1 << 20)
            continue
        while c > 1:  # the first difference lies in these c bytes
            half = c // 2
            if data[a + done:a + done + half] == data[b + done:b + done + half]:
                done += half
                c -= half
            else:
                c = half
        return done
    return n


def _run_length(out, length, low=0):
    if length >= RUN_MASK:
        out.append((RUN_MASK << 4) | low)
        remaining = length - RUN_MASK
        while remaining >= 255:
            out.append(255)
            remaining -= 255
        out.append(remaining)
    else:
        out.append((length << 4) | low)


def compress(data, acceleration=1, trace=None):
    """-> the block as bytes.  trace: a list that receives (start, candidate, catch-up bytes, length) of every match (for the tests that build inputs)"""
    check_acceleration(acceleration)
    data = bytes(data)
    n = len(data)
    if n > MAX_INPUT_SIZE:
        raise ValueError("Max input length exceeded")
    out = bytearray()
    anchor = 0
    if n >= MIN_LENGTH:
        mask = table_size(n) - 1
        padded = np.zeros(n + 8, dtype=np.uint8)
        padded[:n] = np.frombuffer(data, dtype=np.uint8)
        words = np.zeros(n, dtype=np.uint64)
        for i in range(8):
            words |= padded[i:i + n].astype(np.uint64) << np.uint64(8 * i)
        hashes = (((words * np.uint64(889523592379)) >> np.uint64(28)) & np.uint64(mask)).astype(np.int64).tolist()
        four = (words & np.uint64(0xFFFFFFFF)).astype(np.int64).tolist()
        table = [0] * (mask + 1)
        match_find_limit = n - MATCH_FIND_LIMIT
        match_limit = n - LAST_LITERAL_SIZE

        table[hashes[0]] = 0
        pos = 1
        done = False
        while not done:
            # the search :113-138
            next_index = pos
            attempts = acceleration << SKIP_TRIGGER  # (:115, the one changed line)
            step = 1
            while True:
                pos = next_index
                next_index += step
                step = attempts >> SKIP_TRIGGER
                attempts += 1
                if next_index > match_find_limit:
                    done = True
                    break
                h = hashes[pos]
                match = table[h]
                table[h] = pos
                if four[match] == four[pos] and match + MAX_DISTANCE >= pos:
                    break
            if done:
                break
            found = pos
            while pos > anchor and match > 0 and data[pos - 1] == data[match - 1]:  # catch up :141-144
                pos -= 1
                match -= 1
            back = found - pos
            literals = pos - anchor
            token = len(out)
            _run_length(out, literals)
            out += data[anchor:pos]
            while True:  # :147-184
                length = _count(data, pos + MIN_MATCH, match + MIN_MATCH, match_limit)
                offset = pos - match
                if trace is not None:
                    trace.append((pos, match, back, length + MIN_MATCH))
                back = 0
                out.append(offset & 255)
                out.append(offset >> 8)
                if length >= ML_MASK:
                    out[token] |= ML_MASK
                    remaining = length - ML_MASK
                    while remaining >= 510:
                        out.append(255)
                        out.append(255)
                        remaining -= 510
                    if remaining >= 255:
                        out.append(255)
                        remaining -= 255
                    out.append(remaining)
                else:
                    out[token] |= length
                pos += length + MIN_MATCH
                anchor = pos
                if pos > match_find_limit:
                    done = True
                    break
                table[hashes[pos - 2]] = pos - 2
                h = hashes[pos]
                match = table[h]
                table[h] = pos
                if match + MAX_DISTANCE < pos or four[match] != four[pos]:
                    pos += 1
                    break
                token = len(out)
                out.append(0)
    _run_length(out, n - anchor)  # emitLastLiteral :269-280
    out += data[anchor:]
    return bytes(out)


def compress_frame(data, acceleration=1):
    """Lz4FrameCompression.compress :96-140 over compress(): header, 4 MiB blocks (stored when the encoder does not make them smaller), end mark"""
    data = bytes(data)
    out = bytearray(struct.pack("<I", FRAME_MAGIC))
    out += bytes([0x60, 0x70, 0x73])  # FLG (version 01, independent blocks), BD (4 MiB), (xxHash32 of the two >> 8) & 0xFF
    for at in range(0, len(data), FRAME_BLOCK_MAX):
        block = data[at:at + FRAME_BLOCK_MAX]
        c = compress(block, acceleration)
        if len(c) < len(block):
            out += struct.pack("<I", len(c)) + c
        else:
            out += struct.pack("<I", len(block) | FRAME_UNCOMPRESSED) + block
    out += struct.pack("<I", 0)
    return bytes(out)
