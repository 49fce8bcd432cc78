"""An LZ4 frame writer with the whole frame descriptor, in plain Python: the reference of the tests at the settings of achip_ctx_set_lz4frame_writer, which the
oracle's writer does not have (it restates Lz4FrameCompression.compress, frozen at FLG 0x60 / BD 0x70).  The framing follows the LZ4 frame format: magic, FLG =
0x60 | blockChecksum << 4 | contentSize << 3 | contentChecksum << 2 (version 01, independent blocks), BD = id << 4, the 8-byte content size, the header
checksum byte (XXH32 of the descriptor >> 8); per block of at most the block-maximum size its size field, its data -- the block encoder's bytes for that block
alone, or the block itself with the size field's high bit set when those are not fewer (M/lz4/Lz4FrameCompression.java:114-126) -- and XXH32 of the data as
stored; the end mark; XXH32 of the content.  Blocks: the oracle's LZ4 block encoder at acceleration 1, tests/lz4_accel_ref.compress above.  At (4 MiB, 0, 0, 0)
the bytes are the oracle's frame writer's (tests/test_lz4f_writer_ref.py)."""
import collections
import struct

from tests import lz4_accel_ref, oracle_lib
from tests.lz4_linked_ref import xxh32

MAGIC = 0x184D2204
STORED = 0x80000000
BLOCK_SIZES = (65536, 262144, 1048576, 4194304)  # BD ids 4 .. 7
DEFAULT = (4194304, 0, 0, 0)  # (block size, block checksum, content checksum, content size): the Java writer's frame
REFUSALS = ("blockMaxSize must be 65536, 262144, 1048576 or 4194304", "blockChecksum must be 0 or 1", "contentChecksum must be 0 or 1", "contentSize must be 0 or 1")


def check_arguments(block_size, block_checksum, content_checksum, content_size):
    """the setter's checks, in the order of its arguments: -> the refusal's text, or None"""
    if block_size not in BLOCK_SIZES:
        return REFUSALS[0]
    for text, flag in zip(REFUSALS[1:], (block_checksum, content_checksum, content_size)):
        if flag not in (0, 1):
            return text
    return None


def lz4_bound(n):
    return n + n // 255 + 16


def max_compressed_length(n, block_size, block_checksum, content_checksum, content_size):
    """what the block-list writer asks of its destination: the worst-case places of the frame's blocks"""
    each = 4 + 4 * block_checksum
    rest = n % block_size
    return 7 + 8 * content_size + (n // block_size) * (each + lz4_bound(block_size)) + (each + lz4_bound(rest) if rest else 0) + 4 + 4 * content_checksum


def header(n, block_size, block_checksum, content_checksum, content_size):
    descriptor = bytes([0x60 | block_checksum << 4 | content_size << 3 | content_checksum << 2, (4 + BLOCK_SIZES.index(block_size)) << 4])
    if content_size:
        descriptor += struct.pack("<Q", n)
    return struct.pack("<I", MAGIC) + descriptor + bytes([(xxh32(descriptor) >> 8) & 0xFF])


def encode_block(block, acceleration=1, oracle=None):
    if acceleration == 1:
        return (oracle if oracle is not None else oracle_lib.load()).compress("lz4", block)
    return lz4_accel_ref.compress(block, acceleration)


def compress(data, block_size=4194304, block_checksum=0, content_checksum=0, content_size=0, acceleration=1, oracle=None):
    assert check_arguments(block_size, block_checksum, content_checksum, content_size) is None
    data = bytes(data)
    out = bytearray(header(len(data), block_size, block_checksum, content_checksum, content_size))
    for at in range(0, len(data), block_size):
        block = data[at:at + block_size]
        encoded = encode_block(block, acceleration, oracle)
        if len(encoded) < len(block):
            out += struct.pack("<I", len(encoded)) + encoded
            stored = encoded
        else:
            out += struct.pack("<I", len(block) | STORED) + block
            stored = block
        if block_checksum:
            out += struct.pack("<I", xxh32(stored))
    out += struct.pack("<I", 0)
    if content_checksum:
        out += struct.pack("<I", xxh32(data))
    return bytes(out)


Block = collections.namedtuple("Block", "at stored data checksum")  # at: of the size field; checksum: the field, or None
Parsed = collections.namedtuple("Parsed", "flg block_size content_size blocks content_checksum length")


def parse(frame):
    """The structure of ONE well-formed frame of independent blocks that fills `frame`, read field by field (no decoding, no checksum verified -- the oracle's
    reader does both in tests/test_lz4f_writer_ref.py): what the catalog's labels are proved from."""
    assert struct.unpack_from("<I", frame, 0)[0] == MAGIC
    flg, bd = frame[4], frame[5]
    assert flg & 0xE3 == 0x60 and bd & 0x8F == 0 and 4 <= bd >> 4 <= 7, (flg, bd)
    pos = 6
    content_size = None
    if flg & 0x08:
        content_size = struct.unpack_from("<Q", frame, pos)[0]
        pos += 8
    assert frame[pos] == (xxh32(frame[4:pos]) >> 8) & 0xFF, "header checksum"
    pos += 1
    blocks = []
    while True:
        field = struct.unpack_from("<I", frame, pos)[0]
        if field == 0:
            pos += 4
            break
        size = field & ~STORED
        data = frame[pos + 4:pos + 4 + size]
        assert len(data) == size
        checksum = struct.unpack_from("<I", frame, pos + 4 + size)[0] if flg & 0x10 else None
        blocks.append(Block(pos, bool(field & STORED), data, checksum))
        pos += 4 + size + (4 if flg & 0x10 else 0)
    content_checksum = None
    if flg & 0x04:
        content_checksum = struct.unpack_from("<I", frame, pos)[0]
        pos += 4
    assert pos == len(frame), "bytes behind the frame"
    return Parsed(flg, BLOCK_SIZES[(bd >> 4) - 4], content_size, blocks, content_checksum, pos)
