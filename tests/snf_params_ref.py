"""SnappyFramedOutputStream with its five-argument constructor, and a reader of the framing format, in plain Python: the reference of the tests at parameters the
oracle's one-shot writer does not have (it is frozen at the defaults).  The writer is the loop of M/snappy/SnappyFramedOutputStream.java:107-141 (write: the
partial buffer, full blocks straight from the input, the rest into the buffer), :180-187 (flushBuffer) and :199-255 (writeCompressed, writeBlock) over the oracle's
raw Snappy block encoder and CRC-32C; the reader follows the format (stream identifier, compressed / uncompressed data chunks, skippable chunks).  Python's float
is the Java double: `compressed / length <= min_compression_ratio` is the same correctly rounded division and comparison."""
import struct

from tests import oracle_lib

HEADER = bytes([0xFF, 0x06, 0x00, 0x00, 0x73, 0x4E, 0x61, 0x50, 0x70, 0x59])  # SnappyFramed.HEADER_BYTES
COMPRESSED_DATA_FLAG, UNCOMPRESSED_DATA_FLAG, STREAM_IDENTIFIER_FLAG = 0x00, 0x01, 0xFF
MAX_BLOCK_SIZE = DEFAULT_BLOCK_SIZE = 65536
DEFAULT_MIN_COMPRESSION_RATIO = 0.85
DEFAULT_PARAMS = (True, DEFAULT_BLOCK_SIZE, DEFAULT_MIN_COMPRESSION_RATIO)
SMALLEST_RATIO = 5e-324  # Double.MIN_VALUE: nothing compresses that well, every chunk is stored raw


def ratio_bits(ratio):
    """Double.doubleToRawLongBits"""
    return struct.unpack("<q", struct.pack("<d", ratio))[0]


def check_arguments(block_size, min_compression_ratio):
    # the constructor :83, :90 -- the ratio first
    if not (min_compression_ratio > 0 and min_compression_ratio <= 1.0):
        raise ValueError("minCompressionRatio %s must be between (0,1.0]." % ("NaN" if min_compression_ratio != min_compression_ratio else repr(float(min_compression_ratio))))
    if not 0 < block_size <= MAX_BLOCK_SIZE:
        raise ValueError("blockSize must be in (0, 65536]")


def max_compressed_length(n, block_size=DEFAULT_BLOCK_SIZE):
    """what the one-shot form asks of its destination: the stream header, and per block a chunk header, the CRC field and at most the block itself"""
    return 10 + 8 * ((n + block_size - 1) // block_size) + n


class Writer:
    """SnappyFramedOutputStream(compressor, out, writeChecksums, blockSize, minCompressionRatio)"""

    def __init__(self, write_checksums=True, block_size=DEFAULT_BLOCK_SIZE, min_compression_ratio=DEFAULT_MIN_COMPRESSION_RATIO, oracle=None, trace=None):
        check_arguments(block_size, min_compression_ratio)
        self.o = oracle if oracle is not None else oracle_lib.load()
        self.write_checksums, self.block_size, self.min_compression_ratio = write_checksums, block_size, min_compression_ratio
        self.buffer = bytearray()
        self.out = bytearray(HEADER)
        self.trace = trace  # [(length, compressed, kept)] per chunk, for the tests that build inputs at the ratio's edge

    def write(self, data):  # :107-141
        offset, length = 0, len(data)
        free = self.block_size - len(self.buffer)
        if free >= length:
            self.buffer += data
            return
        if len(self.buffer) > 0:
            self.buffer += data[:free]
            self._flush_buffer()
            offset += free
            length -= free
        while length >= self.block_size:
            self._write_compressed(data[offset:offset + self.block_size])
            offset += self.block_size
            length -= self.block_size
        self.buffer += data[offset:offset + length]

    def _flush_buffer(self):  # :180-187
        if len(self.buffer) > 0:
            self._write_compressed(bytes(self.buffer))
            self.buffer = bytearray()

    def _write_compressed(self, block):  # :199-220
        crc = self.o.crc32c(block, masked=True) if self.write_checksums else 0
        compressed = self.o.compress("snappy", block)
        keep = (float(len(compressed)) / float(len(block))) <= self.min_compression_ratio
        if self.trace is not None:
            self.trace.append((len(block), len(compressed), keep))
        self._write_block(compressed if keep else block, keep, crc)

    def _write_block(self, data, compressed, crc):  # :234-255
        header_length = len(data) + 4
        self.out += bytes([COMPRESSED_DATA_FLAG if compressed else UNCOMPRESSED_DATA_FLAG, header_length & 0xFF, (header_length >> 8) & 0xFF, (header_length >> 16) & 0xFF])
        self.out += struct.pack("<I", crc & 0xFFFFFFFF)
        self.out += data

    def close(self):
        self._flush_buffer()
        return bytes(self.out)


def compress(data, write_checksums=True, block_size=DEFAULT_BLOCK_SIZE, min_compression_ratio=DEFAULT_MIN_COMPRESSION_RATIO, oracle=None, trace=None, pieces=None):
    """new SnappyFramedOutputStream(...); write(data) -- or write(piece) for every length in `pieces`, then the rest --; close()"""
    w = Writer(write_checksums, block_size, min_compression_ratio, oracle, trace)
    at = 0
    for n in pieces or ():
        w.write(data[at:at + n])
        at += n
    w.write(data[at:])
    return w.close()


def chunks(stream):
    """[(position, flag, crc field, body)] of the data chunks of a well-formed stream"""
    assert stream[:10] == HEADER, "stream identifier"
    pos, out = 10, []
    while pos < len(stream):
        flag = stream[pos]
        length = stream[pos + 1] | (stream[pos + 2] << 8) | (stream[pos + 3] << 16)
        body = stream[pos + 4:pos + 4 + length]
        assert len(body) == length, "chunk at %d runs past the end" % pos
        if flag in (COMPRESSED_DATA_FLAG, UNCOMPRESSED_DATA_FLAG):
            assert length >= 5, "data chunk at %d too short" % pos
            out.append((pos, flag, struct.unpack("<I", body[:4])[0], body[4:]))
        elif flag == STREAM_IDENTIFIER_FLAG:
            assert body == HEADER[4:], "stream identifier at %d" % pos
        else:
            assert flag >= 0x80, "unskippable chunk %02x at %d" % (flag, pos)
        pos += 4 + length
    return out


class ChecksumError(Exception):
    def __init__(self, position):
        super().__init__("Corrupt input: invalid checksum (chunk at %d)" % position)
        self.position = position


def decompress(stream, verify_checksums=True, oracle=None, plain_lengths=None):
    """SnappyFramedInputStream(decompressor, in, verifyChecksums) read to the end; plain_lengths: a list that receives every data chunk's plaintext length"""
    o = oracle if oracle is not None else oracle_lib.load()
    out = bytearray()
    for position, flag, crc, body in chunks(stream):
        plain = o.decompress("snappy", body, MAX_BLOCK_SIZE) if flag == COMPRESSED_DATA_FLAG else body
        if verify_checksums and crc != o.crc32c(plain, masked=True):
            raise ChecksumError(position)
        if plain_lengths is not None:
            plain_lengths.append(len(plain))
        out += plain
    return bytes(out)
