"""The inputs and parameter sets of the x-snappy-framed parameter tests (tests/test_gpu_snf_params.py, tools/hostemu/check_snf_params.py,
tools/record_snf_params_vectors.py): the smallest shapes at which each mechanism can go wrong, built once.  Expected bytes come from tests/snf_params_ref.py.

  block sizes   1, 2 (a block below every vector width), 63, 64 (one lane each / the wavefront's width), 4096, 65535, 65536 (the largest; one below it)
  lengths       per block size B: 0, 1, B - 1, B, B + 1, 3B + 7 -- no block, a partial one, a full one, a full one and a byte, several and a rest
  data          text-like (kept compressed at 0.85), random (stored raw at every ratio), a run of one byte (kept at every ratio but the smallest)
  ratios        1.0, 0.85, 0.5, the smallest positive double (everything stored raw), and constructed pairs: a block the oracle compresses from l to c bytes is
                kept at the ratio c / l and stored raw at the next double below it -- the device's division held to Java's
  checksums     written, and not
"""
import functools
import math

import numpy as np

from tests import common, oracle_lib, snf_params_ref as ref

BLOCK_SIZES = (1, 2, 63, 64, 4096, 65535, 65536)
RATIOS = (1.0, 0.85, 0.5, ref.SMALLEST_RATIO)
DATA_KINDS = ("text", "random", "run")
MAX_INPUT = 300 * 1024
MALFORMED, OUTPUT_TOO_SMALL = 1, 2                # ACHIP_CLASS_*
CHECKSUM = -(MALFORMED + 16 * 95)                 # ACHIP_D_SNF_CHECKSUM
MAX_OUTPUT = -(OUTPUT_TOO_SMALL + 16 * 97)        # ACHIP_D_SNF_MAX_OUTPUT
OVERFLOW_STREAMS, OVERFLOW_LENGTH, OVERFLOW_BLOCK_SIZE = 1024, 1025, 1  # 1 049 600 blocks: more than the block list's 2^20 entries


def lengths(block_size):
    return [n for n in (0, 1, block_size - 1, block_size, block_size + 1, 3 * block_size + 7) if n <= MAX_INPUT]


@functools.lru_cache(None)
def _text():
    return b"".join(d for _, d, _ in common.corpus_sample())


@functools.lru_cache(None)
def _random():
    return np.random.default_rng(85).integers(0, 256, MAX_INPUT, dtype=np.uint8).tobytes()


def data(kind, n, shift=0):
    """n bytes of a kind; `shift` moves the window, so that equal lengths at different block sizes are different bytes"""
    if kind == "text":
        return _text()[shift:shift + n]
    if kind == "random":
        return _random()[shift % 1000:shift % 1000 + n]
    return bytes([0x61 + shift % 26]) * n


@functools.lru_cache(None)
def inputs(block_size):
    """[(name, bytes)]: every data kind at every length of this block size (equal lengths, as B - 1 and 1 at B = 2, once)"""
    out = []
    for kind in DATA_KINDS:
        for n in sorted(set(lengths(block_size))):
            out.append(("%s %d" % (kind, n), data(kind, n, block_size % 977)))
    return out


@functools.lru_cache(None)
def edge_pairs():
    """[(name, block size, input, ratio kept, ratio raw)]: the first block of the input compresses from l to c bytes; at c / l it is kept, at the double below
    c / l it is stored.  Block lengths 63 and 65535 make the quotient inexact, 4096 makes it exact."""
    o = oracle_lib.load()
    out = []
    for name, block_size, kind, n in (("run 196 at 63", 63, "run", 3 * 63 + 7), ("text 4096 at 4096", 4096, "text", 4096), ("text 65535 at 65535", 65535, "text", 65535),
                                      ("text 65537 at 65536", 65536, "text", 65537), ("text 12295 at 4096", 4096, "text", 3 * 4096 + 7)):
        d = data(kind, n, 4321)
        l = min(n, block_size)
        c = len(o.compress("snappy", d[:l]))
        assert 0 < c < l, (name, c, l)
        kept = float(c) / float(l)
        out.append((name, block_size, d, kept, math.nextafter(kept, 0.0)))
    return out


@functools.lru_cache(None)
def parameter_sets():
    """[(write_checksums, block_size, ratio)] of the catalog: every block size at every ratio, with and without checksums"""
    return [(checksums, block_size, ratio) for block_size in BLOCK_SIZES for ratio in RATIOS for checksums in (True, False)]


def params_name(params):
    return "checksums %d, block %d, ratio %r" % (int(params[0]), params[1], params[2])


@functools.lru_cache(None)
def expected(params, name):
    checksums, block_size, ratio = params
    return ref.compress(dict(inputs(block_size))[name], checksums, block_size, ratio)


@functools.lru_cache(None)
def overflow_streams():
    """1 024 streams of 1 025 bytes for block size 1: four different ones in turn (the model runs 1 025 blocks four times, not a million)"""
    kinds = [data("text", OVERFLOW_LENGTH, 100), data("random", OVERFLOW_LENGTH, 7), data("run", OVERFLOW_LENGTH, 3), data("text", OVERFLOW_LENGTH, 50000)]
    return [kinds[i % 4] for i in range(OVERFLOW_STREAMS)]


def cut_positions(n, block_size, count=6):
    """where a stream of n bytes is handed to a window writer in two pieces: the ends, around the first block boundary, and a few positions between"""
    return sorted({0, n, min(block_size, n), min(block_size + 1, n), max(min(block_size, n) - 1, 0), max(n - 1, 0)} | {int(p) for p in np.linspace(0, n, count)})


@functools.lru_cache(None)
def reader_streams():
    """[(name, stream, plaintext, status with verify on, its offset, status with verify off, its offset)]"""
    out = []
    text = data("text", 3 * 4096 + 7, 11)
    for params in ((True, 4096, 0.85), (True, 63, 0.5), (True, 1, 0.85), (True, 65536, ref.SMALLEST_RATIO)):
        d = text[:300] if params[1] == 1 else text
        out.append(("written with %s" % params_name(params), ref.compress(d, *params), d, 0, 0, 0, 0))
    free = ref.compress(text, False, 4096, 0.85)
    out.append(("checksum-free", free, text, CHECKSUM, 10, 0, 0))
    out.append(("checksum-free, stored chunks", ref.compress(text, False, 4096, ref.SMALLEST_RATIO), text, CHECKSUM, 10, 0, 0))
    out.append(("checksum-free, empty", ref.compress(b"", False, 4096, 0.85), b"", 0, 0, 0, 0))
    good = ref.compress(text, True, 4096, 0.85)
    third = ref.chunks(good)[2][0]
    damaged = bytearray(good)
    damaged[third + 5] ^= 0x10  # one CRC field, in the third chunk
    out.append(("one damaged CRC field", bytes(damaged), text, CHECKSUM, third, 0, 0))
    # structure: the same under both settings
    cut = good[:third + 6]
    out.append(("cut inside a chunk", cut, None, -(MALFORMED + 16 * 91), third, -(MALFORMED + 16 * 91), third))
    unskippable = bytearray(good)
    unskippable[third] = 0x02
    out.append(("an unskippable chunk", bytes(unskippable), None, -(MALFORMED + 16 * 93), third, -(MALFORMED + 16 * 93), third))
    out.append(("no stream header", good[10:], None, -(MALFORMED + 16 * 89), 0, -(MALFORMED + 16 * 89), 0))
    return out
