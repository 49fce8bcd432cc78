"""The inputs and settings of the LZ4 frame writer tests (tests/test_gpu_lz4f_writer.py, tools/hostemu/check_lz4f_writer.py): the smallest shapes at which the
block-list writer's kernels can go wrong, built once.  Expected bytes come from tests/lz4f_writer_ref.py.

  64 KiB       lengths 0, 1, 12 (below the encoder's minimum: literals only), 65535, 65536, 65537 (a second block of one byte), 131072, 3 * 65536 + 777
               data: zeros (long matches), text-like, random (stored), and per-block mixes -- a stored block between compressed ones (the compaction copies from
               the source between two moves), a compressed one between stored ones, all stored (nothing moves)
               all eight combinations of block checksum, content checksum and content size
  256 KiB ..   lengths B - 1, B, B + 1 with every flag off and every flag on: the wide hash table, and a two-block frame whose second block is one byte
  4 MiB
  misalignment four offsets 0 .. 3 beyond a 16-byte boundary for sources and destinations (MISALIGNMENTS; the tests place item i by it): the compaction moves a
               block to the left by a few bytes

Every case carries labels; tests/test_lz4f_writer_ref.py proves from the model's bytes that a case holds what its labels say."""
import collections
import functools
import itertools

import numpy as np

from tests import lz4f_writer_ref as ref

KIB64 = 65536
LENGTHS_64K = (0, 1, 12, 65535, 65536, 65537, 131072, 3 * 65536 + 777)
LARGE_BLOCK_SIZES = (262144, 1048576, 4194304)
FLAG_SETS = tuple(itertools.product((0, 1), repeat=3))  # (block checksum, content checksum, content size)
MISALIGNMENTS = (0, 1, 2, 3)
INVALID_ARGUMENT, OUTPUT_TOO_SMALL = 3, 2                 # ACHIP_CLASS_*
MAX_OUTPUT = -(OUTPUT_TOO_SMALL + 16 * 87)                # ACHIP_D_LZ4F_MAX_OUTPUT
BAD_ARGUMENT = -(INVALID_ARGUMENT + 16 * 102)             # ACHIP_D_BAD_ARGUMENT
UNSUPPORTED = -(INVALID_ARGUMENT + 16 * 103)              # ACHIP_D_UNSUPPORTED

Case = collections.namedtuple("Case", "name settings data labels")  # settings: (block size, block checksum, content checksum, content size)


@functools.lru_cache(None)
def _random():
    return np.random.default_rng(4).integers(0, 256, (4 << 20) + 16, dtype=np.uint8).tobytes()


@functools.lru_cache(None)
def _text():
    """text-like: words of a small vocabulary in random order -- short matches at short distances, literals between them"""
    rng = np.random.default_rng(1984)
    letters = np.frombuffer(b"etaoinshrdlucmfwypvbgkqjxz", dtype=np.uint8)
    words = [letters[rng.integers(0, 26, rng.integers(2, 11))].tobytes() for _ in range(300)]
    picks = rng.integers(0, len(words), 1100000)
    out = b" ".join(words[i] for i in picks)
    assert len(out) >= (4 << 20) + 16
    return out


def data(kind, n, shift=0):
    if kind == "zeros":
        return bytes(n)
    if kind == "text":
        return _text()[shift:shift + n]
    if kind == "random":
        return _random()[shift % 7:shift % 7 + n]
    # a mix: the kinds of its blocks in turn, e.g. "text/random/text"
    kinds = kind.split("/")
    out = bytearray()
    k = 0
    while len(out) < n:
        out += data(kinds[k % len(kinds)], min(KIB64, n - len(out)), shift + 13 * k)
        k += 1
    return bytes(out)


def settings_name(s):
    return "%d KiB, block checksum %d, content checksum %d, content size %d" % (s[0] >> 10, s[1], s[2], s[3])


def _labels(settings, kind, n):
    block_size, bc, cc, cs = settings
    blocks = (n + block_size - 1) // block_size
    labels = set()
    if n == 0:
        labels.add("empty")
    if blocks >= 2:
        labels.add("two blocks")
    if bc and blocks:
        labels.add("block checksum")
    if cc:
        labels.add("content checksum")
    if cs:
        labels.add("content size")
    kinds = kind.split("/")
    per_block = [kinds[k % len(kinds)] for k in range(blocks)]
    sizes = [min(block_size, n - k * block_size) for k in range(blocks)]
    stored = [k == "random" or z <= 12 for k, z in zip(per_block, sizes)]  # (up to 12 bytes are literals only: a token more than the block)
    if any(stored):
        labels.add("stored")
    if not all(stored):
        labels.add("compressed")
    if any(a and not b for a, b in zip(stored, stored[1:])) and not stored[0]:
        labels.add("stored between compressed")
    if len(stored) >= 3 and stored[0] and not stored[1] and stored[2]:
        labels.add("compressed between stored")
    if blocks >= 2 and all(stored):
        labels.add("all stored")
    if any(z > 65536 for z in sizes):
        labels.add("wide table")
    return frozenset(labels)


@functools.lru_cache(None)
def inputs_64k():
    """[(kind, length)] at 64 KiB: the three plain kinds at every length, the mixes at the lengths that have several blocks"""
    out = [(kind, n) for kind in ("zeros", "text", "random") for n in LENGTHS_64K]
    out += [(kind, n) for kind in ("text/random/text", "random/text/random", "zeros/random/zeros/text") for n in (131072, 3 * 65536 + 777)]
    return out


@functools.lru_cache(None)
def catalog():
    out = []
    for flags in FLAG_SETS:
        settings = (KIB64,) + flags
        for i, (kind, n) in enumerate(inputs_64k()):
            out.append(Case("%s %d at %s" % (kind, n, settings_name(settings)), settings, data(kind, n, 100 * i), _labels(settings, kind, n)))
    for block_size in LARGE_BLOCK_SIZES:
        for flags in ((0, 0, 0), (1, 1, 1)):
            settings = (block_size,) + flags
            for n in (block_size - 1, block_size, block_size + 1):
                out.append(Case("text %d at %s" % (n, settings_name(settings)), settings, data("text", n, block_size % 1000), _labels(settings, "text", n)))
    return out


def by_settings():
    """{settings: [Case]} in the catalog's order"""
    out = collections.OrderedDict()
    for c in catalog():
        out.setdefault(c.settings, []).append(c)
    return out


@functools.lru_cache(None)
def expected(name, acceleration=1):
    c = next(c for c in catalog() if c.name == name)
    return ref.compress(c.data, *c.settings, acceleration=acceleration)


def bound(case_or_len, settings=None):
    if isinstance(case_or_len, Case):
        return ref.max_compressed_length(len(case_or_len.data), *case_or_len.settings)
    return ref.max_compressed_length(case_or_len, *settings)


REQUIRED_LABELS = ("empty", "two blocks", "block checksum", "content checksum", "content size", "stored", "compressed", "stored between compressed",
                   "compressed between stored", "all stored", "wide table")
