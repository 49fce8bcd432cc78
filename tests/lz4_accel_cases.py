"""The inputs of the LZ4 acceleration tests (tests/test_gpu_lz4_accel.py, tools/hostemu/check_lz4_accel.py, tools/record_lz4_accel_vectors.py): the smallest
shapes at which the accelerated kernels can go wrong, built once.  Expected bytes come from tests/lz4_accel_ref.py."""
import functools

import numpy as np

from tests import common, lz4_accel_ref as ref

ACCELERATIONS = (1, 2, 3, 4, 7, 8, 16, 63, 64, 65, 1000, 65537)
FRAME_ACCELERATIONS = (1, 4, 64)
LIMIT_ACCELERATIONS = (2, 3, 7)


@functools.lru_cache(None)
def _sample():
    return {name.split("@")[0]: data for name, data, _ in common.corpus_sample() if name.endswith("@0")}


def alice():
    return _sample()["canterbury/alice29.txt"]


def book():
    return _sample()["calgary/book1"]


def noise(n, seed=11):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(None)
def skipped_repeat(a):
    """A block whose only repeat starts at a position acceleration 1 probes (and matches there, no catch-up) and acceleration `a` steps over: `a` finds it at a
    later probe and extends the match backwards by more than 4 bytes -- more than the window encoder has in registers, the catch-up from memory.  Found by
    trying seeds against the model's trace; the first that fits is the case."""
    for seed in range(4000):
        rng = np.random.default_rng(1000 * a + seed)
        filler = rng.integers(0, 256, 400, dtype=np.uint8).tobytes()
        repeat = rng.integers(0, 256, 48, dtype=np.uint8).tobytes()
        s1 = int(rng.integers(3, 80))
        s2 = s1 + 48 + int(rng.integers(8, 120))
        data = filler[:s1] + repeat + filler[s1:s2 - s1 - 48 + s1] + repeat + filler[200:240]
        plain, fast = [], []
        ref.compress(data, 1, plain)
        ref.compress(data, a, fast)
        if len(plain) == 1 and len(fast) == 1 and plain[0][0] == s2 and plain[0][2] == 0 and fast[0][2] > 4 and fast[0][0] == s2:
            return data
    raise AssertionError("no such block for acceleration %d" % a)


@functools.lru_cache(None)
def block_cases():
    """[(name, bytes)] -- every entry goes through every (variant, acceleration)"""
    a, b = alice(), book()
    out = [
        ("alice 64 KiB", a[:65536]),            # short sequences: the masked replay, candidates inside the window, the vector path
        ("book1 64 KiB", b[:65536]),
        ("text 65537", (a + b)[:65537]),        # the wide-table kernel, the launch of both widths
        ("text 70000", (b + a)[:70000]),
        ("random 8 KiB", noise(8192)),          # a search runs through windows into the batch-probe step with the generalised schedule
        ("random 1 MiB", noise(1 << 20, 12)),   # large probe indexes: the advance grows by one every 64 probes
        ("text + random + text", a[:3000] + noise(6000, 13) + a[3000:6000]),  # the batch-probe step hands back to the window: k0 is a popcount
        ("zeros 5000", bytes(5000)),            # re-probe hits, zero-literal tokens
        ("empty", b""), ("one byte", b"x"), ("twelve bytes", a[100:112]),
    ]
    out += [("only repeat skipped at %d" % k, skipped_repeat(k)) for k in (2, 3, 7, 16)]
    return out


def limit_cases(a):
    """every length 13 .. 13 + 3a + 20 of text: a probe that ends the block by stepping past matchFindLimit over positions nobody looked at"""
    text = alice()[2000:]
    return [("text of %d bytes" % n, text[:n]) for n in range(13, 13 + 3 * a + 20 + 1)]


@functools.lru_cache(None)
def frame_cases():
    a = alice()
    tiled = (a[:30000] + book()[:20000]) * 85  # (a period below the 64 KiB a match reaches back: long matches from the second copy on, the model stays quick)
    return [("empty", b""), ("one byte", b"q"), ("100 000 text bytes", (a + book())[:100000]), ("4 MiB + 4321: two blocks", tiled[:(4 << 20) + 4321]),
            ("64 KiB random: a stored block", noise(65536, 14))]


@functools.lru_cache(None)
def expected(name, acceleration):
    data = dict(block_cases())[name]
    return ref.compress(data, acceleration)
