"""The cases of the streaming hashers (aircompressor_amd/csrc/xxhash_stream.hip), shared by the GPU tests (tests/test_gpu_xxhash_stream.py)
and the emulator check (tools/hostemu/check_xxh_stream.py).

Scheme: state i owns a plaintext (bytes [start, start + total) of one shared random buffer) and a list of cut points.  Round r updates every
state with its r-th piece in ONE call (length 0 where a state has run out); after a round every state is digested and compared with the
one-shot reference of the PREFIX absorbed so far -- which also shows that digest leaves the state alone.  References: tests/xxh3_ref.py
for XXH3, the oracle's xxh64 / xxh32 for the others; every comparison is exact equality."""
import numpy as np

from tests import oracle_lib, xxh3_ref

M64 = (1 << 64) - 1
XXH32, XXH64, XXH3_64, XXH3_128 = 0, 1, 2, 3
ALGOS = [XXH32, XXH64, XXH3_64, XXH3_128]
ALGO_NAMES = ["xxh32", "xxh64", "xxh3_64", "xxh3_128"]
SEEDS = [0, 1, -1, 2654435761, 0x9E3779B185EBCA87]
SMALL_CUTS = [0, 1, 3, 4, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129, 240, 241, 255, 256, 257, 319, 320, 321, 511, 512, 513]
LONG_STARTS = [1, 63, 64, 65, 960, 1023, 1024, 1025]
UNEVEN_TOTALS = [0, 5, 16, 100, 240, 241, 1000, 5000, 65536, 70001]

_data = None
_refs = {}


def data():
    """the shared plaintext: 70 001 + 128 random bytes, fixed"""
    global _data
    if _data is None:
        _data = np.random.default_rng(20260117).integers(0, 256, 70001 + 128, dtype=np.uint8).tobytes()
    return _data


def reference_of(algo, b, seed):
    """the one-shot hash of bytes b: an unsigned int, or (low, high) for XXH3-128"""
    if algo == XXH32:
        return int(oracle_lib.load().xxh32(b, seed & 0xFFFFFFFF))
    if algo == XXH64:
        return int(oracle_lib.load().xxh64(b, seed & M64))
    return xxh3_ref.xxh3_128(b, seed) if algo == XXH3_128 else xxh3_ref.xxh3_64(b, seed)


def reference(algo, start, length, seed):
    """... of data()[start, start + length), computed once"""
    key = (algo, start, length, seed & M64)
    if key not in _refs:
        _refs[key] = reference_of(algo, data()[start:start + length], seed)
    return _refs[key]


# ---- plans: lists of (start, total, cuts) ----
def small_plan(totals=range(0, 601), cuts=SMALL_CUTS):
    """every total, cut once at every listed position that is <= total"""
    return [(0, t, [c]) for t in totals for c in cuts if c <= t]


def boundary_plan(ks=(1, 2, 3, 4, 64), ds=range(-65, 66)):
    """totals 1024 k + d.  Per total: a state whose pieces end one before, at and one after a multiple of 64 (not of 1024) near the middle, one the
    same around a multiple of 1024, and one state per position of LONG_STARTS at which its second -- long -- piece starts."""
    plan = []
    for k in ks:
        for d in ds:
            t = 1024 * k + d
            m64 = 64 * ((t // 128) | 1)  # (an odd multiple of 64: never one of 1024)
            m1024 = 1024 * max(1, (k + 1) // 2)
            for m in (m64, m1024):
                plan.append((3, t, [c for c in (m - 1, m, m + 1) if c <= t]))
            plan += [(3, t, [s]) for s in LONG_STARTS if s <= t]
    return plan


def dribble_plan(steps, sizes=(1,)):
    """one state fed `steps` pieces whose sizes rotate through `sizes`"""
    cuts, pos = [], 0
    for r in range(steps):
        pos += sizes[r % len(sizes)]
        cuts.append(pos)
    return [(5, pos, cuts[:-1])]


def uneven_plan(n, seed, totals=UNEVEN_TOTALS):
    """n states, totals drawn from `totals`, 1..9 random cuts each: short and long pieces land in the same call"""
    rng = np.random.default_rng(seed)
    totals = rng.choice(totals, size=n)
    starts = rng.integers(0, 97, n)
    ncuts = rng.integers(1, 10, n)
    return [(int(s), int(t), sorted(int(c) for c in rng.integers(0, t + 1, k))) for s, t, k in zip(starts, totals, ncuts)]


def three_piece_plan(n, blocks=8, size=65536, cuts=(1000, 41000)):
    return [(size * (i % blocks), size, list(cuts)) for i in range(n)]


# ---- running a plan ----
class Backend:
    """What a plan runs on.  Subclasses give memory (alloc / free / h2d / d2h over integer addresses) and the four calls of the C ABI's shape
    (state_size, reset, update, digest over addresses); the same code then drives the library on a GPU and the kernels under the emulator."""

    def to_device(self, array):
        p = self.alloc(array.nbytes + 64)
        assert p
        self.h2d(p, array)
        return p

    def read_hashes(self, algo, states, n):
        out = np.zeros(n * (2 if algo == XXH3_128 else 1), dtype=np.int64)
        p = self.alloc(out.nbytes + 64)
        self.digest(algo, states, p, n)
        self.d2h(out, p)
        self.free(p)
        u = [int(v) & M64 for v in out]
        return [(u[2 * i], u[2 * i + 1]) for i in range(n)] if algo == XXH3_128 else u


def pack(plan, misalign=3):
    """a source buffer that holds every state's plaintext at an odd offset from a misaligned base (as run_batch of tests/test_gpu_xxhash3.py
    packs its buffers) -> (src, offsets)"""
    offs, pos = [], misalign
    for _, t, _ in plan:
        offs.append(pos)
        pos += t + (t % 7) + 1
    src = np.zeros(pos + 64, dtype=np.uint8)
    d = np.frombuffer(data(), dtype=np.uint8)
    for (s, t, _), so in zip(plan, offs):
        src[so:so + t] = d[s:s + t]
    return src, offs


def run_plan(be, algo, plan, seed, packed=False, misalign=3, digest_every_round=True, src=None, want=None):
    """Runs the plan on `be`; returns the mismatches as (state, round, bytes absorbed).  packed: every state's plaintext gets its own odd
    offset in the source (else the states read the shared buffer in place, at base `misalign`).  src / want: another source buffer (plaintext
    i = src[start, start + total)) and the function giving the expected value of (state, absorbed) for it."""
    n = len(plan)
    if src is not None:
        offs = [s for s, _, _ in plan]
    elif packed:
        src, offs = pack(plan, misalign)
    else:
        src = np.zeros(misalign + len(data()) + 64, dtype=np.uint8)
        src[misalign:misalign + len(data())] = np.frombuffer(data(), dtype=np.uint8)
        offs = [misalign + s for s, _, _ in plan]
    if want is None:
        want = lambda i, absorbed: reference(algo, plan[i][0], absorbed, seed)  # noqa: E731
    size = be.state_size(algo)
    assert size > 0 and size % 16 == 0 and size < 1024
    states = be.alloc(size * n + 64)
    dsrc = be.to_device(src)
    doff, dlen = be.alloc(8 * n + 64), be.alloc(4 * n + 64)
    assert states and doff and dlen
    be.reset(algo, states, n, seed)
    rounds = max(len(c) for _, _, c in plan) + 1
    bad = []
    for r in range(rounds + 1):  # (the last round is all zero lengths: nothing may change)
        ends = np.array([(c + [t])[r] if r <= len(c) else t for _, t, c in plan], dtype=np.int64)
        begins = np.array([0 if r == 0 else ((c + [t])[r - 1] if r - 1 <= len(c) else t) for _, t, c in plan], dtype=np.int64)
        be.h2d(doff, np.asarray(offs, dtype=np.int64) + begins)
        be.h2d(dlen, (ends - begins).astype(np.int32))
        be.update(algo, states, dsrc, doff, dlen, n)
        if digest_every_round or r == rounds:
            got = be.read_hashes(algo, states, n)
            bad += [(i, r, int(ends[i])) for i in range(n) if got[i] != want(i, int(ends[i]))]
    for p in (states, dsrc, doff, dlen):
        be.free(p)
    return bad


def seeds_per_half(be, algo):
    """one array whose halves were reset with different seeds, updated in one call; then the first half reset again with a third seed"""
    n, size = 40, be.state_size(algo)
    plan = [(i % 7, 100 + 37 * i, [50 + i]) for i in range(n)]
    src = np.frombuffer(data(), dtype=np.uint8)
    states, dsrc, doff, dlen = be.alloc(size * n), be.to_device(src), be.alloc(8 * n), be.alloc(4 * n)
    seeds = [11] * (n // 2) + [-3] * (n // 2)
    be.reset(algo, states, n // 2, 11)
    be.reset(algo, states + size * (n // 2), n // 2, -3)
    bad = 0
    for again in (False, True):
        if again:
            be.reset(algo, states, n // 2, 0x1_0000_0005)  # (a used state becomes a fresh hasher)
            seeds = [0x1_0000_0005] * (n // 2) + [-3] * (n // 2)
        for lo, hi in ((0, 1), (1, 2)):
            be.h2d(doff, np.array([s + ([0] + c + [t])[lo] for s, t, c in plan], dtype=np.int64))
            be.h2d(dlen, np.array([([0] + c + [t])[hi] - ([0] + c + [t])[lo] if (i < n // 2 or not again) else 0 for i, (s, t, c) in enumerate(plan)], dtype=np.int32))
            be.update(algo, states, dsrc, doff, dlen, n)
        got = be.read_hashes(algo, states, n)
        bad += sum(g != reference(algo, s, t, sd) for g, (s, t, _), sd in zip(got, plan, seeds))
    if algo == XXH32:  # only the low 32 bits of the seed count
        bad += sum(g != reference(algo, s, t, 5) for g, (s, t, _) in zip(got[:n // 2], plan))
    for p in (states, dsrc, doff, dlen):
        be.free(p)
    return bad, 2 * n
