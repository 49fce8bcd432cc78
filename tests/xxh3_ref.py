"""An independent pure-Python XXH3-64 / XXH3-128 (xxHash 0.8, scalar form) for the tests: the GPU kernels are checked against it on
arbitrary data, on machines that have neither libxxhash nor the `xxhash` module.  It is pinned by tests/golden/xxh3_vectors.json
(tests/test_xxh3_ref.py).  Short inputs are plain Python, long ones numpy (a few MB/s).

xxh3_64(data, seed) returns the unsigned 64-bit hash; xxh3_128(data, seed) returns (low64, high64), both unsigned.  The seed is taken
modulo 2^64, so a Java long (signed) can be passed as it is.
"""
import struct

import numpy as np

M64 = (1 << 64) - 1
P32_1, P32_2, P32_3 = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D
P64_1, P64_2, P64_3, P64_4, P64_5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
PRIME_MX1, PRIME_MX2 = 0x165667919E3779F9, 0x9FB21C651E98DF25

K_SECRET = bytes.fromhex(
    "b8fe6c3923a44bbe7c01812cf721ad1cded46de9839097db7240a4a4b7b3671f"
    "cb79e64eccc0e578825ad07dccff7221b8084674f743248ee03590e6813a264c"
    "3c2852bb91c300cb88d0658b1b532ea371644897a20df94e3819ef46a9deacd8"
    "a8fa763fe39c343ff9dcbbc7c70b4f1d8a51e04bcdb45931c89f7ec9d9787364"
    "eac5ac8334d3ebc3c581a0fffa1363eb170ddd51b7f0da49d316552629d4689e"
    "2b16be587d47a1fc8ff8b8d17ad031ce45cb3a8f95160428afd7fbcabb4b407e")
assert len(K_SECRET) == 192

STRIPE_LEN, STRIPES_PER_BLOCK, BLOCK_LEN = 64, 16, 1024
SECRET_LASTACC_START, SECRET_MERGEACCS_START = 7, 11
MIDSIZE_STARTOFFSET, MIDSIZE_LASTOFFSET, SECRET_SIZE_MIN = 3, 17, 136


def r32(b, i):
    return struct.unpack_from("<I", b, i)[0]


def r64(b, i):
    return struct.unpack_from("<Q", b, i)[0]


def rotl64(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def rotl32(x, r):
    return ((x << r) | (x >> (32 - r))) & 0xFFFFFFFF


def swap32(x):
    return int.from_bytes(x.to_bytes(4, "little"), "big")


def swap64(x):
    return int.from_bytes(x.to_bytes(8, "little"), "big")


def mul128(a, b):
    p = a * b
    return p & M64, p >> 64


def fold64(a, b):
    lo, hi = mul128(a, b)
    return lo ^ hi


def xxh64_avalanche(h):
    h ^= h >> 33
    h = (h * P64_2) & M64
    h ^= h >> 29
    h = (h * P64_3) & M64
    return h ^ (h >> 32)


def avalanche(h):
    h ^= h >> 37
    h = (h * PRIME_MX1) & M64
    return h ^ (h >> 32)


def rrmxmx(h, n):
    h ^= rotl64(h, 49) ^ rotl64(h, 24)
    h = (h * PRIME_MX2) & M64
    h ^= ((h >> 35) + n) & M64
    h = (h * PRIME_MX2) & M64
    return h ^ (h >> 28)


def mix16(d, i, s, j, seed):
    return fold64(r64(d, i) ^ ((r64(s, j) + seed) & M64), r64(d, i + 8) ^ ((r64(s, j + 8) - seed) & M64))


def derive_secret(seed):
    """the custom secret of a seeded long input (XXH3_initCustomSecret)"""
    out = bytearray(192)
    for i in range(12):
        struct.pack_into("<QQ", out, 16 * i, (r64(K_SECRET, 16 * i) + seed) & M64, (r64(K_SECRET, 16 * i + 8) - seed) & M64)
    return bytes(out)


def _long_accs(d, s):
    """the eight accumulators of a long input (numpy: the 16 stripes of every block are summed at once, uint64 wraps mod 2^64)"""
    n = len(d)
    acc = np.array([P32_3, P64_1, P64_2, P64_3, P64_4, P32_2, P64_5, P32_1], dtype=np.uint64)
    sw = np.frombuffer(s, dtype="<u8").astype(np.uint64)
    keys = np.stack([sw[k:k + 8] for k in range(STRIPES_PER_BLOCK)])  # (16, 8): stripe k uses secret words k .. k+7
    swap = [i ^ 1 for i in range(8)]
    lo32 = np.uint64(0xFFFFFFFF)

    def parts(x, k):  # x: (..., stripes, 8) words, k: (stripes, 8) keys -> what each stripe adds, summed over the stripes
        dk = x ^ k
        return (x[..., swap] + (dk & lo32) * (dk >> np.uint64(32))).sum(axis=-2, dtype=np.uint64)

    blocks = (n - 1) // BLOCK_LEN
    words = np.frombuffer(d, dtype="<u8", count=blocks * BLOCK_LEN // 8).astype(np.uint64).reshape(blocks, STRIPES_PER_BLOCK, 8)
    adds = parts(words, keys)
    skey = sw[16:24]
    with np.errstate(over="ignore"):
        for b in range(blocks):
            a = acc + adds[b]
            acc = ((a ^ (a >> np.uint64(47))) ^ skey) * np.uint64(P32_1)
        rest = ((n - 1) - BLOCK_LEN * blocks) // STRIPE_LEN
        if rest:
            tail = np.frombuffer(d, dtype="<u8", count=rest * 8, offset=blocks * BLOCK_LEN).astype(np.uint64).reshape(rest, 8)
            acc = acc + parts(tail, keys[:rest])
        last = np.frombuffer(d, dtype="<u8", count=8, offset=n - STRIPE_LEN).astype(np.uint64).reshape(1, 8)
        lkey = np.array([r64(s, 192 - STRIPE_LEN - SECRET_LASTACC_START + 8 * i) for i in range(8)], dtype=np.uint64).reshape(1, 8)
        acc = acc + parts(last, lkey)
    return [int(v) for v in acc]


def _merge(acc, s, so, start):
    r = start
    for i in range(4):
        r += fold64(acc[2 * i] ^ r64(s, so + 16 * i), acc[2 * i + 1] ^ r64(s, so + 16 * i + 8))
    return avalanche(r & M64)


def xxh3_64(data, seed=0):
    d = bytes(data)
    n = len(d)
    seed &= M64
    s = K_SECRET
    if n == 0:
        return xxh64_avalanche(seed ^ r64(s, 56) ^ r64(s, 64))
    if n <= 3:
        c = (d[0] << 16) | (d[n >> 1] << 24) | d[n - 1] | (n << 8)
        return xxh64_avalanche(c ^ (((r32(s, 0) ^ r32(s, 4)) + seed) & M64))
    if n <= 8:
        sd = seed ^ (swap32(seed & 0xFFFFFFFF) << 32)
        x = (r32(d, n - 4) + (r32(d, 0) << 32)) ^ (((r64(s, 8) ^ r64(s, 16)) - sd) & M64)
        return rrmxmx(x, n)
    if n <= 16:
        lo = r64(d, 0) ^ (((r64(s, 24) ^ r64(s, 32)) + seed) & M64)
        hi = r64(d, n - 8) ^ (((r64(s, 40) ^ r64(s, 48)) - seed) & M64)
        return avalanche((n + swap64(lo) + hi + fold64(lo, hi)) & M64)
    if n <= 128:
        acc = n * P64_1
        for i in range((n - 1) // 32, -1, -1):
            acc += mix16(d, 16 * i, s, 32 * i, seed) + mix16(d, n - 16 * (i + 1), s, 32 * i + 16, seed)
        return avalanche(acc & M64)
    if n <= 240:
        acc = n * P64_1
        for i in range(8):
            acc += mix16(d, 16 * i, s, 16 * i, seed)
        acc = avalanche(acc & M64)
        for i in range(8, n // 16):
            acc += mix16(d, 16 * i, s, 16 * (i - 8) + MIDSIZE_STARTOFFSET, seed)
        acc += mix16(d, n - 16, s, SECRET_SIZE_MIN - MIDSIZE_LASTOFFSET, seed)
        return avalanche(acc & M64)
    s = derive_secret(seed) if seed else K_SECRET
    return _merge(_long_accs(d, s), s, SECRET_MERGEACCS_START, (n * P64_1) & M64)


def _mix32(acc, d, i1, i2, s, j, seed):
    lo, hi = acc
    lo = (lo + mix16(d, i1, s, j, seed)) & M64
    lo ^= (r64(d, i2) + r64(d, i2 + 8)) & M64
    hi = (hi + mix16(d, i2, s, j + 16, seed)) & M64
    hi ^= (r64(d, i1) + r64(d, i1 + 8)) & M64
    return lo, hi


def _fin128(acc, n, seed):
    lo, hi = acc
    h_lo = avalanche((lo + hi) & M64)
    h_hi = avalanche((lo * P64_1 + hi * P64_4 + ((n - seed) & M64) * P64_2) & M64)
    return h_lo, (-h_hi) & M64


def xxh3_128(data, seed=0):
    d = bytes(data)
    n = len(d)
    seed &= M64
    s = K_SECRET
    if n == 0:
        return xxh64_avalanche(seed ^ r64(s, 64) ^ r64(s, 72)), xxh64_avalanche(seed ^ r64(s, 80) ^ r64(s, 88))
    if n <= 3:
        cl = (d[0] << 16) | (d[n >> 1] << 24) | d[n - 1] | (n << 8)
        ch = rotl32(swap32(cl), 13)
        lo = cl ^ (((r32(s, 0) ^ r32(s, 4)) + seed) & M64)
        hi = ch ^ (((r32(s, 8) ^ r32(s, 12)) - seed) & M64)
        return xxh64_avalanche(lo), xxh64_avalanche(hi)
    if n <= 8:
        sd = seed ^ (swap32(seed & 0xFFFFFFFF) << 32)
        x = (r32(d, 0) + (r32(d, n - 4) << 32)) ^ (((r64(s, 16) ^ r64(s, 24)) + sd) & M64)
        lo, hi = mul128(x, (P64_1 + (n << 2)) & M64)
        hi = (hi + (lo << 1)) & M64
        lo ^= hi >> 3
        lo ^= lo >> 35
        lo = (lo * PRIME_MX2) & M64
        lo ^= lo >> 28
        return lo, avalanche(hi)
    if n <= 16:
        bl = ((r64(s, 32) ^ r64(s, 40)) - seed) & M64
        bh = ((r64(s, 48) ^ r64(s, 56)) + seed) & M64
        ilo, ihi = r64(d, 0), r64(d, n - 8)
        lo, hi = mul128(ilo ^ ihi ^ bl, P64_1)
        lo = (lo + ((n - 1) << 54)) & M64
        ihi ^= bh
        hi = (hi + ihi + (ihi & 0xFFFFFFFF) * (P32_2 - 1)) & M64
        lo ^= swap64(hi)
        h_lo, h_hi = mul128(lo, P64_2)
        h_hi = (h_hi + hi * P64_2) & M64
        return avalanche(h_lo), avalanche(h_hi)
    if n <= 128:
        acc = ((n * P64_1) & M64, 0)
        for i in range((n - 1) // 32, -1, -1):
            acc = _mix32(acc, d, 16 * i, n - 16 * (i + 1), s, 32 * i, seed)
        return _fin128(acc, n, seed)
    if n <= 240:
        acc = ((n * P64_1) & M64, 0)
        for i in range(4):
            acc = _mix32(acc, d, 32 * i, 32 * i + 16, s, 32 * i, seed)
        acc = (avalanche(acc[0]), avalanche(acc[1]))
        for i in range(4, n // 32):
            acc = _mix32(acc, d, 32 * i, 32 * i + 16, s, MIDSIZE_STARTOFFSET + 32 * (i - 4), seed)
        acc = _mix32(acc, d, n - 16, n - 32, s, SECRET_SIZE_MIN - MIDSIZE_LASTOFFSET - 16, (-seed) & M64)
        return _fin128(acc, n, seed)
    s = derive_secret(seed) if seed else K_SECRET
    acc = _long_accs(d, s)
    return (_merge(acc, s, SECRET_MERGEACCS_START, (n * P64_1) & M64),
            _merge(acc, s, 192 - STRIPE_LEN - SECRET_MERGEACCS_START, (~(n * P64_2)) & M64))
