"""Host-side mirror of the reference's one-shot hashing API (`io.airlift.compress.v3.xxhash`) over the C ABI.

`XxHash64HipHasher.hash(...)` / `XxHash32HipHasher.hash(...)` follow `XxHash64Hasher.hash(byte[] input, int offset,
int length, long seed)` (M/xxhash/XxHash64Hasher.java:55-86) and `XxHash32Hasher.hash(...)` (M/xxhash/XxHash32Hasher.java):
same argument order, same range check, and the result is the Java `long` / `int` (signed).  `hash_batch` hashes many
device-resident buffers per call.  `XxHash3HipHasher` adds XXH3 (64- and 128-bit, the reference's XxHash3Native with a `long` seed;
`XxHash128` is its record of two signed longs).  The streaming form of the same hashers (`create(seed)` / `new_hasher(seed)`, then
`update` / `update_le_long` / `update_le_int` / `digest` / `reset` / `close`, M/xxhash/XxHash64Hasher.java:91-169) is `HipStreamHasher`;
`HipHashStates` is a batch of such states in device memory.  HIP only: no CPU fallback.
"""
import ctypes
import struct
from collections import namedtuple

import numpy as np

from . import native
from .errors import IllegalArgumentException

DEFAULT_SEED = 0


def _check_from_index_size(data, offset, length):
    # Objects.checkFromIndexSize (M/xxhash/XxHash64JavaHasher.java:75, XxHash32JavaHasher.java:70)
    n = len(data)
    if offset < 0 or length < 0 or offset + length > n:
        raise IndexError("Range [%d, %d + %d) out of bounds for length %d" % (offset, offset, length, n))


class _HipHasher:
    _wide = True

    def __init__(self, device=0, native_ctx=None):
        self.native = native_ctx or native.HipNative(device)
        self._lib = self.native.lib

    def hash(self, input, offset=0, length=None, seed=DEFAULT_SEED):
        view = np.frombuffer(input, dtype=np.uint8)
        if length is None:
            length = view.size - offset
        _check_from_index_size(view, offset, length)
        src = view[offset:offset + length]
        ptr = src.ctypes.data if src.size else None
        if self._wide:
            out = ctypes.c_int64(0)
            r = self._lib.achip_xxhash64(self.native.ctx, ptr, int(src.size), ctypes.c_int64(_as_signed(seed, 64)), ctypes.byref(out))
        else:
            out = ctypes.c_int32(0)
            r = self._lib.achip_xxhash32(self.native.ctx, ptr, int(src.size), ctypes.c_int32(_as_signed(seed, 32)), ctypes.byref(out))
        if r < 0:
            native.raise_for_status(r)
        return int(out.value)

    def hash_batch(self, src_base, src_off, src_len, out_hash, n_buffers, seed=DEFAULT_SEED):
        """device pointers (ints or objects with data_ptr()); asynchronous on the context's stream"""
        p = lambda x: ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))  # noqa: E731
        if self._wide:
            r = self._lib.achip_xxhash64_batch(self.native.ctx, p(src_base), p(src_off), p(src_len), ctypes.c_int64(_as_signed(seed, 64)), p(out_hash), int(n_buffers))
        else:
            r = self._lib.achip_xxhash32_batch(self.native.ctx, p(src_base), p(src_off), p(src_len), ctypes.c_int32(_as_signed(seed, 32)), p(out_hash), int(n_buffers))
        if r < 0:
            native.raise_for_status(r)


def _as_signed(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


HASH_XXH32, HASH_XXH64, HASH_XXH3_64, HASH_XXH3_128 = 0, 1, 2, 3


class HipStreamHasher:
    """A streaming hasher on the GPU: the reference's hasher object (XxHash64Hasher.java:91-169; XxHash32Hasher, XxHash3Hasher and
    XxHash3Hasher128 have the same methods).  The bytes of `update` are staged to the device in chunks and absorbed there, so one update
    may be longer than 2 GiB; `update` and `digest` block, `reset` does not.  `digest()` leaves the state as it is: it may be called
    mid-stream and twice.  Returns what the one-shot twins return: a signed long, a signed int (XXH32) or an XxHash128."""

    def __init__(self, algo, seed=DEFAULT_SEED, device=0, native_ctx=None):
        self.native = native_ctx or native.HipNative(device)
        self._lib = self.native.lib
        self._algo = algo
        self._h = self._lib.achip_hasher_create(self.native.ctx, algo, ctypes.c_int64(_as_signed(seed, 64)))
        if not self._h:
            raise native.HipUnavailableError("achip_hasher_create failed: %s" % self._lib.achip_last_error().decode())

    def _check_not_closed(self):
        # checkNotClosed (M/xxhash/XxHash3Native.java:330-334: IllegalStateException)
        if self._h is None:
            raise RuntimeError("Hasher has been closed")

    def update(self, input, offset=0, length=None):
        self._check_not_closed()
        view = np.frombuffer(input, dtype=np.uint8)
        if length is None:
            length = view.size - offset
        _check_from_index_size(view, offset, length)
        src = view[offset:offset + length]
        r = self._lib.achip_hasher_update(self._h, src.ctypes.data if src.size else None, int(src.size))
        if r < 0:
            native.raise_for_status(r)
        return self

    def update_le_long(self, v):
        """updateLE(long): the value's eight bytes, little-endian"""
        return self.update(struct.pack("<Q", v & ((1 << 64) - 1)))

    def update_le_int(self, v):
        """updateLE(int): the value's four bytes, little-endian"""
        return self.update(struct.pack("<I", v & 0xFFFFFFFF))

    def digest(self):
        self._check_not_closed()
        out = (ctypes.c_int64 * 2)()
        r = self._lib.achip_hasher_digest(self._h, out)
        if r < 0:
            native.raise_for_status(r)
        if self._algo == HASH_XXH3_128:
            return XxHash128(int(out[0]), int(out[1]))
        return _as_signed(int(out[0]), 32) if self._algo == HASH_XXH32 else int(out[0])

    def reset(self, seed=DEFAULT_SEED):
        self._check_not_closed()
        r = self._lib.achip_hasher_reset(self._h, ctypes.c_int64(_as_signed(seed, 64)))
        if r < 0:
            native.raise_for_status(r)
        return self

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            self._lib.achip_hasher_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipHashStates:
    """`n` hasher states of one algorithm in device memory (achip_hash_states_*): the batch form.  reset / update / digest take device
    pointers (ints or objects with data_ptr()) and are asynchronous on the context's stream.  update: state i absorbs
    src_base[src_off[i] .. + src_len[i]) (int64 offsets, int32 lengths; a length <= 0 leaves the state alone).  digest: out holds n int64
    (XXH32 zero-extended), 2n for XXH3-128 (low, high).  reset(seed, first, count) resets a sub-range: one array may mix seeds."""

    def __init__(self, algo, n, native_ctx=None, device=0):
        self.native = native_ctx or native.HipNative(device)
        self._lib = self.native.lib
        self.algo, self.n = algo, int(n)
        self.state_size = int(self._lib.achip_hash_state_size(algo))
        if self.state_size < 0:
            native.raise_for_status(self.state_size)
        self.ptr = self._lib.achip_device_alloc(self.native.ctx, max(1, self.state_size * self.n))
        if not self.ptr:
            raise native.HipUnavailableError("achip_device_alloc failed: %s" % self._lib.achip_last_error().decode())

    @staticmethod
    def _p(x):
        return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))

    def reset(self, seed=DEFAULT_SEED, first=0, count=None):
        count = self.n - first if count is None else count
        if first < 0 or count < 0 or first + count > self.n:
            raise IndexError("Range [%d, %d + %d) out of bounds for length %d" % (first, first, count, self.n))
        r = self._lib.achip_hash_states_reset(self.native.ctx, self.algo, ctypes.c_void_p(self.ptr + first * self.state_size), count, ctypes.c_int64(_as_signed(seed, 64)))
        if r < 0:
            native.raise_for_status(r)
        return self

    def update(self, src_base, src_off, src_len):
        r = self._lib.achip_hash_states_update(self.native.ctx, self.algo, ctypes.c_void_p(self.ptr), self._p(src_base), self._p(src_off), self._p(src_len), self.n)
        if r < 0:
            native.raise_for_status(r)
        return self

    def digest(self, out):
        r = self._lib.achip_hash_states_digest(self.native.ctx, self.algo, ctypes.c_void_p(self.ptr), self._p(out), self.n)
        if r < 0:
            native.raise_for_status(r)

    def close(self):
        if getattr(self, "ptr", None):
            self.native.synchronize()
            self._lib.achip_device_free(self.native.ctx, self.ptr)
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class XxHash64HipHasher(_HipHasher):
    """One-shot XXH64 (XxHash64Hasher.hash, M/xxhash/XxHash64Hasher.java:55-86); returns the Java long.  `create(seed)` gives the streaming
    hasher (XxHash64Hasher.create, :91-101)."""
    _wide = True

    @staticmethod
    def create(seed=DEFAULT_SEED, device=0, native_ctx=None):
        return HipStreamHasher(HASH_XXH64, seed, device, native_ctx)


class XxHash32HipHasher(_HipHasher):
    """One-shot XXH32 (XxHash32Hasher.hash, M/xxhash/XxHash32Hasher.java); returns the Java int.  `create(seed)` gives the streaming hasher."""
    _wide = False

    @staticmethod
    def create(seed=DEFAULT_SEED, device=0, native_ctx=None):
        return HipStreamHasher(HASH_XXH32, seed, device, native_ctx)


class XxHash128(namedtuple("XxHash128", ["low", "high"])):
    """The 128-bit XXH3 hash as the reference's record `XxHash128(long low, long high)`: two signed Java longs."""
    __slots__ = ()


class XxHash3HipHasher:
    """One-shot and batched XXH3-64 / XXH3-128 (the reference's XxHash3Native.hash / hash128 with a `long` seed) on the GPU.

    `hash` returns the Java long, `hash128` an XxHash128 of Java longs; argument order, range check and signed results follow
    XxHash64HipHasher.  `hash_batch` / `hash128_batch` hash many device-resident buffers per call (asynchronous on the context's
    stream); the 128-bit batch writes low, high to out_hash[2i], out_hash[2i + 1]."""

    def __init__(self, device=0, native_ctx=None):
        self.native = native_ctx or native.HipNative(device)
        self._lib = self.native.lib

    @staticmethod
    def new_hasher(seed=DEFAULT_SEED, device=0, native_ctx=None):
        """the streaming 64-bit hasher (XxHash3Native.newHasher, M/xxhash/XxHash3Native.java:77-105)"""
        return HipStreamHasher(HASH_XXH3_64, seed, device, native_ctx)

    @staticmethod
    def new_hasher128(seed=DEFAULT_SEED, device=0, native_ctx=None):
        """the streaming 128-bit hasher (XxHash3Native.newHasher128); digest() returns an XxHash128"""
        return HipStreamHasher(HASH_XXH3_128, seed, device, native_ctx)

    def _one(self, fn, words, input, offset, length, seed):
        view = np.frombuffer(input, dtype=np.uint8)
        if length is None:
            length = view.size - offset
        _check_from_index_size(view, offset, length)
        src = view[offset:offset + length]
        out = (ctypes.c_int64 * words)()
        r = fn(self.native.ctx, src.ctypes.data if src.size else None, int(src.size), ctypes.c_int64(_as_signed(seed, 64)), out)
        if r < 0:
            native.raise_for_status(r)
        return [int(v) for v in out]

    def hash(self, input, offset=0, length=None, seed=DEFAULT_SEED):
        return self._one(self._lib.achip_xxhash3_64, 1, input, offset, length, seed)[0]

    def hash128(self, input, offset=0, length=None, seed=DEFAULT_SEED):
        return XxHash128(*self._one(self._lib.achip_xxhash3_128, 2, input, offset, length, seed))

    def _batch(self, fn, src_base, src_off, src_len, out_hash, n_buffers, seed):
        p = lambda x: ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))  # noqa: E731
        r = fn(self.native.ctx, p(src_base), p(src_off), p(src_len), ctypes.c_int64(_as_signed(seed, 64)), p(out_hash), int(n_buffers))
        if r < 0:
            native.raise_for_status(r)

    def hash_batch(self, src_base, src_off, src_len, out_hash, n_buffers, seed=DEFAULT_SEED):
        """device pointers (ints or objects with data_ptr()); out_hash holds n_buffers int64"""
        self._batch(self._lib.achip_xxhash3_64_batch, src_base, src_off, src_len, out_hash, n_buffers, seed)

    def hash128_batch(self, src_base, src_off, src_len, out_hash, n_buffers, seed=DEFAULT_SEED):
        """device pointers (ints or objects with data_ptr()); out_hash holds 2 * n_buffers int64 (low, high per buffer)"""
        self._batch(self._lib.achip_xxhash3_128_batch, src_base, src_off, src_len, out_hash, n_buffers, seed)


__all__ = ["XxHash64HipHasher", "XxHash32HipHasher", "XxHash3HipHasher", "XxHash128", "HipStreamHasher", "HipHashStates",
           "HASH_XXH32", "HASH_XXH64", "HASH_XXH3_64", "HASH_XXH3_128", "DEFAULT_SEED", "IllegalArgumentException"]
