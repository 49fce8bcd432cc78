"""The streaming hashers without a GPU: the nine symbols are exported, achip_hash_state_size answers as documented, every batch call refuses
bad arguments with the status class achip_xxhash64_batch gives for the same mistake (before any context is touched), and the Python twins
fail loudly where no GPU is visible.  What the kernels compute is checked on the emulator (tests/test_xxh_stream_emu.py) and on the GPU
(tests/test_gpu_xxhash_stream.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["achip_hash_state_size", "achip_hash_states_reset", "achip_hash_states_update", "achip_hash_states_digest",
           "achip_hasher_create", "achip_hasher_update", "achip_hasher_digest", "achip_hasher_reset", "achip_hasher_destroy"]
INVALID_ARGUMENT = 3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library()
    import aircompressor_amd as A
    return A.load_library()


def test_the_nine_symbols_are_exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "aircompressor_amd", "libaircompressor_hip.so")], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (achip_[a-z0-9_]+)", out))
    assert not [s for s in SYMBOLS if s not in exported]
    from aircompressor_amd import native
    assert all(s in native.SIGNATURES for s in SYMBOLS)


def test_state_sizes(lib):
    sizes = [lib.achip_hash_state_size(a) for a in range(4)]
    for n in sizes:
        assert 0 < n < 1024 and n % 16 == 0, sizes
    assert sizes[2] == sizes[3]
    for a in (-1, 4):
        r = lib.achip_hash_state_size(a)
        assert r < 0 and lib.achip_status_class(int(r)) == INVALID_ARGUMENT, (a, r)


def test_batch_calls_refuse_what_xxhash64_batch_refuses(lib):
    z = np.zeros(64, dtype=np.int64)
    p = z.ctypes.data
    one_shot = lambda ctx, arrays, n: lib.achip_xxhash64_batch(ctx, p, p if arrays else None, p if arrays else None, 0, p if arrays else None, n)  # noqa: E731
    cls = lib.achip_status_class
    for algo in range(4):
        calls = {
            "reset": lambda ctx, arrays, n: lib.achip_hash_states_reset(ctx, algo, p if arrays else None, n, 0),
            "update": lambda ctx, arrays, n: lib.achip_hash_states_update(ctx, algo, p if arrays else None, p, p if arrays else None, p if arrays else None, n),
            "digest": lambda ctx, arrays, n: lib.achip_hash_states_digest(ctx, algo, p if arrays else None, p if arrays else None, n),
        }
        for name, call in calls.items():
            # null ctx (with good arrays, with null arrays, with a zero count), negative count: refused as the one-shot batch refuses them.  (A null
            # array with a live context is in tests/test_gpu_xxhash_stream.py: without a GPU there is no context to pass.)
            for ctx, arrays, n in ((None, True, 1), (None, False, 1), (None, True, 0), (None, True, -1), (None, False, -1)):
                got, want = call(ctx, arrays, n), one_shot(ctx, arrays, n)
                assert got < 0 and cls(got) == cls(want) == INVALID_ARGUMENT, (name, algo, arrays, n, got, want)
    for algo in (-1, 4, 1 << 20):  # an unknown algorithm is refused whatever else is passed
        assert cls(lib.achip_hash_states_reset(None, algo, p, 1, 0)) == INVALID_ARGUMENT
        assert cls(lib.achip_hash_states_update(None, algo, p, p, p, p, 1)) == INVALID_ARGUMENT
        assert cls(lib.achip_hash_states_digest(None, algo, p, p, 1)) == INVALID_ARGUMENT


def test_host_hasher_refuses_null(lib):
    for algo in (0, 1, 2, 3, 4, -1):
        assert not lib.achip_hasher_create(None, algo, 0)
    out = (ctypes.c_int64 * 2)()
    assert lib.achip_status_class(lib.achip_hasher_update(None, None, 0)) == INVALID_ARGUMENT
    assert lib.achip_status_class(lib.achip_hasher_digest(None, out)) == INVALID_ARGUMENT
    assert lib.achip_status_class(lib.achip_hasher_reset(None, 0)) == INVALID_ARGUMENT
    assert lib.achip_status_class(lib.achip_hasher_destroy(None)) == INVALID_ARGUMENT


def test_twins_fail_loudly_without_a_gpu(lib):
    import aircompressor_amd as A
    makers = [A.XxHash64HipHasher.create, A.XxHash32HipHasher.create, A.XxHash3HipHasher.new_hasher, A.XxHash3HipHasher.new_hasher128,
              lambda: A.HipHashStates(1, 4)]
    if lib.achip_device_count() > 0:
        for make in makers:  # (a GPU is visible: the objects come up; tests/test_gpu_xxhash_stream.py checks what they compute)
            make().close()
        return
    for make in makers:
        with pytest.raises(A.HipUnavailableError):
            make()
