"""Runs the XXH3 kernels (xxhash3.hip) on the CPU under the fiber emulator (tools/hostemu/libemu_xxh3.so: tools/hostemu/build.sh xxh3) and
compares them with the pure-Python reference (tests/xxh3_ref.py): every length class of both outputs, seeds, misaligned buffers, and a
batch that interleaves short and long buffers across the long kernel's buffer groups.  `--quick` runs a smaller set."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib  # noqa: E402
from tests import xxh3_ref  # noqa: E402

emu = emulib.load("xxh3")
emu.emu_xxh3_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p]
M64 = (1 << 64) - 1


def run(buffers, seed, wide, misalign=3):
    offs, pos = [], misalign
    for b in buffers:
        offs.append(pos)
        pos += len(b) + (len(b) % 7) + 1
    src = np.zeros(pos + 64, dtype=np.uint8)
    for b, so in zip(buffers, offs):
        src[so:so + len(b)] = np.frombuffer(b, dtype=np.uint8)
    so = np.array(offs, dtype=np.int64)
    sl = np.array([len(b) for b in buffers], dtype=np.int32)
    out = np.zeros(len(buffers) * (2 if wide else 1), dtype=np.int64)
    assert emu.emu_xxh3_batch(src.ctypes.data, so.ctypes.data, sl.ctypes.data, len(buffers), seed & M64, int(wide), out.ctypes.data) == 0
    u = [int(v) & M64 for v in out]
    return [(u[2 * i], u[2 * i + 1]) for i in range(len(buffers))] if wide else u


def main():
    quick = "--quick" in sys.argv
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    lengths = list(range(0, 300 if quick else 600, 1 if not quick else 3))
    lengths += [1024 * k + d for k in (1, 2, 3) for d in (-65, -64, -63, -1, 0, 1, 63, 64, 65)] + [4800]
    buffers = [data[i % 11:i % 11 + n] for i, n in enumerate(lengths)]
    bad = total = 0
    for seed in ((0, -1) if quick else (0, 1, -1, 0x9E3779B1, 0x9E3779B185EBCA87)):
        for wide in (False, True):
            got = run(buffers, seed, wide)
            ref = xxh3_ref.xxh3_128 if wide else xxh3_ref.xxh3_64
            for b, g in zip(buffers, got):
                total += 1
                if g != ref(b, seed):
                    bad += 1
                    if bad <= 10:
                        print("MISMATCH len=%d seed=%d wide=%s" % (len(b), seed, wide))
    print("xxh3 emulator: %d / %d hashes equal the reference" % (total - bad, total))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
