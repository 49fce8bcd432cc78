"""Runs the streaming hashers' kernels (xxhash_stream.hip) on the CPU under the fiber emulator (tools/hostemu/libemu_xxh_stream.so:
tools/hostemu/build.sh xxh_stream) over the plans of tests/xxh_stream_cases.py -- the cases of the GPU tests -- and compares every digest
with the one-shot references (tests/xxh3_ref.py for XXH3, the oracle's xxh64 / xxh32 through tests/oracle_lib.py): every total and first
cut, the stream's block boundaries, dribbles, uneven pieces in batches large enough that a wavefront looks after several states, and
sub-ranges reset with different seeds.  `--quick` runs a smaller set."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib  # noqa: E402
from tests import xxh_stream_cases as C  # noqa: E402

emu = emulib.load("xxh_stream")
_vp, _i32 = ctypes.c_void_p, ctypes.c_int32
emu.emu_hash_state_size.restype = ctypes.c_longlong
emu.emu_hash_state_size.argtypes = [_i32]
emu.emu_hash_states_reset.argtypes = [_i32, _vp, _i32, ctypes.c_uint64]
emu.emu_hash_states_update.argtypes = [_i32, _vp, _vp, _vp, _vp, _i32]
emu.emu_hash_states_digest.argtypes = [_i32, _vp, _vp, _i32]


class EmuBackend(C.Backend):
    """host memory (numpy buffers kept alive by address) and the emulated launchers"""

    def __init__(self):
        self.live = {}

    def alloc(self, nbytes):
        a = np.zeros(nbytes, dtype=np.uint8)
        self.live[a.ctypes.data] = a
        return a.ctypes.data

    def free(self, p):
        del self.live[p]

    def h2d(self, p, array):
        ctypes.memmove(p, array.ctypes.data, array.nbytes)

    def d2h(self, array, p):
        ctypes.memmove(array.ctypes.data, p, array.nbytes)

    def state_size(self, algo):
        return emu.emu_hash_state_size(algo)

    def reset(self, algo, states, n, seed):
        assert emu.emu_hash_states_reset(algo, states, n, seed & C.M64) == 0

    def update(self, algo, states, src, off, ln, n):
        assert emu.emu_hash_states_update(algo, states, src, off, ln, n) == 0

    def digest(self, algo, states, out, n):
        assert emu.emu_hash_states_digest(algo, states, out, n) == 0


def main():
    quick = "--quick" in sys.argv
    be = EmuBackend()
    bad = total = 0

    def run(name, algo, plan, seed, **kw):
        nonlocal bad, total
        t0 = time.time()
        wrong = C.run_plan(be, algo, plan, seed, **kw)
        if "--times" in sys.argv:
            print("%s %s: %d states, %.1f s" % (name, C.ALGO_NAMES[algo], len(plan), time.time() - t0))
        total += len(plan)
        bad += len(wrong)
        for i, r, absorbed in wrong[:5]:
            print("MISMATCH %s %s seed=%d state=%d (start %d, total %d, cuts %s) round=%d absorbed=%d" % ((name, C.ALGO_NAMES[algo], seed, i) + plan[i][:2] + (plan[i][2][:6], r, absorbed)))

    for algo in C.ALGOS:
        if quick:
            run("small", algo, C.small_plan(totals=range(0, 601, 7)), -1, packed=True)
            run("small", algo, C.small_plan(totals=[240, 241, 256, 257, 320, 600]), 0x9E3779B185EBCA87, packed=True, misalign=1)
            run("boundary", algo, C.boundary_plan(ks=(1, 3), ds=(-65, -64, -1, 0, 1, 63, 64, 65)), 0x9E3779B185EBCA8D)
            run("dribble", algo, C.dribble_plan(330), 7)
            run("dribble", algo, C.dribble_plan(150, (1, 2, 3, 4, 5, 6, 7)), 7)
            run("uneven", algo, C.uneven_plan(300, 3), -7)
        else:
            for seed in C.SEEDS:
                run("small", algo, C.small_plan(), seed, packed=True, misalign=seed & 7)
            run("boundary", algo, C.boundary_plan(), 0x9E3779B185EBCA8D)
            run("dribble", algo, C.dribble_plan(700), 7)
            run("dribble", algo, C.dribble_plan(700, (1, 2, 3, 4, 5, 6, 7)), 7)
            run("uneven", algo, C.uneven_plan(2000, 3), -7)
        # a batch in which a wavefront of the XXH3 update looks after several states (from 16 384 states on)
        # (--quick: XXH3-64 shares the update with XXH3-128 and sits this one out; the fibers of 8 000 wavefronts take a while)
        if not (quick and algo == C.XXH3_64):
            run("uneven", algo, C.uneven_plan(16500, 4, (0, 5, 100, 241, 257, 300, 1100)) if quick else C.uneven_plan(20000, 4), -7, digest_every_round=False)
        b, t = C.seeds_per_half(be, algo)
        bad += b
        total += t
    print("xxh stream emulator: %d states, %d wrong" % (total, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
