"""Runs the bound kernel, the pack scan and the dense copy (pack_outputs.hip) on the CPU under the fiber emulator (tools/hostemu/libemu_pack.so:
tools/hostemu/build.sh pack) against numpy and the library's host bound functions, over the cases of tests/pack_cases.py (the GPU test's generator): the way to
develop the kernels on a machine without a GPU.  `--quick`: the same shapes at a tenth of the size.  HOSTEMU_LIB names another build of emu_pack.cpp to load
(one with -fsanitize=address, under the sanitizer's runtime as tools/hostemu/run_asan_fuzz.sh sets it up: the numpy buffers are exact, so a read or write past an
item or past the stream lands in a red zone)."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib  # noqa: E402
from tests import pack_cases as cases  # noqa: E402

emu = emulib.load("pack")
_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
emu.emu_pack_tile_bytes.restype = ctypes.c_longlong
emu.emu_compress_bound.argtypes = [_i32, _vp, _vp, _vp, _i32, _i32]
emu.emu_pack_outputs.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _vp]
TILE = int(emu.emu_pack_tile_bytes())


def _p(a):
    return None if a is None else a.ctypes.data


def check_bounds(lib):
    bad = checks = 0
    lengths = np.array(cases.BOUND_LENGTHS + list(range(250, 262)) * 30, dtype=np.int32)  # (more than one workgroup)
    for name, op in cases.COMPRESS_OPS.items():
        for buffer_size in ((cases.HADOOP_DEFAULT_BUFFER, cases.HADOOP_OTHER_BUFFER) if "hadoop" in name else (cases.HADOOP_DEFAULT_BUFFER,)):
            size = np.full(len(lengths), -7, dtype=np.int64)
            status = np.full(len(lengths), -7, dtype=np.int32)
            assert emu.emu_compress_bound(op, _p(lengths), _p(size), _p(status), len(lengths), buffer_size) == 0
            wrong = cases.check_bounds(lib, name, lengths, size, status, lib.achip_status_class, buffer_size)
            checks += len(lengths)
            bad += len(wrong)
            for w in wrong[:5]:
                print("BOUND MISMATCH", w)
    return checks, bad


def run_pack(case, align, use_raw, cap_delta=0, plan_only=False, dst_shift=0):
    """-> mismatches (a list of words) of one emulated call against case.expect"""
    want_total = case.expect(align, use_raw)[3]
    cap = want_total + cap_delta
    buf = np.full(max(cap, 0) + cases.GUARD + 32, cases.PREFILL, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data % 16) + dst_shift  # the destination's address mod 16 is dst_shift
    at = base - buf.ctypes.data
    off = np.full(case.n, -7, dtype=np.int64)
    ln = np.full(case.n, -7, dtype=np.int32)
    stored = np.full(case.n, -7, dtype=np.int32) if use_raw else None
    total = np.full(3, -7, dtype=np.int64)
    raw = (case.raw, case.raw_off, case.raw_len) if use_raw else (None, None, None)
    r = emu.emu_pack_outputs(_p(case.src), _p(case.src_off), _p(case.out_len), _p(case.status), _p(raw[0]), _p(raw[1]), _p(raw[2]), case.n, align,
                             None if plan_only else base, cap, _p(off), _p(ln), _p(stored), _p(total))
    wrong = ["return %d" % r] if r != 0 else []
    wrong += cases.mismatches(case, align, use_raw, not plan_only and cap_delta >= 0, buf, at, off, ln, stored, total)
    return wrong


def check_packs(quick):
    bad = checks = 0

    def one(what, wrong):
        nonlocal bad, checks
        checks += 1
        if wrong:
            bad += 1
            print("PACK MISMATCH %s: %s" % (what, ", ".join(wrong)))

    for align in cases.ALIGNS:
        sets = cases.pack_cases(TILE, align, quick)
        for c in sets:
            one("%s align %d" % (c.name, align), run_pack(c, align, False))
        b = sets[1]
        one("b align %d, one byte too small" % align, run_pack(b, align, False, cap_delta=-1))
        one("b align %d, plan only" % align, run_pack(b, align, False, plan_only=True))
        one("b align %d, room to spare" % align, run_pack(b, align, False, cap_delta=TILE + 5))
        for shift in (1, 9, 15):  # a destination that is not 16-byte aligned: the tiles are cut by address
            one("b align %d, destination address mod 16 = %d" % (align, shift), run_pack(b, align, False, dst_shift=shift))
        b.with_raw(np.random.default_rng(5 + align))
        one("b align %d, keep the smaller" % align, run_pack(b, align, True))
        one("d align %d, keep the smaller" % align, run_pack(sets[3].with_raw(np.random.default_rng(6)), align, True))
    return checks, bad


def main():
    quick = "--quick" in sys.argv
    import aircompressor_amd as A
    lib = A.load_library()
    n1, bad1 = check_bounds(lib)
    n2, bad2 = check_packs(quick)
    print("pack emulator: %d bounds, %d pack calls, %d wrong" % (n1, n2, bad1 + bad2))
    return 1 if bad1 + bad2 else 0


if __name__ == "__main__":
    sys.exit(main())
