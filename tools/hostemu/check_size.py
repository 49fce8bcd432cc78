"""Runs the sizing kernels and the output planner (decoded_size.hip) on the CPU under the fiber emulator (tools/hostemu/libemu_size.so: tools/hostemu/build.sh size)
against the oracle: every op's clean items must be sized exactly (R1), seeded damaged items must fall under R1 / R2 / R3 "a reported fault is the reader's fault"
(tests/decoded_size_cases.py has the rules), both LZ4 launch shapes must agree, and the planner must equal a numpy scan.  The way to develop the kernels on a
machine without a GPU.  `--quick`: fewer damaged items, no multi-megabyte items."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib  # noqa: E402
from tests import decoded_size_cases as cases, oracle_lib  # noqa: E402

emu = emulib.load("size")
_vp, _i32 = ctypes.c_void_p, ctypes.c_int32
emu.emu_decoded_size.argtypes = [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32]
emu.emu_lz4_size_shape.argtypes = [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32]
emu.emu_plan_outputs.argtypes = [_vp, _vp, _i32, _i32, _vp, _vp, _vp]


def pack(items, misalign=3):
    offs, pos = [], misalign
    for b in items:
        offs.append(pos)
        pos += len(b) + (len(b) % 5) + 1
    src = np.zeros(pos + 64, dtype=np.uint8)
    for b, so in zip(items, offs):
        src[so:so + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return src, np.array(offs, dtype=np.int64), np.array([len(b) for b in items], dtype=np.int32)


def size(op, items, shape=0):
    src, so, sl = pack(items)
    n = len(items)
    out = np.full(n, -7, dtype=np.int64)
    st = np.full(n, -7, dtype=np.int32)
    eo = np.full(n, -7, dtype=np.int64)
    args = (src.ctypes.data, so.ctypes.data, sl.ctypes.data, out.ctypes.data, st.ctypes.data, eo.ctypes.data, n)
    r = emu.emu_lz4_size_shape(shape, *args) if shape else emu.emu_decoded_size(op, *args)
    assert r == 0, r
    return out, st, eo


def check_planner(rng):
    bad = 0
    for n in (1, 63, 1024, 1025, 300001):
        sizes = rng.integers(0, 70000, n).astype(np.int64)
        status = np.where(rng.integers(0, 10, n) == 0, -33, 0).astype(np.int32)
        sizes[n // 2] = (1 << 31) + 5
        for align in (1, 16, 4096):
            off = np.zeros(n, dtype=np.int64)
            cap = np.zeros(n, dtype=np.int32)
            total = np.zeros(2, dtype=np.int64)
            assert emu.emu_plan_outputs(sizes.ctypes.data, status.ctypes.data, n, align, off.ctypes.data, cap.ctypes.data, total.ctypes.data) == 0
            out = (status != 0) | (sizes > cases.INT32_MAX)
            want_cap = np.where(out, 0, sizes)
            room = (want_cap + align - 1) // align * align
            want_off = np.cumsum(room) - room
            ok = (cap == want_cap).all() and (off == want_off).all() and total[0] == room.sum() and total[1] == out.sum()
            bad += 0 if ok else 1
            if not ok:
                print("PLANNER MISMATCH n=%d align=%d" % (n, align))
    return bad


def main():
    quick = "--quick" in sys.argv
    o = oracle_lib.load()
    bad = total = 0
    for name, op in cases.OPS.items():
        clean = cases.clean_items(o, name, big=not quick)
        got, st, _ = size(op, [c for _, c, _ in clean])
        for (label, comp, n), g, s in zip(clean, got, st):
            total += 1
            assert cases.exact_length(o, name, comp, n + 64) == n, (name, label)  # the set is not hollow
            if s != 0 or g != n:
                bad += 1
                print("CLEAN MISMATCH %s %s: want %d, got status %d size %d" % (name, label, n, s, g))
        if name == "lz4":  # both launch shapes on the same batch
            for shape in (1, 2):
                g2, s2, _ = size(op, [c for _, c, _ in clean], shape)
                if not ((g2 == got).all() and (s2 == st).all()):
                    bad += 1
                    print("LZ4 SHAPE %d differs from the launcher's choice" % shape)
        if name == "zstd":  # every header form the format has (tests/zstd_frame_cases.py), as the GPU test sizes them
            from tests import test_gpu_zstd
            frames, plains = test_gpu_zstd.header_form_items(o)
            got, st, _ = size(op, frames)
            total += len(frames)
            for i, (p, g, s) in enumerate(zip(plains, got, st)):
                if s != 0 or g != len(p):
                    bad += 1
                    print("HEADER FORMS frame %d: want %d, got status %d size %d" % (i, len(p), s, g))
        items = cases.damaged_items(o, name, 100 + op, 120 if quick else 400)
        seen = {"exact": 0, "r2": 0, "fault": 0, "payload": 0}
        for shape in ((0, 1, 2) if name == "lz4" else (0,)):
            got, st, eo = size(op, [d for _, d, _ in items], shape)
            for (kind, d, room), g, s, e in zip(items, got, st, eo):
                total += 1
                category, wrong = cases.judge(o, name, d, room, int(g), int(s), int(e))
                seen[category] += 1
                if wrong:
                    bad += 1
                    print("DAMAGED %s (%s, %d bytes, shape %d): %s" % (name, kind, len(d), shape, wrong))
        wrong = None if quick else cases.payload_share_wrong(name, seen)  # (the share is bounded at the tests' count of items)
        if wrong:
            bad += 1
            print(wrong)
        print("%-13s clean %3d   damaged: %d exact, %d status 0 but undecodable, %d faults the decoder's own (R3), %d more behind a payload fault of its" % (
            name, len(clean), seen["exact"], seen["r2"], seen["fault"], seen["payload"]))
    bad += check_planner(np.random.default_rng(9))
    print("decoded-size emulator: %d checks, %d wrong" % (total, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
