"""Runs the window kernels of the chunked containers (achip_window_*: hadoop_streams.hip, snappy_frame.hip) on the CPU under the fiber emulator
(tools/hostemu/libemu_window.so: tools/hostemu/build.sh window) against the model of tests/window_cases.py, which is built from the oracle's one-shot readers and
writers: every cut of every case stream, the standard loop driven to the end, the writers cut at fixed positions.  The way to develop these kernels on a machine
without a GPU.  `--quick`: cuts up to two units behind a window's start, a fifth of the writers' cut positions, and the x-snappy-framed writer left out (its
blocks are 64 KiB: minutes under the emulator).  The writers' outputs are compared block length by block length, not byte for byte: under soft order points the block encoders do not run as on
the device (tools/hostemu/check_enc.py runs them exactly, in a library of its own), so what is checked here is the window plan; the GPU test compares bytes.  The listed chunks take the two-pass decoders here (variant 2: the ring decoders at 4 lanes per chunk lean on the
hardware's in-order memory pipeline and do not run under the emulator)."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import oracle_lib, window_cases as cases  # noqa: E402

emu = ctypes.CDLL(os.path.join(ROOT, "tools", "hostemu", os.environ.get("HOSTEMU_LIB", "libemu_window.so")))
_vp, _i32 = ctypes.c_void_p, ctypes.c_int32
emu.emu_window.argtypes = [_i32, _i32, _i32] + [_vp] * 10 + [_i32] + [_vp] * 3
PREFILL = 0xA5


def run(fmt, compress, buffer_size, windows, flags, caps):
    n = len(windows)
    src_len = np.array([len(w) for w in windows], dtype=np.int32)
    src_off = np.zeros(n, dtype=np.int64)
    dst_off = np.zeros(n, dtype=np.int64)
    dst_cap = np.array(caps, dtype=np.int32)
    pos = 64
    for i, w in enumerate(windows):
        src_off[i] = pos
        pos += len(w) + 3
    src = np.full(pos + 64, 0x5A, dtype=np.uint8)
    for i, w in enumerate(windows):
        src[src_off[i]:src_off[i] + len(w)] = np.frombuffer(bytes(w), dtype=np.uint8)
    pos = 64
    for i, c in enumerate(caps):
        dst_off[i] = pos
        pos += c + 16
    dst = np.full(pos + 64, PREFILL, dtype=np.uint8)
    fl = np.array(flags, dtype=np.int32)
    out_len = np.full(n, -7, dtype=np.int32)
    status = np.full(n, -7, dtype=np.int32)
    stop = np.full(n, -7, dtype=np.int32)
    err = np.full(n, -7, dtype=np.int64)
    consumed = np.full(n, -7, dtype=np.int64)
    need = np.full(n, -7, dtype=np.int64)
    op = (cases.COMPRESS_OP if compress else cases.DECOMPRESS_OP)[fmt]
    P = lambda a: a.ctypes.data
    r = emu.emu_window(op, buffer_size, 2, P(fl), P(src), P(src_off), P(src_len), P(dst), P(dst_off), P(dst_cap), P(out_len), P(status), P(err), n, P(consumed), P(stop), P(need))
    assert r == 0, r
    for i in range(n):
        hi = dst_off[i + 1] if i + 1 < n else len(dst)
        assert (dst[dst_off[i] + caps[i]:hi] == PREFILL).all(), "window %d: wrote beyond its capacity" % i
    return [{"consumed": int(consumed[i]), "out": dst[dst_off[i]:dst_off[i] + max(int(out_len[i]), 0)].tobytes(), "stop": int(stop[i]), "need": int(need[i]),
             "status": int(status[i]), "err": int(err[i])} for i in range(n)]


def main():
    """check_window.py [--quick] [--part cuts|drive|writers] [--format snappyframed|lz4hadoop|snappyhadoop]: all parts and formats unless named"""
    quick = "--quick" in sys.argv
    part = sys.argv[sys.argv.index("--part") + 1] if "--part" in sys.argv else None
    only = sys.argv[sys.argv.index("--format") + 1] if "--format" in sys.argv else None
    o = oracle_lib.load()
    chosen = [c for c in cases.all_cases(o) if only in (None, c.fmt)]
    formats = [f for f in (cases.FORMATS[1:] if quick else cases.FORMATS) if only in (None, f)]
    checks = {"cuts": ("every cut", lambda: cases.check_every_cut(run, o, chosen, quick)), "drive": ("drive to the end", lambda: cases.check_drive(run, o, chosen)),
              "writers": ("writers", lambda: cases.check_writers(run, o, quick, formats=formats, same=cases.same_blocks))}
    bad = 0
    for key, (name, check) in checks.items():
        if part not in (None, key):
            continue
        total, wrong = check()
        for w in wrong[:12]:
            print("WINDOW MISMATCH (%s): %s" % (name, w))
        print("window emulator, %s: %d checks, %d wrong" % (name, total, len(wrong)))
        bad += len(wrong)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
