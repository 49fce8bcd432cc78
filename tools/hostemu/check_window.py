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

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib  # noqa: E402
from emu_harness import run_windows  # noqa: E402
from tests import oracle_lib, window_cases as cases  # noqa: E402

emu = emulib.load("window")
_vp, _i32 = ctypes.c_void_p, ctypes.c_int32
emu.emu_window.argtypes = [_i32, _i32, _i32] + [_vp] * 10 + [_i32] + [_vp] * 3


def run(fmt, compress, buffer_size, windows, flags, caps):
    op = (cases.COMPRESS_OP if compress else cases.DECOMPRESS_OP)[fmt]
    return run_windows(lambda *a: emu.emu_window(op, buffer_size, 2, *a), windows, flags, caps)


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
