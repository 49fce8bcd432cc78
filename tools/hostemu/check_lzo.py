"""The LZO kernels (lzo_decompress.hip, lzo_compress.hip, the LZO line of decoded_size.hip) on the CPU under the fiber emulator (tools/hostemu/libemu_lzo_r.so,
libemu_lzo_w.so: tools/hostemu/build.sh lzo), the whole catalog of tests/lzo_cases.py against the pure-Python model tests/lzo_ref.py -- bytes, lengths,
statuses and error offsets:

    lzo_parse2_kernel + the record executor       lzo_decompress_wave_kernel alone       the hand-over of an exhausted arena (a tiny maxChunks)
    the sizing kernel                             the encoder                            the decode paths at four destination misalignments

  check_lzo.py [--quick]     --quick: without the ~4 MiB long-run item and with the encoder's inputs up to 6 000 bytes (the encoder's library switches fibers at
                             every memory access: its 50 KB inputs take minutes)"""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib  # noqa: E402
from emu_harness import Layout, P  # noqa: E402
from tests import lzo_cases as cases, lzo_ref as ref  # noqa: E402

quick = "--quick" in sys.argv
dec = emulib.load("lzo_r")
enc = emulib.load("lzo_w", env=False)
MALFORMED = -(1 + 16 * 111)
MAX_OUTPUT = -(2 + 16 * 113)
total = wrong = 0


def report(title, n, bad, t):
    global total, wrong
    total += n
    wrong += bad
    print("%-78s %5d items  %d wrong  (%.0f s)" % (title, n, bad, time.time() - t), flush=True)


def decode_runs(with_long):
    """[(label, stream, capacity, expected)]: every case with exact and with generous room"""
    out = []
    for case in cases.decode_cases() + ([cases.long_run_case()] if with_long else []):
        for cap, exp in cases.runs(case):
            out.append((case[0], case[1], cap, exp))
    return out


def check_decode(title, variant, runs, max_chunks=0, lead=64, want_fallback=None):
    t = time.time()
    lay = Layout([r[1] for r in runs], [r[2] for r in runs], lambda i, n: i % 7, lambda i, c: 16 + (i % 5), src_lead=61 + lead % 4, dst_lead=lead)
    fb = ctypes.c_int32(-1)
    r = dec.emu_lzo_decode(variant, *lay.args(), max_chunks, ctypes.byref(fb))
    assert r == 0, r
    lay.check_guards()
    bad = 0
    for i, ((label, stream, cap, exp), got) in enumerate(zip(runs, lay.outputs())):
        st, eo = int(lay.status[i]), int(lay.err[i])
        ok = (st == 0 and got == exp[1]) if exp[0] == "ok" else (st == MALFORMED and eo == exp[1] and int(lay.out_len[i]) == 0)
        if not ok:
            bad += 1
            print("  MISMATCH %s: %s (capacity %d): status %d offset %d length %d, the model: %s %s" %
                  (title, label, cap, st, eo, int(lay.out_len[i]), exp[0], exp[1] if exp[0] != "ok" else len(exp[1])))
    if want_fallback is not None and not want_fallback(fb.value):
        bad += 1
        print("  MISMATCH %s: %d items were handed to the wavefront decoder" % (title, fb.value))
    report(title + (" [%d handed over]" % fb.value if variant == 1 else ""), len(runs), bad, t)


def check_size(streams):
    t = time.time()
    lay = Layout(streams, [0] * len(streams), lambda i, n: i % 5, lambda i, c: 0)
    size = np.full(lay.n, -7, dtype=np.int64)
    r = dec.emu_lzo_size(P(lay.src), P(lay.src_off), P(lay.src_len), P(size), P(lay.status), P(lay.err), lay.n)
    assert r == 0, r
    bad = 0
    for i, s in enumerate(streams):
        try:
            want = (ref.decoded_size(s), 0, 0)
        except ref.Malformed as e:
            want = (0, MALFORMED, e.offset)
        got = (int(size[i]), int(lay.status[i]), int(lay.err[i]))
        if got != want:
            bad += 1
            print("  MISMATCH size: item %d: %s, the model: %s" % (i, got, want))
    report("the sizing kernel", len(streams), bad, t)


def check_encode():
    t = time.time()
    inputs = [(label, data) for label, data, _ in cases.encode_cases() if not quick or len(data) <= 6000]
    want = [ref.compress(d) for _, d in inputs]
    caps = [ref.max_compressed_length(len(d)) for _, d in inputs]
    inputs += [("one byte short of the bound", inputs[5][1]), ("empty, fifteen bytes of room", b"")]
    want += [b"", b""]
    caps += [caps[5] - 1, 15]
    lay = Layout([d for _, d in inputs], caps, lambda i, n: i % 3, lambda i, c: 16 + i % 4)
    r = enc.emu_lzo_encode(*lay.args())
    assert r == 0, r
    lay.check_guards()
    bad = 0
    for i, ((label, d), got) in enumerate(zip(inputs, lay.outputs())):
        ws = MAX_OUTPUT if i >= len(inputs) - 2 else 0
        if int(lay.status[i]) != ws or got != want[i]:
            bad += 1
            print("  MISMATCH encode: %s (%d bytes): status %d / %d, %d bytes / %d" % (label, len(d), int(lay.status[i]), ws, len(got), len(want[i])))
    report("lzo_compress_kernel", len(inputs), bad, t)


def main():
    runs = decode_runs(False)
    everything = runs if quick else decode_runs(True)
    # 64 items fill a parser wavefront: the catalog is more than that, so wavefronts with idle lanes and full ones both occur
    check_decode("lzo_parse2_kernel + executor", 1, everything, want_fallback=lambda n: n <= (0 if quick else 2))
    check_decode("lzo_decompress_wave_kernel", 2, everything)
    check_decode("two passes, an arena of 24 chunks", 1, runs, max_chunks=24, want_fallback=lambda n: n > 0)
    for lead in (65, 66, 67):
        check_decode("two passes, destination misaligned by %d" % (lead % 4), 1, runs, lead=lead)
        check_decode("a wavefront per item, destination misaligned by %d" % (lead % 4), 2, runs, lead=lead)
    check_size([r[1] for r in everything if r[2] != 0][::2])
    check_encode()
    print("lzo emulator: %d items, %d wrong" % (total, wrong))
    return 1 if wrong else 0


if __name__ == "__main__":
    sys.exit(main())
