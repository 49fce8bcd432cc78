"""Runs the catalog of LZ4 frames with linked blocks (tests/lz4_linked_cases.py) through lz4frame_decompress_kernel (libemu_serial.so: the wavefront-per-item
kernel of lz4_frame.hip, the history-aware block decoder of lz4_decode_body.h over Rings::prime_history) and through the LZ4FRAME line of the sizing kernels
(libemu_size.so: decoded_size.hip) on the CPU under the fiber emulator, against the model (tests/lz4_linked_ref.py): with the setting on and off, at four
destination misalignments (the rings' outBase 0 .. 3; the source moves along).

    decode   bytes, outLen, status and errOffset of every item are the model's; with the setting off every linked case is ACHIP_D_LZ4F_LINKED_BLOCKS at its
             descriptor; nothing is written in front of an item's dstOff or behind its capacity (canaries)
    size     R1: an item the model decodes is sized exactly; R2: a size reported for any other item is never one the model decodes it to with that capacity
             -- a fault is reported at the model's status where the fault is the container's; with the setting off: the descriptor's refusal

The way to develop the reader on a machine without a GPU.  `--part decode|size` runs one of the two."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib  # noqa: E402
from tests import lz4_linked_cases as cat, lz4_linked_ref as ref  # noqa: E402

_vp, _i32 = ctypes.c_void_p, ctypes.c_int32
CANARY = 0xA5
GAP = 48  # canary bytes between items


def layout(items, caps, shift):
    """the batch's arrays: sources and destinations `shift` bytes off a 16-byte boundary, GAP canary bytes around every destination"""
    src_off, dst_off, sp, dp = [], [], 16 + shift, 64 + shift
    for data, cap in zip(items, caps):
        src_off.append(sp)
        sp += (len(data) + 15) // 16 * 16 + 16
        dst_off.append(dp)
        dp += (cap + GAP + 15) // 16 * 16
    src = np.zeros(sp + 64, dtype=np.uint8)
    for data, so in zip(items, src_off):
        src[so:so + len(data)] = np.frombuffer(data, dtype=np.uint8)
    dst = np.full(dp + 64, CANARY, dtype=np.uint8)
    return src, np.array(src_off, dtype=np.int64), np.array([len(d) for d in items], dtype=np.int32), dst, np.array(dst_off, dtype=np.int64), np.array(caps, dtype=np.int32)


def check_decode(cases):
    emu = emulib.load("serial")
    emu.emu_lz4frame_serial_linked.argtypes = [_vp] * 9 + [_i32, _i32]
    checks = wrong = 0
    for accept in (1, 0):
        want = [ref.decompress(c.data, c.cap, bool(accept)) for c in cases]
        for shift in range(4):
            src, so, sl, dst, do, dc = layout([c.data for c in cases], [c.cap for c in cases], shift)
            n = len(cases)
            out_len, status, err = np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int64)
            r = emu.emu_lz4frame_serial_linked(src.ctypes.data, so.ctypes.data, sl.ctypes.data, dst.ctypes.data, do.ctypes.data, dc.ctypes.data, out_len.ctypes.data,
                                               status.ctypes.data, err.ctypes.data, n, accept)
            assert r == 0, r
            covered = np.zeros(len(dst), dtype=bool)
            for k, (c, w) in enumerate(zip(cases, want)):
                checks += 1
                at = int(do[k])
                covered[at:at + c.cap] = True
                got = (int(status[k]), int(err[k]), int(out_len[k]), dst[at:at + max(int(out_len[k]), 0)].tobytes())
                problems = [] if got == (w.status, w.offset, len(w.out), w.out) else ["status %d offset %d length %d, want %d / %d / %d%s" % (
                    got[0], got[1], got[2], w.status, w.offset, len(w.out), "" if got[3] == w.out or got[0] != 0 else " -- bytes differ")]
                if not accept and c.linked and (w.status, w.offset) != (ref.malformed(ref.D_LINKED_BLOCKS), cat.linked_descriptor(c)):
                    problems.append("the model itself does not refuse it at the descriptor")
                if problems:
                    wrong += 1
                    print("DECODE accept=%d shift=%d %s: %s" % (accept, shift, c.name, "; ".join(problems)))
            checks += 1
            if not (dst[~covered] == CANARY).all():  # in front of the first item, between items, behind the last
                wrong += 1
                print("DECODE accept=%d shift=%d: bytes outside the items' capacities were written at %s" % (accept, shift, np.nonzero((dst != CANARY) & ~covered)[0][:8].tolist()))
    print("lz4 linked emulator, decode: %d checks, %d wrong" % (checks, wrong))
    return wrong


def check_size(cases):
    emu = emulib.load("size", env=False)
    emu.emu_lz4frame_size_linked.argtypes = [_vp] * 6 + [_i32, _i32]
    checks = wrong = 0
    for accept in (1, 0):
        for shift in range(4):
            src, so, sl, _, _, _ = layout([c.data for c in cases], [c.cap for c in cases], shift)
            n = len(cases)
            size, status, err = np.full(n, -7, dtype=np.int64), np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int64)
            r = emu.emu_lz4frame_size_linked(src.ctypes.data, so.ctypes.data, sl.ctypes.data, size.ctypes.data, status.ctypes.data, err.ctypes.data, n, accept)
            assert r == 0, r
            for k, c in enumerate(cases):
                checks += 1
                s, z, e = int(status[k]), int(size[k]), int(err[k])
                roomy = ref.decompress(c.data, max(c.cap, z if s == 0 else 0) + 64, bool(accept))  # what the reader makes of the item when room is no question
                if not accept and c.linked:
                    problem = None if (s, e) == (ref.malformed(ref.D_LINKED_BLOCKS), cat.linked_descriptor(c)) else "status %d offset %d: not the descriptor's refusal" % (s, e)
                elif roomy.status == 0:  # R1
                    problem = None if (s, z) == (0, len(roomy.out)) else "status %d size %d, the item decodes to %d bytes" % (s, z, len(roomy.out))
                elif s == 0:  # R2: the walk leaves checks out (checksums, offsets), but a size it reports is not a wrong one
                    exact = ref.decompress(c.data, z, bool(accept))
                    problem = "size %d, and the item decodes to %d bytes at that capacity" % (z, len(exact.out)) if exact.status == 0 and len(exact.out) != z else None
                else:  # R3: a reported fault is the reader's fault
                    problem = None if (s, e) == (roomy.status, roomy.offset) else "status %d offset %d, the reader fails with %d at %d" % (s, e, roomy.status, roomy.offset)
                if problem:
                    wrong += 1
                    print("SIZE accept=%d shift=%d %s: %s" % (accept, shift, c.name, problem))
    print("lz4 linked emulator, size: %d checks, %d wrong" % (checks, wrong))
    return wrong


def main():
    part = sys.argv[sys.argv.index("--part") + 1] if "--part" in sys.argv else "all"
    cases = cat.cases()
    wrong = 0
    if part in ("all", "decode"):
        wrong += check_decode(cases)
    if part in ("all", "size"):
        wrong += check_size(cases)
    return 1 if wrong else 0


if __name__ == "__main__":
    sys.exit(main())
