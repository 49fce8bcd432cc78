"""The `_accel` kernels of lz4_compress.hip -- the LZ4 encoders with the search schedule of Lz4Compressor.create(acceleration) -- on the CPU under the fiber emulator
(tools/hostemu/libemu_lz4_accel.so: tools/hostemu/build.sh lz4_accel), bytes, lengths and statuses against the pure-Python model tests/lz4_accel_ref.py: serial
probes, batch probes and the window encoder with uint16_t and int32_t tables, the two-tier arrangement with a grid of two workgroups, the max_src_len_hint launch
and the frame writer.  The correctness argument for the masked replay (lz4_compress_mw.h) that needs no GPU.

  check_lz4_accel.py [--quick]     --quick: accelerations 2, 7 and 64 and a few KiB of text (seconds); without it every acceleration of the GPU test and that test's
                                   own 64 KiB blocks (a fiber switch per memory access and lane: about twenty minutes)"""
import os
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib  # noqa: E402
from emu_harness import EmuBatch  # noqa: E402
from tests import lz4_accel_cases as cases, lz4_accel_ref as ref  # noqa: E402

emu = emulib.load("lz4_accel")
quick = "--quick" in sys.argv
BAD_HINT = -(3 + 16 * 102)  # INVALID_ARGUMENT / ACHIP_D_BAD_ARGUMENT


class AccelBatch(EmuBatch):
    def __init__(self, frame, variant, mem_waves, acceleration, hint=0):
        self.options = {}
        self.args = (variant, mem_waves, hint, acceleration)
        self.frame = frame

    def _call(self, op, *batch):
        return emu.emu_lz4_accel(self.frame, *batch, *self.args)


def inputs():
    """the shapes of tests/lz4_accel_cases.py at sizes the emulator finishes in seconds"""
    a = cases.alice()
    text = 4000 if quick else 9000
    blocks = [("text", a[:text]), ("random 8 KiB", cases.noise(8192)), ("random 200 KiB", cases.noise(200000, 12)),
              ("text + random + text", a[:1500] + cases.noise(3000, 13) + a[1500:3000]), ("zeros 5000", bytes(5000)),
              ("beyond 64 KiB: the wide table", (a[:1200] * 60)[:66000]), ("empty", b""), ("one byte", b"x"), ("twelve bytes", a[100:112])]
    blocks += [(n, d) for n, d in cases.block_cases() if n.startswith("only repeat")]
    if not quick:  # ... and the GPU test's own blocks, whole
        blocks += [(n, d) for n, d in cases.block_cases() if "KiB" in n or n.startswith("text")]
    return blocks


def compare(title, batch, blocks, want, caps=None, want_status=None):
    t = time.time()
    caps = caps or [ref.max_compressed_length(len(d)) for _, d in blocks]
    outs, status, _ = batch.run(0, [d for _, d in blocks], caps, unaligned=True)
    bad = 0
    for i, ((name, d), c, s) in enumerate(zip(blocks, outs, status)):
        ws = want_status[i] if want_status else 0
        if s != ws or (ws == 0 and c != want[i]):
            bad += 1
            print("  MISMATCH %s: %s (%d bytes): status %d / %d, %d bytes / %d" % (title, name, len(d), s, ws, len(c), len(want[i])))
    print("%-72s %4d items %8d bytes  %d wrong  (%.0f s)" % (title, len(blocks), sum(len(d) for _, d in blocks), bad, time.time() - t), flush=True)
    return bad


def main():
    bad = checks = 0
    blocks = inputs()
    forms = (("serial probes", 0, 0), ("batch probes", 1, 0), ("window", 4, 0), ("window, two tiers, one memory wavefront", 4, 1), ("window, two tiers, two memory wavefronts", 4, 2))
    for a in ((2, 7, 64) if quick else (2, 3, 4, 7, 8, 16, 63, 64, 65, 1000, 65537)):
        want = [ref.compress(d, a) for _, d in blocks]
        limits = cases.limit_cases(a) if a in cases.LIMIT_ACCELERATIONS else []
        want_limits = [ref.compress(d, a) for _, d in limits]
        for what, variant, mem_waves in forms:
            bad += compare("acceleration %d, %s" % (a, what), AccelBatch(0, variant, mem_waves, a), blocks + limits, want + want_limits)
            checks += len(blocks) + len(limits)
        # max_src_len_hint = 65536 with a longer block in the batch: the narrow launch alone, the long block gets its status
        some = [blocks[0], blocks[5], blocks[4]]
        st = [0, BAD_HINT, 0]
        for what, variant, mem_waves in (forms[2], forms[3]):
            bad += compare("acceleration %d, %s, hint 65536" % (a, what), AccelBatch(0, variant, mem_waves, a, hint=65536), some, [want[0], b"", want[4]], want_status=st)
            checks += 3
        frames = [blocks[0], blocks[1], blocks[4], blocks[6], blocks[7], ("text, twice", blocks[0][1] * 2)]
        bad += compare("acceleration %d, frame writer" % a, AccelBatch(1, 0, 0, a), frames, [ref.compress_frame(d, a) for _, d in frames],
                       caps=[ref.max_compressed_length(len(d)) + 15 for _, d in frames])
        checks += len(frames)
    print("lz4 acceleration emulator: %d items, %d wrong" % (checks, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
