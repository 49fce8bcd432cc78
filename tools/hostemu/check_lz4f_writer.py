"""The block-list LZ4 frame writer of lz4_frame_writer.hip (plan, seal, encode, compact) on the CPU under the fiber emulator (tools/hostemu/libemu_lz4f_writer.so:
tools/hostemu/build.sh lz4f_writer), against the pure-Python model tests/lz4f_writer_ref.py:

  catalog     tests/lz4f_writer_cases.py, a batch per setting at exact capacities, sources and destinations at the four misalignments: bytes, lengths, statuses
  defaults    the block list at the Java writer's settings (lz4frame.compress.variant 1) against the oracle's frame writer
  refusals    a capacity a byte below the bound: OUTPUT_TOO_SMALL with not one byte of the destination written, the item beside it written; a negative length
  small list  a list sealed at a few entries (KernelSettings::lz4fListEntries): the frame whose blocks do not fit is INVALID_ARGUMENT / ACHIP_D_UNSUPPORTED, the
              frames beside it are written -- the only place that path can be tested
  acceleration 7 under non-default settings

  check_lz4f_writer.py [--quick]     --quick: the 64 KiB settings with every flag off and every flag on, inputs of at most two blocks, and one large setting's
                                     B + 1 (the block encoder runs an order point per memory access)"""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib  # noqa: E402
from emu_harness import Layout  # noqa: E402
from tests import lz4f_writer_cases as cases, lz4f_writer_ref as ref, oracle_lib  # noqa: E402

W = emulib.load("lz4f_writer")
_vp, _i32 = ctypes.c_void_p, ctypes.c_int32
W.emu_lz4f_write.argtypes = [_i32] * 6 + [_vp] * 9 + [_i32]
quick = "--quick" in sys.argv


def write(settings, items, caps, list_entries=0, acceleration=1, lengths=None):
    """one launch: items[i] at source misalignment i % 4 and destination misalignment (i // 4) % 4 beyond 16-byte boundaries -> (outputs, statuses, offsets,
    the layout); lengths: srcLen as the kernels see it, where it is not len(items[i])"""
    lay = Layout(items, caps, lambda i, n: -(64 + n) % 16 + 16 + (i + 1) % 4 - i % 4, lambda i, c: -(64 + c) % 16 + 32 + ((i + 1) // 4) % 4 - (i // 4) % 4)
    # (the gaps above keep item i at 64 + 16 k + misalignment: every step restores the boundary and adds the next item's offset)
    if lengths is not None:
        lay.src_len[:] = np.array(lengths, dtype=np.int32)
    r = W.emu_lz4f_write(list_entries, *settings, acceleration, *lay.args())
    assert r == 0, r
    lay.check_guards("frame")
    return lay.outputs(), lay.status.tolist(), lay.err.tolist(), lay


def compare(title, settings, named, want, caps=None, want_status=None, **kw):
    t = time.time()
    if caps is None:
        caps = [ref.max_compressed_length(len(d), *settings) for _, d in named]
    outs, status, err, lay = write(settings, [d for _, d in named], caps, **kw)
    bad = 0
    for i, ((name, d), c, s) in enumerate(zip(named, outs, status)):
        ws = want_status[i] if want_status else 0
        untouched = ws == 0 or (lay.dst[lay.dst_off[i]:lay.dst_off[i] + lay.dst_cap[i]] == lay.prefill).all()
        if s != ws or err[i] != 0 or (ws == 0 and c != want[i]) or (ws != 0 and len(c) != 0) or not untouched:
            bad += 1
            print("  MISMATCH %s: %s (%d bytes): status %d / %d, %d bytes / %d%s" % (title, name, len(d), s, ws, len(c), len(want[i]), "" if untouched else ", destination written"))
    print("%-100s %4d items %9d bytes  %d wrong  (%.0f s)" % (title, len(named), sum(len(d) for _, d in named), bad, time.time() - t), flush=True)
    return bad, len(named)


def emulator_settings():
    by = cases.by_settings()
    if not quick:
        return list(by.items())
    out = [(s, [c for c in cs if len(c.data) <= 65537 or (len(c.data) == 131072 and "/" in c.name.split(" ")[0])]) for s, cs in by.items() if s in ((65536, 0, 0, 0), (65536, 1, 1, 1))]
    out.append(((262144, 1, 1, 1), [c for c in by[(262144, 1, 1, 1)] if len(c.data) == 262145]))
    return out


def main():
    bad = total = 0

    def add(r):
        nonlocal bad, total
        bad, total = bad + r[0], total + r[1]

    o = oracle_lib.load()
    for settings, cs in emulator_settings():
        named = [(c.name, c.data) for c in cs]
        add(compare("catalog: %s" % cases.settings_name(settings), settings, named, [cases.expected(c.name) for c in cs]))
    # the Java writer's settings through the block list: the oracle's frame writer
    d4 = [("zeros 70000", cases.data("zeros", 70000)), ("text 3000", cases.data("text", 3000, 9)), ("empty", b""), ("random 100", cases.data("random", 100)),
          ("text 70001", cases.data("text", 70001, 77))]
    if not quick:
        d4.append(("text 4 MiB + 1", cases.data("text", (4 << 20) + 1, 3)))
    add(compare("defaults through the block list against the oracle's writer", ref.DEFAULT, d4, [o.compress("lz4frame", d) for _, d in d4]))
    # refusals: a byte short beside an item that is written; a negative length
    s = (65536, 1, 1, 1)
    text, zeros = cases.data("text", 65537, 31), cases.data("zeros", 65536 + 20)
    b_text, b_zeros = ref.max_compressed_length(len(text), *s), ref.max_compressed_length(len(zeros), *s)
    add(compare("a byte short", s, [("text 65537", text), ("zeros 65556", zeros), ("empty", b""), ("empty", b"")], [b"", ref.compress(zeros, *s), b"", ref.compress(b"", *s)],
                caps=[b_text - 1, b_zeros, ref.max_compressed_length(0, *s) - 1, ref.max_compressed_length(0, *s)], want_status=[cases.MAX_OUTPUT, 0, cases.MAX_OUTPUT, 0]))
    add(compare("a negative length", s, [("negative", b"abc"), ("zeros 65556", zeros)], [b"", ref.compress(zeros, *s)], caps=[64, b_zeros], want_status=[cases.BAD_ARGUMENT, 0],
                lengths=[-1, len(zeros)]))
    # a list of three entries: two frames of one block fit, the frame of four blocks between them does not
    small = [("text 1000", cases.data("text", 1000, 5)), ("zeros 4 blocks", cases.data("zeros", 3 * 65536 + 5)), ("text 65536", cases.data("text", 65536, 8)), ("text 12", cases.data("text", 12))]
    add(compare("a block list of three entries", s, small, [ref.compress(d, *s) if i != 1 else b"" for i, (_, d) in enumerate(small)], want_status=[0, cases.UNSUPPORTED, 0, 0],
                list_entries=3))
    # acceleration under non-default settings
    acc = [("text 65537", text), ("zeros 65556", zeros), ("random 300", cases.data("random", 300))]
    add(compare("acceleration 7 at %s" % cases.settings_name(s), s, acc, [ref.compress(d, *s, acceleration=7) for _, d in acc], acceleration=7))
    print("lz4 frame writer emulator: %d items, %d wrong" % (total, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
