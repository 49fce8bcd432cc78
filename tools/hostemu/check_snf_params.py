"""The x-snappy-framed writers and readers of snappy_frame.hip with the parameters of achip_ctx_set_snappyframed_writer / _verify_checksums on the CPU under the fiber
emulator (tools/hostemu/libemu_snf_params_w.so and _r.so: tools/hostemu/build.sh snf_params), against the pure-Python model tests/snf_params_ref.py:

  writers   the catalog of tests/snf_params_cases.py through the wavefront-per-stream kernel (variant 0), the block list (variant 1) and the block list sealed at a
            few entries, so that streams of the same call take the serial kernel behind it; exact capacities, and one capacity a byte short
  windows   the window writer at every cut of a few streams, with ample room and with room for one block: the pieces, one behind the other, are the one-shot
            bytes at the same parameters
  readers   variants 0 .. 3 and the window reader with verify on and off: streams of the catalog, a checksum-free stream, a stream with one damaged CRC field,
            structurally damaged streams (the same status and offset under both settings)

  check_snf_params.py [--quick]     --quick: block sizes up to 64 whole, 4096 with a few inputs (the block encoder runs an order point per memory access)"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib  # noqa: E402
from emu_harness import EmuBatch, run_windows  # noqa: E402
from tests import snf_params_cases as cases, snf_params_ref as ref, window_cases  # noqa: E402

W = emulib.load("snf_params_w")  # (HOSTEMU_LIB: another build of the writers' unit)
R = emulib.load("snf_params_r", env=False)
_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
for lib in (W, R):
    lib.emu_snf_write.argtypes = [_i32, _i32, _i32, _i32, _i64] + [_vp] * 9 + [_i32]
    lib.emu_snf_read.argtypes = [_i32, _i32] + [_vp] * 9 + [_i32]
    lib.emu_snf_window.argtypes = [_i32, _i32, _i32, _i32, _i64, _i32] + [_vp] * 10 + [_i32] + [_vp] * 3
quick = "--quick" in sys.argv
CHECKSUM, MAX_OUTPUT = cases.CHECKSUM, cases.MAX_OUTPUT


class Writer(EmuBatch):
    def __init__(self, variant, list_entries, params):
        self.options = {}
        self.args = (variant, list_entries, int(params[0]), params[1], ref.ratio_bits(params[2]))

    def _call(self, op, *batch):
        return W.emu_snf_write(*self.args, *batch)


class Reader(EmuBatch):
    def __init__(self, variant, verify):
        self.options = {}
        self.args = (variant, int(verify))

    def _call(self, op, *batch):
        return R.emu_snf_read(*self.args, *batch)


def window_run(lib, compress, variant, params, verify):
    """-> run(fmt, compress, buffer_size, windows, flags, caps) as tests/window_cases.py's loops want it"""
    head = (int(compress), variant, int(params[0]), params[1], ref.ratio_bits(params[2]), int(verify))
    return lambda fmt, _compress, _buffer_size, windows, flags, caps: run_windows(lambda *a: lib.emu_snf_window(*head, *a), windows, flags, caps)


def emulator_parameter_sets():
    """the catalog's parameter sets at the block sizes whose inputs the emulator finishes in seconds, the ratio's extremes, and the constructed pairs"""
    sets = [(c, b, r) for b in (1, 2, 63, 64) for r in (0.85, 0.5) for c in (True, False)]
    sets += [(True, 64, 1.0), (False, 63, ref.SMALLEST_RATIO), (True, 4096, 0.85), (False, 4096, 0.5)]
    if not quick:
        sets += [(c, b, r) for b in (4096, 65535, 65536) for r in cases.RATIOS for c in (True, False) if (c, b, r) not in sets]
    return sets


def emulator_inputs(block_size):
    named = cases.inputs(block_size)
    if quick and block_size >= 4096:  # a full block and a byte of every kind, and the several-block text
        named = [(n, d) for n, d in named if len(d) in (0, 1, block_size + 1) or (n.startswith("run") and len(d) > block_size)]
    return named


def compare(title, batch, named, want, caps=None, want_status=None):
    t = time.time()
    outs, status, err = batch.run(0, [d for _, d in named], caps, unaligned=True)
    bad = 0
    for i, ((name, d), c, s) in enumerate(zip(named, outs, status)):
        ws = want_status[i] if want_status else 0
        if s != ws or err[i] != 0 or (ws == 0 and c != want[i]):
            bad += 1
            print("  MISMATCH %s: %s (%d bytes): status %d / %d, %d bytes / %d" % (title, name, len(d), s, ws, len(c), len(want[i])))
    print("%-86s %4d items %8d bytes  %d wrong  (%.0f s)" % (title, len(named), sum(len(d) for _, d in named), bad, time.time() - t), flush=True)
    return bad, len(named)


def check_writers():
    bad = total = 0
    for params in emulator_parameter_sets():
        checksums, block_size, ratio = params
        named = emulator_inputs(block_size)
        want = [ref.compress(d, *params) for _, d in named]
        caps = [ref.max_compressed_length(len(d), block_size) for _, d in named]
        blocks = sum((len(d) + block_size - 1) // block_size for _, d in named)
        for what, variant, entries in (("a wavefront per stream", 0, 0), ("block list", 1, 0), ("block list of %d entries + serial kernel" % (blocks // 2), 1, max(blocks // 2, 1))):
            b, n = compare("%s: %s" % (cases.params_name(params), what), Writer(variant, entries, params), named, want, caps)
            bad, total = bad + b, total + n
        # a capacity one byte below the bound is refused, the item beside it is written
        short = [named[-1], named[1]]
        for variant in (0, 1):
            b, n = compare("%s: variant %d, a byte short" % (cases.params_name(params), variant), Writer(variant, 0, params), short, [b"", want[1]],
                           [caps[-1] - 1, caps[1]], want_status=[MAX_OUTPUT, 0])
            bad, total = bad + b, total + n
    for name, block_size, data, kept, raw in cases.edge_pairs():
        if block_size > 4096 and quick:
            continue
        for ratio in (kept, raw):
            params = (True, block_size, ratio)
            for variant in (0, 1):
                b, n = compare("edge %s, ratio %r: variant %d" % (name, ratio, variant), Writer(variant, 0, params), [(name, data)], [ref.compress(data, *params)],
                               [ref.max_compressed_length(len(data), block_size)])
                bad, total = bad + b, total + n
    return bad, total


def check_window_writer():
    """every cut of a few streams, ample room and room for one block: the one-shot bytes at the same parameters.  Once with a block list of 400 entries for all the
    windows of a call together: a window then stops at its share of the list (NEED_ROOM, need 0) and the loop calls again -- never FAILED"""
    bad = total = 0
    for params, entries in (((True, 63, 0.85), 0), ((False, 64, 0.5), 0), ((True, 1, 0.85), 0), ((True, 4096, 0.85), 0), ((True, 1, 0.85), 400), ((False, 2, 1.0), 400)):
        checksums, block_size, ratio = params
        W.emu_snf_window_list_entries(entries)
        run = window_run(W, True, 0, params, True)
        plains = [d for n, d in emulator_inputs(block_size) if n.startswith(("text", "run"))]
        loops, what = [], []
        for plain in plains:
            for room in (2 * ref.max_compressed_length(len(plain), block_size) + 64, 8 + block_size + 10):
                for cut in cases.cut_positions(len(plain), block_size):
                    loops.append(window_cases.write_stream(plain, cut, room, block_size))
                    what.append((plain, cut, room))
        t = time.time()
        wrong = 0
        for (plain, cut, room), got in zip(what, window_cases.lockstep(run, "snappyframed", True, 0, loops)):
            if got != ref.compress(plain, *params):
                wrong += 1
                print("  MISMATCH window writer, %s: %d bytes cut at %d, room %d" % (cases.params_name(params), len(plain), cut, room))
        print("%-86s %4d items  %d wrong  (%.0f s)" % ("window writer, %s, list of %d" % (cases.params_name(params), entries or 1 << 20), len(what), wrong, time.time() - t), flush=True)
        bad, total = bad + wrong, total + len(what)
    W.emu_snf_window_list_entries(0)
    return bad, total


def check_readers():
    bad = total = 0
    streams = cases.reader_streams()
    for variant in (0, 1, 2, 3):
        for verify in (True, False):
            outs, status, err = Reader(variant, verify).run(0, [s for _, s, *_ in streams], [len(p) + 9 if p is not None else 20000 for _, _, p, *_ in streams], unaligned=True)
            for (name, _, plain, st_on, eo_on, st_off, eo_off), got, st, eo in zip(streams, outs, status, err):
                want_st, want_eo = (st_on, eo_on) if verify else (st_off, eo_off)
                total += 1
                if st != want_st or eo != want_eo or (want_st == 0 and got != plain):
                    bad += 1
                    print("  MISMATCH reader variant %d, verify %d: %s: status %d at %d, want %d at %d (%d bytes)" % (variant, verify, name, st, eo, want_st, want_eo, len(got)))
    # the window reader: the whole stream as one window, and cut in two at a chunk boundary
    FIRST, LAST, FAILED = window_cases.FIRST, window_cases.LAST, window_cases.FAILED
    for variant in (1, 2, 3):
        for verify in (True, False):
            run = window_run(R, False, variant, ref.DEFAULT_PARAMS, verify)
            got = run("snappyframed", False, 0, [s for _, s, *_ in streams], [FIRST | LAST] * len(streams), [len(p) + 9 if p is not None else 20000 for _, _, p, *_ in streams])
            for (name, stream, plain, st_on, eo_on, st_off, eo_off), r in zip(streams, got):
                want_st, want_eo = (st_on, eo_on) if verify else (st_off, eo_off)
                total += 1
                ok = r["status"] == want_st and (want_st == 0 or (r["stop"] == FAILED and r["err"] == want_eo)) and (want_st != 0 or r["out"] == plain)
                if want_st == CHECKSUM:  # a window delivers what lies in front of the chunk that failed
                    ok = ok and r["consumed"] == want_eo and plain.startswith(r["out"])
                if not ok:
                    bad += 1
                    print("  MISMATCH window reader variant %d, verify %d: %s: %r" % (variant, verify, name, {k: (len(v) if k == "out" else v) for k, v in r.items()}))
    print("%-86s %4d items  %d wrong" % ("readers: variants 0 .. 3 and the window reader, verify on and off", total, bad), flush=True)
    return bad, total


def main():
    bad = total = 0
    for check in (check_readers, check_window_writer, check_writers):
        b, n = check()
        bad, total = bad + b, total + n
    print("snf parameters emulator: %d items, %d wrong" % (total, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
