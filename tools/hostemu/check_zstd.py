"""Runs the Zstd decode pipeline (zstd_decompress_pipe.hip) on the CPU (tools/hostemu/libemu_zstd.so) over frames of the oracle's encoder
(the Java compressor restated) and of libzstd, and compares with the plaintext.  Items the pipeline hands to its fallback list (the
one-kernel decoder, which these parts do not run) are counted; `--expect-fast` makes any of them a failure.  `--part entropy` runs the catalog of
tests/zstd_entropy_cases.py through both: the one-kernel decoder on libemu_serial.so, and the pipeline."""
import ctypes, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib
from emu_harness import Layout, P
from tests import common, oracle_lib, native_libs

try:
    import pyarrow as pa  # (bundles its own libzstd, whose level 3 splits blocks where the statistics change: frames of many short blocks)

    def libzstd(p, level):
        return pa.Codec("zstd", compression_level=level).compress(p, asbytes=True)
    HAVE_LIBZSTD = True
except ImportError:
    libzstd = native_libs.zstd_compress
    HAVE_LIBZSTD = native_libs.available()

emu = emulib.load("zstd")
o = oracle_lib.load()


def run(frames, caps, tile=0, exec_mode=1, pass_blocks=0, mb_max_bytes=0):
    lay = Layout(frames, caps, lambda i, n: 3, lambda i, c: 64 + i % 5, fresh=(0, 0, 0))  # (unaligned on purpose)
    fb = np.zeros(lay.n + 1, dtype=np.int32)
    counters = np.zeros(64, dtype=np.int32)
    k = emu.emu_zstd_pipe(*lay.args(), tile, exec_mode, P(fb), pass_blocks, P(counters), ctypes.c_int64(mb_max_bytes))
    run.counters = counters
    # (a few bytes beyond the capacity may be scribbled by whole-vector stores only where the product allows it: nowhere)
    lay.check_guards()
    return [out if st == 0 else None for out, st in zip(lay.outputs(), lay.status)], lay.status, sorted(int(x) for x in fb[:k])


def frame_blocks(f):
    fhd = f[4]
    pos = 5 + (0 if fhd & 0x20 else 1) + ((1 if fhd & 0x20 else 0) if fhd >> 6 == 0 else 1 << (fhd >> 6))
    n = 0
    while True:
        h = int.from_bytes(f[pos:pos + 3], "little")
        pos += 3 + (1 if (h >> 1) & 3 == 1 else h >> 3)
        n += 1
        if h & 1:
            return n


def multi_block(expect_fast):
    """frames of several blocks (and of raw / RLE blocks) through the multi-block stages, at several pass sizes"""
    plains = common.multi_block_plains()  # (tests/common.py: also the GPU test's inputs)
    long_frame = len(plains) - 1
    bad = 0
    encs = [("oracle", lambda p: o.compress("zstd", p))]
    if HAVE_LIBZSTD:
        encs += [("libzstd-%d" % l, (lambda l: lambda p: libzstd(p, l))(l)) for l in ((1, 3, 9, 19) if "--quick" not in sys.argv else (3, 19))]
    for name, enc in encs:
        frames = [bytes(enc(p)) for p in plains]
        for pass_blocks, pad in (((2048, 0), (16, 11), (64, 0), (8192, 3)) if "--quick" not in sys.argv else ((2048, 0), (16, 11)) if name == "oracle" else (((8192, 3), (16, 11)) if name == "libzstd-3" else ((2048, 0),))):
            # (the provider refuses more than 400 MB: more than this batch needs -- the stages ask for what the batch needs, not for a full pass)
            outs, status, fb = run(frames, [len(p) + pad for p in plains], pass_blocks=pass_blocks, mb_max_bytes=400 << 20 if pass_blocks == 8192 else 0)
            c = run.counters
            for i, p in enumerate(plains):
                if i in fb:
                    continue
                if status[i] != 0 or outs[i] != p:
                    bad += 1
                    first = -1
                    if outs[i] is not None:
                        m = min(len(outs[i]), len(p))
                        d = np.nonzero(np.frombuffer(outs[i][:m], dtype=np.uint8) != np.frombuffer(p[:m], dtype=np.uint8))[0]
                        first = int(d[0]) if len(d) else m
                    print("MISMATCH %s pass %d item %d (len %d): status %d, produced %s, first difference at %d" % (name, pass_blocks, i, len(p), status[i], None if outs[i] is None else len(outs[i]), first))
            too_long = [i for i, f in enumerate(frames) if frame_blocks(f) > 8 * pass_blocks]
            print("%s, passes of %d: %d frames, listed %d (%d blocks), fast %d, fallback list %s (more blocks than a pass has slots: %s), by stage %s" % (
                name, pass_blocks, len(frames), c[40], c[41], c[42], fb, too_long, [int(x) for x in c[33:39]]))
            if fb != too_long:
                bad += 1
                print("MISMATCH %s pass %d: fallback list %s, expected %s" % (name, pass_blocks, fb, too_long))
    # the multi-block execute stage with the 8 KiB window (option zstd.decompress.exec_window): the oracle's frames again
    frames = [bytes(encs[0][1](p)) for p in plains]
    # (exec_mode bits 4 .. 6: the sequence stage in full workgroups of 4 wavefronts x 16 block slots -- option zstd.decompress.seq_waves)
    outs, status, fb = run(frames, [len(p) for p in plains], exec_mode=1 | (4 << 4) | (3 << 2), pass_blocks=2048)  # (... and the literal stage's split tables)
    wide = sum(1 for i, p in enumerate(plains) if i in fb or status[i] != 0 or outs[i] != p)
    print("oracle, 8 KiB executor window: %d frames, %d mismatches" % (len(frames), wide))
    bad += wide
    # a provider that gives nothing: every listed frame must come back on the fallback list, none touched
    frames = [bytes(encs[0][1](p)) for p in plains[:6]]
    outs, status, fb = run(frames, [len(p) for p in plains[:6]], pass_blocks=2048, mb_max_bytes=1)
    if fb != list(range(6)):
        bad += 1
        print("MISMATCH no scratch: fallback list %s" % fb)
    print("zstd multi-block stages: %d mismatches" % bad)
    return bad


def mutations(expect_fast):
    """damaged multi-block frames: whatever the stages do NOT hand to the fallback list must be exactly what the oracle's decoder returns"""
    whole = b"".join(d for _, d, _ in common.corpus_sample())
    rng = np.random.default_rng(23)
    plains = [whole[:300000], whole[200000:200000 + 140000], b"ab" * 90000 + whole[:50000]]
    bad = 0; kept = 0; total = 0
    encs = [("oracle", lambda p: o.compress("zstd", p))]
    if HAVE_LIBZSTD:
        encs.append(("libzstd-3", lambda p: libzstd(p, 3)))
    for name, enc in encs:
        cases = []; caps = []
        for p in plains:
            f = bytearray(enc(p))
            for k in range(24 if "--quick" not in sys.argv else 8):
                g = bytearray(f)
                kind = k % 6
                if kind == 0:    # a byte somewhere
                    g[int(rng.integers(0, len(g)))] ^= 1 << int(rng.integers(0, 8))
                elif kind == 1:  # a byte in the first block's headers
                    g[int(rng.integers(4, min(40, len(g))))] = int(rng.integers(0, 256))
                elif kind == 2:  # truncated
                    g = g[:int(rng.integers(8, len(g)))]
                elif kind == 3:  # bytes appended
                    g += bytes(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8).tolist())
                elif kind == 4:  # a run of zeros
                    at = int(rng.integers(0, max(1, len(g) - 16))); g[at:at + 16] = bytes(min(16, len(g) - at))
                else:            # the last bytes (block tail / checksum)
                    g[len(g) - 1 - int(rng.integers(0, 6))] ^= 0x10
                cases.append(bytes(g)); caps.append(len(p) if k % 3 else len(p) - int(rng.integers(1, 5000)))
        outs, status, fb = run(cases, caps, pass_blocks=2048)
        for i, (c, cap) in enumerate(zip(cases, caps)):
            total += 1
            try:
                want = o.decompress("zstd", c, cap)
            except oracle_lib.OracleError:
                want = None
            if i in fb:
                continue
            kept += 1
            if want is None or status[i] != 0 or outs[i] != want:
                bad += 1
                print("MISMATCH %s damaged case %d: oracle %s, stages status %d len %s" % (name, i, "refuses" if want is None else len(want), status[i], None if outs[i] is None else len(outs[i])))
    print("zstd multi-block stages, damaged frames: %d cases, %d decoded by the stages, %d mismatches" % (total, kept, bad))
    return bad


def fuzz(n_cases, seed):
    """--fuzz N [SEED]: N damaged multi-block frames (several mutations each, all encoders) through the stages; whatever is not handed to the
    fallback list must be exactly what the oracle's decoder returns.  For the record: profiles/r02_zstd_mb_emulator_fuzz.txt"""
    rng = np.random.default_rng(seed)
    plains = [p for p in common.multi_block_plains() if 131072 < len(p) <= 800000]
    encs = [lambda p: o.compress("zstd", p)] + ([lambda p: libzstd(p, 1), lambda p: libzstd(p, 3), lambda p: libzstd(p, 19)] if HAVE_LIBZSTD else [])
    frames = [(bytes(e(p)), len(p)) for p in plains for e in encs]
    bad = kept = refused_ok = 0
    done = 0
    while done < n_cases:
        cases = []; caps = []
        for _ in range(min(48, n_cases - done)):
            f, n = frames[int(rng.integers(0, len(frames)))]
            g = bytearray(f)
            for _ in range(int(rng.integers(1, 4))):
                kind = int(rng.integers(0, 7))
                if kind == 0:
                    g[int(rng.integers(0, len(g)))] ^= 1 << int(rng.integers(0, 8))
                elif kind == 1:
                    g[int(rng.integers(4, min(64, len(g))))] = int(rng.integers(0, 256))
                elif kind == 2 and len(g) > 16:
                    g = g[:int(rng.integers(8, len(g)))]
                elif kind == 3:
                    g += bytes(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8).tolist())
                elif kind == 4:
                    at = int(rng.integers(0, max(1, len(g) - 16))); g[at:at + 8] = bytes(rng.integers(0, 256, min(8, len(g) - at), dtype=np.uint8).tolist())
                elif kind == 5:
                    g[len(g) - 1 - int(rng.integers(0, min(8, len(g))))] ^= 0x10
                else:  # a block header: find one by walking, then flip a bit of it
                    at = int(rng.integers(0, len(g)))
                    g[at] ^= int(rng.integers(1, 256))
            cases.append(bytes(g)); caps.append(n if rng.random() < 0.7 else max(1, n - int(rng.integers(1, 70000))))
        outs, status, fb = run(cases, caps, pass_blocks=2048)
        for i, (c, cap) in enumerate(zip(cases, caps)):
            try:
                want = o.decompress("zstd", c, cap)
            except oracle_lib.OracleError:
                want = None
            if i in fb:
                refused_ok += 1
                continue
            kept += 1
            if want is None or status[i] != 0 or outs[i] != want:
                bad += 1
                print("MISMATCH case %d of batch at %d: oracle %s, stages status %d len %s" % (i, done, "refuses" if want is None else len(want), status[i], None if outs[i] is None else len(outs[i])))
        done += len(cases)
    print("zstd multi-block stages, fuzz seed %d: %d damaged frames, %d decoded by the stages (all equal to the oracle's output: %s), %d handed to the fallback list, %d mismatches" % (
        seed, done, kept, bad == 0, refused_ok, bad))
    return bad


def catalog_cases(quick):
    """the case catalog of tests/zstd_frame_cases.py: the hand frames, and the encoders' frames next to them"""
    from tests import zstd_frame_cases as zc
    text = b"".join(d for _, d, _ in common.corpus_sample()[:3])
    encs = [("oracle", lambda p: o.compress("zstd", p))] + ([("libzstd-3", lambda p: libzstd(p, 3))] if HAVE_LIBZSTD else [])
    cases = zc.catalog() + zc.encoder_cases(zc.encoder_plains(text, common.synthetic_blocks(21, 1, 131072)[0]), encs)
    if quick:  # (the frames beyond 40 KB: only the far offsets' -- nothing else in them that a smaller frame does not have)
        cases = [c for c in cases if c.cap <= 40000 or c.name.startswith("far-")]
    return cases


def catalog(expect_fast):
    """--part catalog: the execute stage's case catalog under BOTH executors -- exec_mode low bits 0: the ring executor (zstd_pipe_execute_kernel), without a
    staging area for far matches and (bit 8) with the product's; 1: the record executor -- at exact capacities and with slack.  A valid frame must come back as the
    oracle's plaintext from the fast path; a malformed one (all of them are malformed at the execute stage) must be on the fallback list, counted at stage 4."""
    cases = catalog_cases("--quick" in sys.argv)
    bad = 0
    for mode, what in ((0, "ring executor, no staging area"), (0 | (1 << 8), "ring executor, far matches staged"), (1, "record executor")):
        for pad in (0, 64):
            caps = [c.capacity(pad) for c in cases]
            outs, status, fb = run([c.frame for c in cases], caps, exec_mode=mode)
            wrong = 0
            for i, c in enumerate(cases):
                try:
                    want = o.decompress("zstd", c.frame, caps[i])
                except oracle_lib.OracleError:
                    want = None
                if (want is None) != c.malformed or (want is not None and want != c.plain):
                    wrong += 1
                    print("MISMATCH catalog %s: the oracle %s" % (c.name, "refuses" if want is None else "decodes %d bytes" % len(want)))
                elif want is None:
                    if i not in fb:
                        wrong += 1
                        print("MISMATCH %s, pad %d, %s: malformed, but not on the fallback list (status %d)" % (what, pad, c.name, status[i]))
                elif i in fb or status[i] != 0 or outs[i] != want:
                    wrong += 1
                    first = -1
                    if outs[i] is not None:
                        m = min(len(outs[i]), len(want))
                        d = np.nonzero(np.frombuffer(outs[i][:m], dtype=np.uint8) != np.frombuffer(want[:m], dtype=np.uint8))[0]
                        first = int(d[0]) if len(d) else m
                    print("MISMATCH %s, pad %d, %s: %s, status %d, %s bytes of %d, first difference at %d" % (
                        what, pad, c.name, "on the fallback list" if i in fb else "fast path", status[i], None if outs[i] is None else len(outs[i]), len(want), first))
            stages = [int(x) for x in run.counters[33:39]]
            n_bad = sum(1 for c in cases if c.malformed)
            if stages != [0, 0, 0, n_bad, 0, 0]:
                wrong += 1
                print("MISMATCH %s, pad %d: fallback list by stage %s, expected %d at stage 4 only" % (what, pad, stages, n_bad))
            print("catalog, %s, pad %d: %d frames (%d malformed), fallback list by stage %s, %d wrong" % (what, pad, len(cases), n_bad, stages, wrong), flush=True)
            bad += wrong
    print("zstd execute-stage catalog under both executors: %d mismatches" % bad)
    return bad


def entropy(expect_fast):
    """--part entropy: the catalog of tests/zstd_entropy_cases.py (hand-built FSE tables, Huffman tables and streams, treeless literals and repeat-mode tables across
    blocks) through the one-kernel decoder (libemu_serial.so) -- status, error offset and bytes as the oracle has them -- and through the pipeline: the literal stage with
    split tables (13 items), plain entries (16) and lengths by symbol (16), the sequence stage on 1 and 4 wavefronts, exact capacities and 64 bytes of slack, catalog order and a seeded shuffle.
    Every malformed case and every case the parse stage hands over by design must be on the fallback list; every other valid one must come back from the fast path."""
    from emu_harness import EmuBatch
    from tests import zstd_entropy_cases as ze
    cases = ze.entropy_catalog()
    quick = "--quick" in sys.argv
    bad = 0

    def expect(c, cap):
        try:
            return 0, 0, o.decompress("zstd", c.frame, cap)
        except oracle_lib.OracleError as e:
            return e.status, e.offset, None
    expected = {pad: [expect(c, c.capacity(pad)) for c in cases] for pad in (0, 64)}
    for pad in (0, 64):
        for c, (est, _, eout) in zip(cases, expected[pad]):
            if (est != 0) != c.malformed or (est == 0 and eout != c.plain):
                bad += 1
                print("MISMATCH entropy catalog %s: the oracle %s" % (c.name, "refuses" if est else "decodes %d bytes" % len(eout)))
    one = EmuBatch()
    for pad in (0, 64):
        outs, status, err = one.run(4, [c.frame for c in cases], [c.capacity(pad) for c in cases], unaligned=(pad == 0))
        wrong = 0
        for i, (c, (est, eoff, eout)) in enumerate(zip(cases, expected[pad])):
            if status[i] != est or (est == 0 and outs[i] != eout) or (est != 0 and err[i] != eoff):
                wrong += 1
                print("MISMATCH one-kernel decoder, pad %d, %s: status %d offset %d, the oracle's %d offset %d" % (pad, c.name, status[i], err[i], est, eoff))
        print("entropy catalog, one-kernel decoder, pad %d: %d frames, %d wrong" % (pad, len(cases), wrong), flush=True)
        bad += wrong
    LIT = {3 << 2: "split tables (13 items)", 0: "plain entries (16 items)", 1 << 7: "lengths by symbol (16 items)"}
    runs = [(3 << 2, 1, 0, False), (0, 4, 64, True), (1 << 7, 1, 0, True)] if quick else [(lit, waves, pad, shuffled) for lit in LIT for waves in (1, 4) for pad in (0, 64) for shuffled in (False, True)]
    for lit, waves, pad, shuffled in runs:
        order = np.random.default_rng(77).permutation(len(cases)) if shuffled else np.arange(len(cases))
        sub = [cases[i] for i in order]
        outs, status, fb = run([c.frame for c in sub], [c.capacity(pad) for c in sub], exec_mode=1 | lit | (waves << 4), pass_blocks=2048)
        wrong = 0
        for i, c in enumerate(sub):
            est, eoff, eout = expected[pad][order[i]]
            if c.malformed or c.fallback:
                if i not in fb:
                    wrong += 1
                    print("MISMATCH pipeline, %s: %s, but not on the fallback list (status %d)" % (c.name, "malformed" if c.malformed else c.fallback, status[i]))
            elif i in fb or status[i] != 0 or outs[i] != eout:
                wrong += 1
                first = -1
                if outs[i] is not None:
                    m = min(len(outs[i]), len(eout))
                    d = np.nonzero(np.frombuffer(outs[i][:m], dtype=np.uint8) != np.frombuffer(eout[:m], dtype=np.uint8))[0]
                    first = int(d[0]) if len(d) else m
                print("MISMATCH pipeline, %s: %s, status %d, %s bytes of %d, first difference at %d" % (
                    c.name, "on the fallback list" if i in fb else "fast path", status[i], None if outs[i] is None else len(outs[i]), len(eout), first))
        stages = [int(x) for x in run.counters[33:39]]
        want = sum(1 for c in cases if c.malformed or c.fallback)
        if sum(stages) != want or len(fb) != want:
            wrong += 1
            print("MISMATCH pipeline: %d on the fallback list, by stage %s, expected %d" % (len(fb), stages, want))
        print("entropy catalog, pipeline, literal stage %s, sequence stage on %d wavefronts, pad %d, %s: %d frames, fallback list by stage %s, %d wrong" % (
            LIT[lit], waves, pad, "shuffled" if shuffled else "catalog order", len(cases), stages, wrong), flush=True)
        bad += wrong
    print("zstd entropy catalog on the one-kernel decoder and the pipeline: %d mismatches" % bad)
    return bad


def main():
    if "--fuzz" in sys.argv:
        k = sys.argv.index("--fuzz")
        sys.exit(1 if fuzz(int(sys.argv[k + 1]), int(sys.argv[k + 2]) if len(sys.argv) > k + 2 else 1) else 0)
    expect_fast = "--expect-fast" in sys.argv
    part = sys.argv[sys.argv.index("--part") + 1] if "--part" in sys.argv else "all"  # single | multi | damaged | catalog | entropy | all
    if part == "multi":
        sys.exit(1 if multi_block(expect_fast) else 0)
    if part == "damaged":
        sys.exit(1 if mutations(expect_fast) else 0)
    if part == "catalog":
        sys.exit(1 if catalog(expect_fast) else 0)
    if part == "entropy":
        sys.exit(1 if entropy(expect_fast) else 0)
    plains = [d for _, d in common.HAND_CASES if len(d) > 0] + [d[:131072] for _, d, _ in common.corpus_sample()[:8]] + common.synthetic_blocks(5, 6)
    plains = [p for p in plains if len(p) <= 131072]
    bad = 0; slow = 0; total = 0
    quick = "--quick" in sys.argv
    for name, enc in (("oracle", lambda p: o.compress("zstd", p)), ("libzstd-1", lambda p: libzstd(p, 1)), ("libzstd-3", lambda p: libzstd(p, 3)),
                      ("libzstd-9", lambda p: libzstd(p, 9))):
        if name.startswith("libzstd") and (not HAVE_LIBZSTD or (quick and name != "libzstd-3")):
            continue
        frames = [bytes(enc(p)) for p in plains]
        # (second run: the 8-items-per-wavefront instantiations of the literal and sequence stages -- mode bits 2 and 3)
        # (... and the sequence stage in full workgroups of 1, 2 and 4 wavefronts: mode bits 4 .. 6, lanes without an item beside lanes with one)
        # (... and the literal stage at 8 and 10 items per wavefront: mode bits 2, 3 -- option zstd.decompress.lit_items)
        for pad, mode in ((0, 1), (37, 1), (0, 1 | (1 << 4)), (0, 1 | (2 << 4)), (0, 1 | (4 << 4)), (0, 1 | (1 << 2)), (0, 1 | (2 << 2)), (0, 1 | (3 << 2)), (0, 1 | (1 << 7))):  # (3 << 2: 13 items, symbols and length nibbles apart; 1 << 7: 16 items, lengths by symbol)
            outs, status, fb = run(frames, [len(p) + pad for p in plains], exec_mode=mode)
            for i, p in enumerate(plains):
                total += 1
                if i in fb:
                    slow += 1
                elif status[i] != 0 or outs[i] != p:
                    bad += 1
                    print("MISMATCH %s item %d (len %d): status %d" % (name, i, len(p), status[i]))
        print("%s: %d frames, fallback list %s" % (name, len(frames), fb))
    print("zstd pipeline: %d cases, %d mismatches, %d on the fallback list" % (total, bad, slow))
    if part == "all":
        bad += multi_block(expect_fast)
        bad += mutations(expect_fast)
        bad += catalog(expect_fast)
        bad += entropy(expect_fast)
    if bad or (expect_fast and slow):
        sys.exit(1)


def stream_cases():
    """launch_zstd_stream_step under the emulator: frames cut into steps of a few blocks, tables / repeat offsets / window / checksum carried from
    step to step; this script plays the host's part (abi_zstd_stream.cpp: achip_zstdstream_decompress_feed) -- the stand-in frame header in front of a step, the
    history kept behind the output -- over the product's own walk (achip_zstd_frame.h: read_frame_header, list_step).  Damaged frames: the blocks in front of
    the damage are delivered, the first damaged block is where the oracle's decoder fails too; where the WALK stops, the oracle's decoder must fail as well."""
    emu.emu_zstd_stream_carry_bytes.restype = ctypes.c_int64
    cb = emu.emu_zstd_stream_carry_bytes()

    def decode(frame, step_blocks):
        """returns (plaintext delivered, None or where the stream stopped: the index of the first bad block, "checksum", or the WALK's verdict -- "header", "window",
        "block type", "truncated")"""
        assert frame[:4] == b"\x28\xb5\x2f\xfd"
        buf = np.frombuffer(frame, dtype=np.uint8).copy()
        head = np.zeros(7, dtype=np.int64)
        emu.emu_zstd_read_frame_header(P(buf[4:]), ctypes.c_int64(len(buf) - 4), P(head))
        state, _, _, header_size, has_checksum, look, beyond_java = (int(x) for x in head)
        if state != 0:
            return b"", "truncated" if state == 1 else "header"
        if look < 0:
            return b"", "window"
        pos = 4 + header_size
        carry = np.zeros(cb, dtype=np.uint8)
        emu.emu_zstd_stream_carry_init(P(carry))
        W = max(look, 1 << 16)
        room = step_blocks + 15  # (a RAW / RLE block of up to 16 parts needs a step with room for it: the product's 32 always have, steps of 1, 3 or 4 get a longer one)
        S = room * 131072
        hist = np.full(W + S + 64, 0xEE, dtype=np.uint8)
        hist_len = 0
        out = bytearray()
        block_no = 0
        listed = np.zeros(4 * room, dtype=np.int64)
        info = np.zeros(4, dtype=np.int64)
        while True:
            n = emu.emu_zstd_list_step(P(buf[pos:]), ctypes.c_int64(len(buf) - pos), has_checksum, beyond_java, step_blocks, P(listed), P(info))
            if n == 0 and int(info[3]) == 0:  # (nothing listed, nothing broken: truncated -- or a block of more parts than a step of step_blocks has room for)
                n = emu.emu_zstd_list_step(P(buf[pos:]), ctypes.c_int64(len(buf) - pos), has_checksum, beyond_java, room, P(listed), P(info))
            at, closing, expected, broken = (int(x) for x in info)
            if n == 0:
                return bytes(out), ("truncated", "block type", "window")[broken]
            body = bytearray(b"\x28\xb5\x2f\xfd\x20\x00")
            for i in range(n):
                hd, data_pos, data_len, _ = (int(x) for x in listed[4 * i:4 * i + 4])
                body += ((hd & ~1) | (1 if i == n - 1 else 0)).to_bytes(3, "little") + frame[pos + data_pos:pos + data_pos + data_len]
            src = np.frombuffer(bytes(body), dtype=np.uint8).copy()
            result = np.zeros(3, dtype=np.int32)
            base = hist[W - hist_len:]
            rc = emu.emu_zstd_stream_step(P(carry), P(src), len(src), n, P(base), hist_len, hist_len + S, closing, has_checksum, ctypes.c_uint32(expected), P(result))
            assert rc == 0, rc
            good, produced, verdict = int(result[0]), int(result[1]), int(result[2])
            out += hist[W:W + produced].tobytes()
            keep = min(look, hist_len + produced)
            hist[W - keep:W] = hist[W + produced - keep:W + produced].copy()
            hist_len = keep
            if good < n:
                return bytes(out), block_no + good
            block_no += n
            if closing:
                if has_checksum and verdict != 1:
                    return bytes(out), "checksum"
                return bytes(out), None
            pos += at

    bad = 0
    plains = common.multi_block_plains()
    whole = b"".join(d for _, d, _ in common.corpus_sample())
    plains = [p for p in plains if len(p) > 131072][:6] + [whole[:700000], (whole * 3)[:1500000]]
    encs = [("oracle", lambda p: o.compress("zstd", p)), ("oracle-stream", lambda p: o.zstd_stream_compress(p))]
    if HAVE_LIBZSTD:
        encs += [("libzstd-3", lambda p: libzstd(p, 3)), ("libzstd-19", lambda p: libzstd(p, 19))]
    total = 0
    for name, enc in encs:
        for k, p in enumerate(plains):
            f = bytes(enc(p))
            for step_blocks in ((1, 3, 32) if "--quick" not in sys.argv else (2,)):
                got, where = decode(f, step_blocks)
                total += 1
                if where is not None or got != p:
                    bad += 1
                    print("MISMATCH stream %s plain %d (%d bytes) steps of %d: stopped at %s, %d bytes" % (name, k, len(p), step_blocks, where, len(got)))
    print("zstd stream steps: %d decodes, %d mismatches" % (total, bad), flush=True)
    # damage: what is delivered is a prefix of the plaintext made of whole blocks, and the oracle's decoder fails as well
    rng = np.random.default_rng(5)
    cases = 0
    for name, enc in encs[:3]:
        for p in plains[:3]:
            f = bytearray(enc(p))
            for _ in range(4 if "--quick" not in sys.argv else 1):
                g = bytearray(f)
                g[int(rng.integers(12, len(g) - 4))] ^= 1 << int(rng.integers(0, 8))
                got, where = decode(bytes(g), 4)  # (a damaged block header: the walk's own verdict, which the oracle failing must bear out)
                cases += 1
                try:
                    ref_plain = o.decompress("zstd", bytes(g), len(p) + 1024)
                    ref_ok = True
                except oracle_lib.OracleError:
                    ref_ok = False
                if where is None:
                    if not ref_ok or got != ref_plain:
                        bad += 1
                        print("MISMATCH damaged %s: the steps decoded %d bytes, the oracle %s" % (name, len(got), "fails" if not ref_ok else "differs"))
                else:
                    # (a flipped bit in literal or sequence DATA decodes to other bytes and is caught by the checksum at the frame's end, here as in the
                    # Java stream; a stop at a block must deliver whole blocks of the plaintext in front of it)
                    if ref_ok or (where != "checksum" and got != p[:len(got)]):
                        bad += 1
                        print("MISMATCH damaged %s: stopped at %s with %d bytes (a prefix: %s), the oracle %s" % (name, where, len(got), got == p[:len(got)], "decodes" if ref_ok else "fails"))
    print("zstd stream steps, damaged frames: %d cases, %d mismatches in all" % (cases, bad), flush=True)
    return bad


if __name__ == "__main__":
    if "--stream" in sys.argv:
        sys.exit(1 if stream_cases() else 0)
    main()
