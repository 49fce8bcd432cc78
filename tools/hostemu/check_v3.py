"""Runs the ring decoders and the two-pass decoders on the CPU (tools/hostemu/libemu.so) over the GPU parity suite's cases and compares
with the oracle: plaintext, status, error offset, and no write outside the block's output (guard bands).
--part edges [--ops ...]: the catalog of constructed streams of tests/decoder_edge_cases.py instead -- every ring instantiation of the launch tables (lane
widths 1 .. 64, both ring classes, the latency class) on the cases built for its own ring sizes, the two-pass decoders on the 4-lane cases, at four
(source, destination) misalignments."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib
from emu_harness import Layout
from tests import common, oracle_lib
from tests.oracle_lib import OracleError

emu = emulib.load("emu")  # (HOSTEMU_LIB=libemu_lockstep.so: emu_lockstep.cpp, emulib's target `lockstep`)
o = oracle_lib.load()


def run(op, blocks, caps, misalign=0, dst_misalign=None):
    GUARD = 64
    lay = Layout(blocks, caps, lambda i, n: 7 + n % 5, lambda i, c: GUARD + c % 3, src_lead=misalign, dst_lead=GUARD + (misalign if dst_misalign is None else dst_misalign),
                 filler=0, fresh=(0, 0, 0))
    r = emu.emu_batch(op, *lay.args())
    assert r == 0
    lay.check_guards("block")
    return lay.outputs(), lay.status.tolist(), lay.err.tolist()


def expect(codec, data, cap):
    try:
        return 0, 0, o.decompress(codec, data, cap)
    except OracleError as e:
        return e.status, e.offset, None


def cases_for(codec):
    rng = np.random.default_rng(99)
    blocks = [d for _, d in common.HAND_CASES] + [d for _, d, _ in common.corpus_sample()] + common.synthetic_blocks(5, 36)
    base = common.corpus_sample()[0][1]
    blocks += [base[:n] for n in range(1, 256, 7)]
    cases = [(o.compress(codec, b), len(b)) for b in blocks] + [(o.compress(codec, b), len(b) + 37) for b in blocks[:40]]
    if codec == "lz4":
        cases += [(bytes([15, 0, 0, 255, 255, 0x8A, 49, 255, 255, 0]), 1024), (b"", 10), (b"\x00", 0), (b"\x10a", 0),
                  (bytes([0xF0]) + b"\xff" * 4000, 1 << 16), (bytes([0x1F, ord("a"), 1, 0]) + b"\xff" * 4000, 1 << 16)]
    else:
        cases += [(bytes([16, 1, 0, 1, 0, 1, 0, 1, 0]), 1024), (bytes([0xFF, 0xFF, 0xFF, 0xFF, 0x0F, 0]), 10), (bytes([0xFF] * 5), 10), (bytes([0x80]), 10), (b"", 10),
                  (bytes([10, 0xFC, 0xFF, 0xFF, 0xFF, 0x7F]) + b"abc", 100)]
    sample = [d for _, d, _ in common.corpus_sample()[:4]] + common.synthetic_blocks(8, 6)[:6]
    for b in sample:
        c = bytearray(o.compress(codec, b))
        cases += [(bytes(c), len(b) - 1), (bytes(c[:len(c) // 2]), len(b)), (bytes(c[:-1]), len(b))]
        for _ in range(12):
            m = bytearray(c)
            for _ in range(int(rng.integers(1, 4))):
                m[int(rng.integers(0, len(m)))] = int(rng.integers(0, 256))
            cases += [(bytes(m), len(b)), (bytes(m), len(b) + 64)]
    return cases


# --part edges: op -> the (lanes, ring class) whose catalog it runs.  The ops above 2000 are emu.cpp's generic ones (2000 + 10 * lanes + ring class, Snappy
# 1000 higher): every configuration the launch tables hold and no older op runs.
def edge_ops(codec):
    ops = {"lz4": {16: (1, 0), 17: (1, 1), 44: (4, 0), 46: (16, 0), 48: (64, 0), 49: (4, 3)}, "snappy": {12: (1, 0), 13: (1, 1), 54: (4, 0), 56: (16, 0), 58: (64, 0), 59: (4, 3)}}[codec]
    for op in ((24, 25, 26, 27) if codec == "lz4" else (34, 35, 36, 37)):
        ops[op] = (4, 0)
    for lanes, ring in ((2, 0), (2, 1), (4, 1), (4, 2), (8, 0), (8, 1), (16, 1), (32, 0), (32, 1), (64, 1)):
        ops[(2000 if codec == "lz4" else 3000) + 10 * lanes + ring] = (lanes, ring)
    return ops


def edges(only):
    from tests import decoder_edge_cases as dc
    total = 0
    for codec in ("lz4", "snappy"):
        want = {}
        for op, config in edge_ops(codec).items():
            if only is not None and op not in only:
                continue
            if emu.emu_batch(op, None, None, None, None, None, None, None, None, None, 0) != 0:
                print(codec, "op", op, "not built: skipped")
                continue
            valid, damaged = dc.cases(codec, config), dc.malformed(codec, config)
            for k, (src_mis, dst_mis) in enumerate(dc.SHIFTS):
                pad = 9 * (k & 1)  # exact capacity at the first and third pair, capacity + 9 at the others
                cases = [(c.name, c.stream, len(c.plain) + pad) for c in valid] + [(name, s, cap) for name, _, s, cap in damaged]
                key = (config, pad)
                if key not in want:
                    want[key] = [expect(codec, s, cap) for _, s, cap in cases]
                    for c, (est, _, eout) in zip(valid, want[key]):
                        assert est == 0 and eout == c.plain, "the oracle does not decode %r to the builder's plaintext" % c.name
                    assert all(est != 0 for est, _, _ in want[key][len(valid):]), "a malformed case decodes"
                outs, status, err = run(op, [s for _, s, _ in cases], [cap for _, _, cap in cases], src_mis, dst_mis)
                bad = 0
                for i, ((name, s, cap), (est, eoff, eout)) in enumerate(zip(cases, want[key])):
                    if not (status[i] == est and (err[i] == eoff if est != 0 else outs[i] == eout)):
                        bad += 1
                        if bad <= 5 or "--all-mismatches" in sys.argv:
                            print("  MISMATCH %r (%s): emu status %d off %d len %d | oracle status %d off %d len %s" % (
                                name, "targeted" if i < len(valid) and valid[i].kind == "targeted" else ("grammar" if i < len(valid) else "malformed"),
                                status[i], err[i], len(outs[i]), est, eoff, len(eout) if eout is not None else None))
                total += bad
                print("%s op %d lanes %d ring class %d misalign (%d, %d): %d cases, %d mismatches" % (codec, op, config[0], config[1], src_mis, dst_mis, len(cases), bad), flush=True)
    return total


def main():
    # (44 / 46 / 48, 54 / 56 / 58: the ring decoders with 4 / 16 / 64 lanes per block -- the product's default is 4 --: the lanes of a group meet
    #  at the emulator-only lockstep points of achip_rings.h)
    only = [int(x) for x in sys.argv[sys.argv.index("--ops") + 1].split(",")] if "--ops" in sys.argv else None
    if "--part" in sys.argv and sys.argv[sys.argv.index("--part") + 1] == "edges":
        edges(only)
        return
    for codec, ops in (("lz4", (16, 17, 24, 25, 26, 27, 44, 46, 48, 49)), ("snappy", (12, 13, 34, 35, 36, 37, 54, 56, 58, 59))):
        if only is not None:
            ops = tuple(op for op in ops if op in only)
        elif "--quick" in sys.argv:
            ops = tuple(op for op in ops if op not in (46, 48, 56, 58))  # (49 / 59: the latency class stays in)  # (the product's 4 lanes per block only)
        cases = cases_for(codec)
        for op in ops:
            if emu.emu_batch(op, None, None, None, None, None, None, None, None, None, 0) != 0:
                print(codec, "op", op, "not built: skipped")
                continue
            for mis in ((3,) if "--quick" in sys.argv else (0, 3, 13)):
                outs, status, err = run(op, [c for c, _ in cases], [max(cap, 0) for _, cap in cases], mis)
                bad = 0
                for i, (c, cap) in enumerate(cases):
                    est, eoff, eout = expect(codec, c, cap)
                    ok = status[i] == est and (err[i] == eoff if est != 0 else outs[i] == eout)
                    if not ok:
                        bad += 1
                        if bad <= 5:
                            print("  MISMATCH case %d (len %d cap %d): emu status %d off %d len %d | oracle status %d off %d len %s" % (
                                i, len(c), cap, status[i], err[i], len(outs[i]), est, eoff, len(eout) if eout is not None else None))
                print("%s op %d misalign %d: %d cases, %d mismatches" % (codec, op, mis, len(cases), bad))


main()
