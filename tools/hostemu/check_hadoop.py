"""Hadoop LZ4 / Snappy block streams (hadoop_streams.hip) on the CPU (tools/hostemu/libemu.so): the reader's variant 2 -- walk, the chunks
through the two-pass decoders with an arena asked for after the chunk count is known, fold, the serial kernel for everything else --
against the oracle, on the streams every writer produces.  (Variant 1 runs the chunks through the ring decoders at 4 / 16 lanes per chunk,
which lean on the hardware's in-order memory pipeline and do not run here.)"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib
from emu_harness import Layout
from tests import common, oracle_lib

emu = emulib.load("emu")
o = oracle_lib.load()


def run(snappy, buffer_size, variant, streams, caps):
    lay = Layout(streams, caps, lambda i, n: 7, lambda i, c: 64, fresh=(0, -999, 0))
    emu.emu_hadoop(0, 1 if snappy else 0, buffer_size, variant, *lay.args())
    lay.check_guards("stream")
    return lay.outputs(), lay.status.tolist(), lay.err.tolist()


def main():
    whole = b"".join(d for _, d, _ in common.corpus_sample())
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 256, 90000, dtype=np.uint8).tobytes()
    plains = [b"", b"x", whole[:1000], whole[:70000], whole[:300000], whole[100000:700000], noise, b"ab" * 150000, whole[:218422], whole[:259523 * 2]]
    bad = 0
    for codec, snappy in (("lz4", False), ("snappy", True)):
        for buf in (262144, 70000, 4096):
            streams = [o.hadoop_compress(codec, p, buf) for p in plains]
            caps = [len(p) for p in plains]
            cases = list(zip(streams, caps))
            # (valid streams only: anything irregular goes to the wavefront-per-stream kernel, whose block decoder moves bytes between lanes in
            # hardware order and does not run here -- tests/test_gpu_hadoop.py covers it on the GPU)
            outs, status, err = run(snappy, buf, 2, [c for c, _ in cases], [cap for _, cap in cases])
            m = 0
            for i, (c, cap) in enumerate(cases):
                try:
                    want = o.hadoop_decompress(codec, c, cap, buf); est = 0; eoff = 0
                except oracle_lib.OracleError as e:
                    want = None; est = e.status; eoff = e.offset
                if status[i] != est or (est == 0 and outs[i] != want) or (est != 0 and err[i] != eoff):
                    m += 1
                    print("MISMATCH %s buffer %d case %d: status %d@%d, oracle %d@%d" % (codec, buf, i, status[i], err[i], est, eoff))
            bad += m
            print("hadoop %s reader, variant 2, buffer %d: %d streams, %d mismatches" % (codec, buf, len(cases), m))
    if bad:
        sys.exit(1)


if __name__ == "__main__":
    main()
