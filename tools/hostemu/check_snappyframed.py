"""x-snappy-framed streams (snappy_frame.hip) on the CPU (tools/hostemu/libemu.so): reader variant 2 -- walk, the chunks through the two-pass
Snappy decoder with an arena asked for after the chunk count is known, CRC-32C verification, fold -- against the plaintext, on the streams the
oracle's restatement of SnappyFramedOutputStream writes (64 KiB chunks, stored when compression does not pay)."""
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


def run(variant, streams, caps):
    lay = Layout(streams, caps, lambda i, n: 5, lambda i, c: 64, fresh=(0, -999, 0))
    emu.emu_snappyframed(variant, *lay.args())
    lay.check_guards("stream")
    return lay.outputs(), lay.status.tolist()


def main():
    whole = b"".join(d for _, d, _ in common.corpus_sample())
    rng = np.random.default_rng(4)
    noise = rng.integers(0, 256, 150000, dtype=np.uint8).tobytes()
    plains = [b"", b"x", whole[:1000], whole[:65536], whole[:65537], whole[:300000], whole[200000:900000], noise, b"ab" * 100000, whole[:100000] + noise + whole[:50000]]
    streams = [o.compress("snappyframed", p) for p in plains]
    bad = 0
    for pad in (0, 21):
        outs, status = run(2, streams, [len(p) + pad for p in plains])
        for i, p in enumerate(plains):
            if status[i] != 0 or outs[i] != p:
                bad += 1
                print("MISMATCH stream %d (len %d, pad %d): status %d, %d bytes" % (i, len(p), pad, status[i], len(outs[i])))
    print("snappy-framed reader, variant 2: %d streams x 2 capacities, %d mismatches" % (len(plains), bad))
    if bad:
        sys.exit(1)


if __name__ == "__main__":
    main()
