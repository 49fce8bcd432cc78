"""What the LZO1X block codec makes on an MI355X, beside LZ4 on the same plaintext in the same run: achip_lzo_decompress_batch at variants 1 (two passes) and 2 (a
wavefront per item), achip_lzo_compress_batch, and LZO decode at 64, 1 024 and 4 096 blocks -- the table auto mode's line ("lzo.decompress.auto_min_blocks") is
set from.

Batches: 16 384 x 64 KiB blocks of bench.py's fragments data and of its text-like corpus data.  Per row three warm-up launches, then the mean of --launches (at
least 5) timed launches, device events on the context's stream; GiB/s of plaintext, compressed / plain.  Every encoder's output is decoded by the GPU decoder
of the same codec and compared with the plaintext once, every decode is compared with the plaintext once.  Nothing is asserted about speed.

    python tools/lzo_rate.py [--launches 5] [--scale 1.0] [--out profiles/lzo_rate.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OP_LZ4_DECOMPRESS, OP_LZ4_COMPRESS, OP_LZO_DECOMPRESS, OP_LZO_COMPRESS = 0, 1, 16, 17
SMALL = (64, 1024, 4096)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="development aid: blocks per batch times this")
    ap.add_argument("--out")
    args = ap.parse_args()
    launches = max(5, args.launches)
    import torch
    import aircompressor_amd as A
    import bench
    if not torch.cuda.is_available():
        sys.exit("lzo_rate.py needs a GPU")
    codec = A.HipBatchCodec(0)
    stream = torch.cuda.ExternalStream(codec.native.stream)
    dev = torch.device("cuda", 0)
    n, size = max(64, int(16384 * args.scale)), 65536
    cap = codec.lib.achip_lzo_max_compressed_length(size)  # (LZ4's bound is the same formula)
    assert cap == codec.lib.achip_lz4_max_compressed_length(size)
    i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dev)  # noqa: E731
    p_off = torch.arange(n, dtype=torch.int64, device=dev) * size
    c_off = torch.arange(n, dtype=torch.int64, device=dev) * cap
    p_len, c_cap, st, d_len = i32(size), i32(cap), i32(0), i32(0)
    eo = torch.zeros(n, dtype=torch.int64, device=dev)
    slots = {"lz4": torch.empty(n * cap + 64, dtype=torch.uint8, device=dev), "lzo": torch.empty(n * cap + 64, dtype=torch.uint8, device=dev)}
    c_len = {"lz4": i32(0), "lzo": i32(0)}
    back = torch.empty(n * size + 64, dtype=torch.uint8, device=dev)
    results = []

    def timed(call):
        for _ in range(3):
            call()
        codec.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(launches):
            call()
        e1.record(stream)
        e1.synchronize()
        assert int((st != 0).sum().item()) == 0, "statuses %s" % torch.unique(st).tolist()[:8]
        return e0.elapsed_time(e1) / launches

    def row(kind, what, blocks, ms, ratio=None):
        r = {"batch": kind, "what": what, "blocks": blocks, "ms": round(ms, 3), "gib_s": round(blocks * size / (ms / 1e3) / 2**30, 2)}
        if ratio is not None:
            r["ratio"] = round(ratio, 4)
        results.append(r)
        print(json.dumps(r), flush=True)

    for kind in ("fragments", "corpus"):
        plain = bench.gen_data(torch, dev, kind, n, size, 0.5, 77)
        torch.cuda.synchronize()  # (the tensors are made on torch's stream, the calls run on the context's)
        for name, op in (("lz4", OP_LZ4_COMPRESS), ("lzo", OP_LZO_COMPRESS)):
            ms = timed(lambda: codec.launch(op, plain, p_off, p_len, slots[name], c_off, c_cap, c_len[name], st, eo, n))
            row(kind, "%s compress" % name, n, ms, int(c_len[name].sum(dtype=torch.int64).item()) / (n * size))

        def decode(name, op, blocks):
            codec.launch(op, slots[name], c_off, c_len[name], back, p_off, p_len, d_len, st, eo, blocks)

        def restored(blocks):
            codec.synchronize()
            return bool((back[:blocks * size] == plain[:blocks * size]).all().item())

        back.zero_()
        row(kind, "lz4 decompress (auto)", n, timed(lambda: decode("lz4", OP_LZ4_DECOMPRESS, n)))
        assert restored(n), "LZ4 does not restore the plaintext"
        for variant, what in ((1, "two passes"), (2, "a wavefront per item")):
            codec.native.set_option("lzo.decompress.variant", variant)
            for blocks in (n,) + tuple(b for b in SMALL if b < n):
                back.zero_()
                ms = timed(lambda: decode("lzo", OP_LZO_DECOMPRESS, blocks))
                row(kind, "lzo decompress, %s" % what, blocks, ms)
                assert restored(blocks), "LZO variant %d does not restore the plaintext" % variant
                if variant == 1:
                    assert codec.native.get_stat("lzo.decompress.fallback_blocks") == 0
        codec.native.set_option("lzo.decompress.variant", 0)
        for blocks in tuple(b for b in SMALL if b < n):
            row(kind, "lz4 decompress (auto)", blocks, timed(lambda: decode("lz4", OP_LZ4_DECOMPRESS, blocks)))
        del plain
    lines = ["The LZO1X block codec beside LZ4 on the same plaintext, the same run: blocks of 64 KiB, mean of %d launches after 3 warm-ups, device events on the" % launches,
             "context's stream; every output decoded / compared with the plaintext once (tools/lzo_rate.py).  GiB/s of plaintext.",
             "", "%-10s %-40s %8s %10s %9s %18s" % ("batch", "what", "blocks", "ms", "GiB/s", "compressed/plain")]
    for r in results:
        lines.append("%-10s %-40s %8d %10.3f %9.2f %18s" % (r["batch"], r["what"], r["blocks"], r["ms"], r["gib_s"], "%.4f" % r["ratio"] if "ratio" in r else ""))
    print("\n" + "\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
