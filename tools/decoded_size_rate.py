"""What sizing a device-resident batch costs next to decoding it: achip_decoded_size_batch against the op's decoder, in one process, on the same buffers.

For every row: plaintext made on the device (bench.py's fragments / tiled corpus generators), compressed by the product's encoder for the op, then three
warm-ups of each call and --rounds alternating rounds (size, decode, size, decode, ...), each timed with device events on the context's stream.  The decode is
the known-size path: dstCap = the plaintext length.  Every size is checked against the plaintext length before anything is timed.  Prints one JSON line per
row and a table: sizing ms, decode ms, their ratio (condition 1 of DESIGN 10b: below 1 on every row).

    python tools/decoded_size_rate.py [--rows lz4,snappy,zstd,lz4frame,snappyframed,lz4hadoop,snappyhadoop] [--kinds fragments,corpus] [--rounds 7] [--out rows.json]

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/decoded_size_rate.py --rounds 1 --rows lz4`.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# row -> (compress op, decompress op, items, item bytes): the sizes of README's table (262 144 x 64 KiB blocks, 65 536 x 128 KiB Zstd frames) and the
# 1024 x 4 MiB container batches
ROWS = {
    "lz4": (1, 0, 262144, 65536),
    "snappy": (3, 2, 262144, 65536),
    "zstd": (5, 4, 65536, 131072),
    "lz4frame": (7, 6, 1024, 4 << 20),
    "snappyframed": (9, 8, 1024, 4 << 20),
    "lz4hadoop": (11, 10, 1024, 4 << 20),
    "snappyhadoop": (13, 12, 1024, 4 << 20),
}


def bound(lib, row, n):
    if row in ("lz4", "snappy", "zstd", "lz4frame", "snappyframed"):
        return getattr(lib, "achip_%s_max_compressed_length" % row)(n)
    return lib.achip_hadoop_max_compressed_length(0 if row == "lz4hadoop" else 1, n, 262144)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--kinds", default="fragments,corpus")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0, help="development aid: items per row times this")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    import aircompressor_amd as A
    import bench
    if not torch.cuda.is_available():
        sys.exit("decoded_size_rate.py needs a GPU")
    codec = A.HipBatchCodec(0)
    stream = torch.cuda.ExternalStream(codec.native.stream)
    dev = torch.device("cuda", 0)
    results = []
    for row in args.rows.split(","):
        cop, dop, n, size = ROWS[row]
        n = max(1, int(n * args.scale))
        for kind in args.kinds.split(","):
            plain = bench.gen_data(torch, dev, kind, n, size, 0.5, 77)
            cap = bound(codec.lib, row, size)
            i64 = lambda v: torch.full((n,), v, dtype=torch.int64, device=dev)  # noqa: E731
            i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dev)  # noqa: E731
            p_off = torch.arange(n, dtype=torch.int64, device=dev) * size
            c_off = torch.arange(n, dtype=torch.int64, device=dev) * cap
            comp = torch.empty(n * cap + 64, dtype=torch.uint8, device=dev)
            c_len, st, eo = i32(0), i32(-7), i64(0)
            torch.cuda.synchronize()
            codec.launch(cop, plain, p_off, i32(size), comp, c_off, i32(cap), c_len, st, eo, n)
            codec.synchronize()
            assert int((st != 0).sum().item()) == 0, "the encoder failed"
            compressed = int(c_len.sum().item())
            out = torch.empty(n * size + 64, dtype=torch.uint8, device=dev)
            o_len, d_cap, out_size = i32(-7), i32(size), i64(-7)

            def size_call():
                codec.decoded_sizes(dop, comp, c_off, c_len, out_size, st, eo, n)

            def decode_call():
                codec.launch(dop, comp, c_off, c_len, out, p_off, d_cap, o_len, st, eo, n)

            size_call()
            codec.synchronize()
            assert int((st != 0).sum().item()) == 0 and int((out_size != size).sum().item()) == 0, "sizes differ from the plaintext length"
            decode_call()
            codec.synchronize()
            assert int((st != 0).sum().item()) == 0 and bool((out[:n * size] == plain).all().item()), "the decoder's output differs from the plaintext"
            for _ in range(3):
                size_call()
                decode_call()
            codec.synchronize()
            times = {"size": [], "decode": []}
            for _ in range(args.rounds):
                for what, call in (("size", size_call), ("decode", decode_call)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    call()
                    e1.record(stream)
                    e1.synchronize()
                    times[what].append(e0.elapsed_time(e1))
            ts, td = statistics.median(times["size"]), statistics.median(times["decode"])
            r = {"op": row, "data": kind, "items": n, "item_bytes": size, "compressed_bytes": compressed, "size_ms": round(ts, 4), "decode_ms": round(td, 4),
                 "ratio": round(ts / td, 4), "size_runs_ms": [round(x, 4) for x in times["size"]], "decode_runs_ms": [round(x, 4) for x in times["decode"]],
                 "size_gib_s_of_compressed": round(compressed / (ts / 1e3) / 2**30, 1), "decode_gib_s_of_plaintext": round(n * size / (td / 1e3) / 2**30, 1)}
            results.append(r)
            print(json.dumps(r), flush=True)
            del plain, comp, out
            torch.cuda.empty_cache()
    print("\n%-13s %-10s %8s %9s %11s %11s %7s" % ("op", "data", "items", "item", "sizing ms", "decode ms", "ratio"))
    for r in results:
        print("%-13s %-10s %8d %9d %11.3f %11.3f %7.3f" % (r["op"], r["data"], r["items"], r["item_bytes"], r["size_ms"], r["decode_ms"], r["ratio"]))
    print("condition 1 (sizing costs less than decoding): %s" % ("holds on every row" if all(r["ratio"] < 1 for r in results) else "FAILS on " + ", ".join(
        "%s/%s" % (r["op"], r["data"]) for r in results if r["ratio"] >= 1)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
