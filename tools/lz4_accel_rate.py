"""What the acceleration of Lz4Compressor.create(acceleration) buys on an MI355X: achip_lz4_compress_batch at accelerations 1, 2, 4, 8, 16 and 64, window encoder
(lz4.compress.variant 4, the default) and batch probes (variant 1) in the same run.

Batches: 65 536 x 64 KiB corpus blocks and 65 536 x 64 KiB fragments blocks (bench.py's generators).  Per (batch, variant, acceleration), acceleration 1 first: three
warm-up launches, then the mean of --launches (at least 10) timed launches, device events on the context's stream; GiB/s of plaintext and the compressed / plain
ratio.  After the timing every row's output is decoded by the GPU decoder and compared with the plaintext, once.  Acceleration 1 runs the kernels the parameter
did not touch, the others their `_accel` twins (lz4_compress.hip).  Nothing is asserted about speed: rows where a higher acceleration is slower stay in the file.

    python tools/lz4_accel_rate.py [--launches 10] [--scale 1.0] [--out profiles/lz4_accel_rate.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACCELERATIONS = (1, 2, 4, 8, 16, 64)
VARIANTS = ((4, "window (default)"), (1, "batch probes"))
OP_LZ4_DECOMPRESS, OP_LZ4_COMPRESS = 0, 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="development aid: blocks per batch times this")
    ap.add_argument("--out")
    args = ap.parse_args()
    launches = max(10, args.launches)
    import torch
    import aircompressor_amd as A
    import bench
    if not torch.cuda.is_available():
        sys.exit("lz4_accel_rate.py needs a GPU")
    codec = A.HipBatchCodec(0)
    stream = torch.cuda.ExternalStream(codec.native.stream)
    dev = torch.device("cuda", 0)
    n, size = max(1, int(65536 * args.scale)), 65536
    cap = codec.lib.achip_lz4_max_compressed_length(size)
    i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dev)  # noqa: E731
    p_off = torch.arange(n, dtype=torch.int64, device=dev) * size
    c_off = torch.arange(n, dtype=torch.int64, device=dev) * cap
    p_len, c_cap, c_len, st, d_len, d_st = i32(size), i32(cap), i32(0), i32(0), i32(0), i32(0)
    eo = torch.zeros(n, dtype=torch.int64, device=dev)
    slots = torch.empty(n * cap + 64, dtype=torch.uint8, device=dev)
    back = torch.empty(n * size + 64, dtype=torch.uint8, device=dev)
    results = []
    for kind in ("corpus", "fragments"):
        plain = bench.gen_data(torch, dev, kind, n, size, 0.5, 77)
        torch.cuda.synchronize()  # (the tensors are made on torch's stream, the calls run on the context's)

        def compress_call():
            codec.launch(OP_LZ4_COMPRESS, plain, p_off, p_len, slots, c_off, c_cap, c_len, st, eo, n)

        for variant, what in VARIANTS:
            codec.native.set_option("lz4.compress.variant", variant)
            for acceleration in ACCELERATIONS:
                codec.native.set_lz4_acceleration(acceleration)
                for _ in range(3):
                    compress_call()
                codec.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(launches):
                    compress_call()
                e1.record(stream)
                e1.synchronize()
                ms = e0.elapsed_time(e1) / launches
                assert int((st != 0).sum().item()) == 0, "the encoder failed: statuses %s" % torch.unique(st).tolist()[:8]
                compressed = int(c_len.sum(dtype=torch.int64).item())
                codec.launch(OP_LZ4_DECOMPRESS, slots, c_off, c_len, back, p_off, p_len, d_len, d_st, eo, n)
                codec.synchronize()
                assert int((d_st != 0).sum().item()) == 0 and bool((back[:n * size] == plain).all().item()), "the output does not decode to the plaintext"
                r = {"batch": kind, "blocks": n, "variant": variant, "form": what, "acceleration": acceleration, "ms": round(ms, 3),
                     "gib_s": round(n * size / (ms / 1e3) / 2**30, 1), "ratio": round(compressed / (n * size), 4)}
                results.append(r)
                print(json.dumps(r), flush=True)
        codec.native.set_lz4_acceleration(1)
        codec.native.set_option("lz4.compress.variant", 4)
        del plain
    lines = ["achip_lz4_compress_batch by acceleration (Lz4Compressor.create(acceleration)): %d blocks of 64 KiB per batch, mean of %d launches after 3 warm-ups," % (n, launches),
             "device events on the context's stream; every output decoded by the GPU decoder and compared once (tools/lz4_accel_rate.py).  GiB/s of plaintext.",
             "", "%-10s %-18s %13s %9s %8s %18s %12s" % ("batch", "form", "acceleration", "ms", "GiB/s", "compressed/plain", "vs a = 1")]
    for r in results:
        base = next(b for b in results if (b["batch"], b["variant"], b["acceleration"]) == (r["batch"], r["variant"], 1))
        lines.append("%-10s %-18s %13d %9.3f %8.1f %18.4f %11.2fx" % (r["batch"], r["form"], r["acceleration"], r["ms"], r["gib_s"], r["ratio"], base["ms"] / r["ms"]))
    print("\n" + "\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
