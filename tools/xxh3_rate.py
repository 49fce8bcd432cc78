"""XXH3-64, XXH3-128 and XXH64 batch rates on the GPU, in one process, on the same device buffers.

For every shape: one set of device buffers (random bytes made on the device, distinct data for every buffer), a warm-up of each
hash, then five alternating rounds (XXH3-64, XXH3-128, XXH64, XXH3-64, ...) each timed with device events on the context's stream.
Bytes moved = the buffer lengths + srcOff (8 B) + srcLen (4 B) + the hashes (8 or 16 B) per buffer; GiB/s from the median time and
the fraction of the 8 TB/s HBM peak.  Prints one JSON line per (shape, hash) and a table (and writes the rows to --out if given).

    python tools/xxh3_rate.py [--shapes 64k,1m,64b,mixed] [--rounds 5] [--out xxh3_rate.json]

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/xxh3_rate.py --rounds 1`.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12
SHAPES = {
    "64k": ("65536 x 64 KiB", 65536, 65536),
    "1m": ("4096 x 1 MiB", 4096, 1 << 20),
    "64b": ("16777216 x 64 B", 16777216, 64),
    "mixed": ("16384 x log-uniform 0-256 KiB, seeded", 16384, None),
}


def make_shape(torch, key, dev):
    name, n, size = SHAPES[key]
    g = torch.Generator(device="cpu").manual_seed(1234)
    if size is None:  # log-uniform lengths in [0, 256 KiB]: exp(U(0, ln(262145))) - 1
        u = torch.rand(n, generator=g, dtype=torch.float64)
        lengths = (torch.exp(u * torch.log(torch.tensor(262145.0, dtype=torch.float64))) - 1).floor().to(torch.int64)
    else:
        lengths = torch.full((n,), size, dtype=torch.int64)
    offs = torch.zeros(n, dtype=torch.int64)
    offs[1:] = torch.cumsum(lengths, 0)[:-1]
    total = int(lengths.sum())
    src = torch.randint(0, 256, (total + 64,), dtype=torch.uint8, device=dev)
    return name, n, total, src, offs.to(dev), lengths.to(torch.int32).to(dev)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="64k,1m,64b,mixed")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    import aircompressor_amd as A
    if not torch.cuda.is_available():
        sys.exit("xxh3_rate.py needs a GPU")
    nat = A.HipNative(0)
    lib, ctx = nat.lib, nat.ctx
    stream = torch.cuda.ExternalStream(nat.stream)
    dev = torch.device("cuda", 0)
    hashes = [("xxh3_64", lib.achip_xxhash3_64_batch, 1), ("xxh3_128", lib.achip_xxhash3_128_batch, 2), ("xxh64", lib.achip_xxhash64_batch, 1)]
    results = []
    for key in args.shapes.split(","):
        name, n, total, src, offs, lens = make_shape(torch, key, dev)
        seed = 0x9E3779B1 if key == "mixed" else 0
        out = torch.empty(2 * n, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def launch(fn):
            r = fn(ctx, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(offs.data_ptr()), ctypes.c_void_p(lens.data_ptr()), ctypes.c_int64(seed),
                   ctypes.c_void_p(out.data_ptr()), n)
            assert r == 0, r

        for _, fn, _ in hashes:  # warm-up
            launch(fn)
        assert lib.achip_ctx_synchronize(ctx) == 0
        times = {h: [] for h, _, _ in hashes}
        for _ in range(args.rounds):
            for h, fn, _ in hashes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch(fn)
                e1.record(stream)
                e1.synchronize()
                times[h].append(e0.elapsed_time(e1) / 1e3)
        for h, _, words in hashes:
            t = statistics.median(times[h])
            moved = total + 12 * n + 8 * words * n
            row = {"shape": name, "hash": h, "buffers": n, "bytes_hashed": total, "bytes_moved": moved, "median_ms": round(t * 1e3, 4),
                   "runs_ms": [round(x * 1e3, 4) for x in times[h]], "gib_s": round(moved / t / 2**30, 1), "frac_of_8TBs": round(moved / t / PEAK, 3)}
            results.append(row)
            print(json.dumps(row), flush=True)
        del src, offs, lens, out
        torch.cuda.empty_cache()
    print("\n%-40s %-9s %10s %9s %7s" % ("shape", "hash", "median ms", "GiB/s", "of 8TB/s"))
    for r in results:
        print("%-40s %-9s %10.3f %9.1f %7.3f" % (r["shape"], r["hash"], r["median_ms"], r["gib_s"], r["frac_of_8TBs"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    nat.close()


if __name__ == "__main__":
    main()
