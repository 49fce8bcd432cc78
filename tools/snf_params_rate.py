"""What the constructor arguments of the x-snappy-framed streams cost or buy on an MI355X: achip_snappyframed_decompress_batch with verifyChecksums on and off, and
achip_snappyframed_compress_batch with writeChecksums on and off at block sizes 4 KiB, 16 KiB and 64 KiB, the defaults in the same run.

Batches: 1 024 streams of 4 MiB, fragments and corpus (bench.py's generators and its container shape).  Per row: two warm-up launches, then the mean of --launches
timed launches, device events on the context's stream; GiB/s of plaintext.  Every encode row's output is decoded by the GPU reader and compared with the plaintext,
once.  Nothing is asserted about speed: a row that is slower than the default stays in the file.

    python tools/snf_params_rate.py [--launches 5] [--scale 1.0] [--out profiles/snf_params_rate.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCK_SIZES = (65536, 16384, 4096)
OP_D, OP_C = 8, 9


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="development aid: streams per batch times this")
    ap.add_argument("--out")
    args = ap.parse_args()
    launches = max(2, args.launches)
    import torch
    import aircompressor_amd as A
    import bench
    if not torch.cuda.is_available():
        sys.exit("snf_params_rate.py needs a GPU")
    codec = A.HipBatchCodec(0)
    native = codec.native
    stream = torch.cuda.ExternalStream(native.stream)
    dev = torch.device("cuda", 0)
    n, fs = max(1, int(1024 * args.scale)), 4 << 20
    cap = codec.lib.achip_snappyframed_max_compressed_length_for(fs, min(BLOCK_SIZES))  # (the largest of the bounds: one layout for every row)
    cstride = (cap + 15) // 16 * 16
    i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dev)  # noqa: E731
    p_off = torch.arange(n, dtype=torch.int64, device=dev) * fs
    c_off = torch.arange(n, dtype=torch.int64, device=dev) * cstride
    p_len, c_cap, c_len, st, d_len = i32(fs), i32(cap), i32(0), i32(0), i32(0)
    eo = torch.zeros(n, dtype=torch.int64, device=dev)
    comp = torch.empty(n * cstride + 64, dtype=torch.uint8, device=dev)
    back = torch.empty(n * fs + 64, dtype=torch.uint8, device=dev)
    results = []

    def timed(fn):
        for _ in range(2):
            fn()
        codec.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(launches):
            fn()
        e1.record(stream)
        e1.synchronize()
        assert int((st != 0).sum().item()) == 0, "statuses %s" % torch.unique(st).tolist()[:8]
        return e0.elapsed_time(e1) / launches

    def row(kind, what, ms, **more):
        r = dict({"batch": kind, "row": what, "ms": round(ms, 3), "gib_s": round(n * fs / (ms / 1e3) / 2**30, 1)}, **more)
        results.append(r)
        print(json.dumps(r), flush=True)

    for kind in ("fragments", "corpus"):
        plain = bench.gen_data(torch, dev, kind, n * (fs // 65536), 65536, 0.5, 99)
        torch.cuda.synchronize()
        encode = lambda: codec.launch(OP_C, plain, p_off, p_len, comp, c_off, c_cap, c_len, st, eo, n)  # noqa: E731
        decode = lambda: codec.launch(OP_D, comp, c_off, c_len, back, p_off, p_len, d_len, st, eo, n)  # noqa: E731
        for block_size in BLOCK_SIZES:
            for checksums in (True, False):
                native.set_snappyframed_writer(checksums, block_size, 0.85)
                ms = timed(encode)
                compressed = int(c_len.sum(dtype=torch.int64).item())
                native.set_snappyframed_verify_checksums(checksums)
                back.zero_()
                decode()
                codec.synchronize()
                assert int((st != 0).sum().item()) == 0 and bool((back[:n * fs] == plain).all().item()), "the output does not decode to the plaintext"
                default = block_size == 65536 and checksums
                row(kind, "encode, block %d, checksums %s%s" % (block_size, "on" if checksums else "off", " (default)" if default else ""), ms, ratio=round(n * fs / compressed, 3))
            # the reader over streams of this block size, written with checksums: verify on (the default) and off
            native.set_snappyframed_writer(True, block_size, 0.85)
            encode()
            codec.synchronize()
            for verify in (True, False):
                native.set_snappyframed_verify_checksums(verify)
                ms = timed(decode)
                assert bool((back[:n * fs] == plain).all().item())
                default = block_size == 65536 and verify
                row(kind, "decode, block %d, verify %s%s" % (block_size, "on" if verify else "off", " (default)" if default else ""), ms)
        native.set_snappyframed_writer(True, 65536, 0.85)
        native.set_snappyframed_verify_checksums(True)
        del plain
    lines = ["x-snappy-framed streams by constructor argument (achip_ctx_set_snappyframed_writer / _verify_checksums): %d streams of 4 MiB per batch, mean of %d launches" % (n, launches),
             "after 2 warm-ups, device events on the context's stream; every encode row decoded by the GPU reader and compared once (tools/snf_params_rate.py).",
             "GiB/s of plaintext; `vs default`: the default row's time over this row's (encode against the default encode, decode against the default decode).",
             "", "%-10s %-44s %9s %8s %8s %12s" % ("batch", "row", "ms", "GiB/s", "ratio", "vs default")]
    for r in results:
        base = next(b for b in results if b["batch"] == r["batch"] and b["row"].startswith(r["row"][:6]) and b["row"].endswith("(default)"))
        lines.append("%-10s %-44s %9.3f %8.1f %8s %11.2fx" % (r["batch"], r["row"], r["ms"], r["gib_s"], r.get("ratio", ""), base["ms"] / r["ms"]))
    print("\n" + "\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
