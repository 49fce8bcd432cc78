"""What the LZ4 frame writer's settings (achip_ctx_set_lz4frame_writer) cost or buy on an MI355X, the default writer as the baseline of the same run:

  default            the wavefront-per-frame writer at (4 MiB, no checksums, no content size): the parent's path, unchanged
  list, B            the block-list writer at block-maximum sizes 64 KiB, 256 KiB, 1 MiB and 4 MiB, flags off
  list, 64 KiB, ...  with block checksums, with the content checksum, with both
  list, defaults     lz4frame.compress.variant 1 at the default settings (the default writer's bytes through the block list)

and for each row the decode rate of the frames it wrote (the GPU reader at its default variant, checksums verified) and the ratio.

Batches: 1 024 frames of 4 MiB, corpus and fragments (bench.py's generators and its container shape).  Per row: two warm-up launches, then the mean of --launches
timed launches, device events on the context's stream; GiB/s of plaintext.  Every row's output is decoded and compared with the plaintext.  Nothing is asserted
about speed: a row that is slower than the baseline stays in the file.

    python tools/lz4f_writer_rate.py [--launches 5] [--scale 1.0] [--out profiles/lz4f_writer_rate.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OP_D, OP_C = 6, 7
DEFAULT = (4194304, False, False, False)
# (row, variant, settings)
ROWS = [("default writer (baseline)", 0, DEFAULT)]
ROWS += [("list, %d KiB" % (b >> 10), 0, (b, False, False, False)) for b in (65536, 262144, 1048576)]
ROWS += [("list, 4096 KiB", 1, DEFAULT)]  # (the default settings through the block list: lz4frame.compress.variant 1)
ROWS += [("list, 64 KiB, block checksums", 0, (65536, True, False, False)), ("list, 64 KiB, content checksum", 0, (65536, False, True, False)),
         ("list, 64 KiB, both checksums", 0, (65536, True, True, False))]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="development aid: frames per batch times this")
    ap.add_argument("--out")
    args = ap.parse_args()
    launches = max(2, args.launches)
    import torch
    import aircompressor_amd as A
    import bench
    if not torch.cuda.is_available():
        sys.exit("lz4f_writer_rate.py needs a GPU")
    codec = A.HipBatchCodec(0)
    native = codec.native
    stream = torch.cuda.ExternalStream(native.stream)
    dev = torch.device("cuda", 0)
    n, fs = max(1, int(1024 * args.scale)), 4 << 20
    cap = max(codec.lib.achip_lz4frame_max_compressed_length_for(fs, *(int(v) for v in s)) for _, _, s in ROWS)  # (the largest of the bounds: one layout for every row)
    cap = max(cap, codec.lib.achip_lz4frame_max_compressed_length(fs))
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

    rate = lambda ms: round(n * fs / (ms / 1e3) / 2**30, 1)  # noqa: E731
    for kind in ("corpus", "fragments"):
        plain = bench.gen_data(torch, dev, kind, n * (fs // 65536), 65536, 0.5, 99)
        torch.cuda.synchronize()
        encode = lambda: codec.launch(OP_C, plain, p_off, p_len, comp, c_off, c_cap, c_len, st, eo, n)  # noqa: E731
        decode = lambda: codec.launch(OP_D, comp, c_off, c_len, back, p_off, p_len, d_len, st, eo, n)  # noqa: E731
        for what, variant, settings in ROWS:
            native.set_option("lz4frame.compress.variant", variant)
            native.set_lz4frame_writer(*settings)
            enc_ms = timed(encode)
            compressed = int(c_len.sum(dtype=torch.int64).item())
            back.zero_()
            dec_ms = timed(decode)
            assert bool((back[:n * fs] == plain).all().item()), "the output does not decode to the plaintext"
            r = {"batch": kind, "row": what, "encode_ms": round(enc_ms, 3), "encode_gib_s": rate(enc_ms), "decode_ms": round(dec_ms, 3), "decode_gib_s": rate(dec_ms),
                 "ratio": round(n * fs / compressed, 3)}
            results.append(r)
            print(json.dumps(r), flush=True)
        native.set_option("lz4frame.compress.variant", 0)
        native.set_lz4frame_writer(*DEFAULT)
        del plain
    lines = ["LZ4 frame writer by frame setting (achip_ctx_set_lz4frame_writer, lz4frame.compress.variant): %d frames of 4 MiB per batch, mean of %d launches after 2 warm-ups," % (n, launches),
             "device events on the context's stream; every row's frames decoded by the GPU reader (default variant, checksums verified) and compared (tools/lz4f_writer_rate.py).",
             "GiB/s of plaintext; `vs default`: the default writer's encode time over this row's, same run.",
             "", "%-10s %-34s %10s %8s %12s %10s %8s %8s" % ("batch", "row", "encode ms", "GiB/s", "vs default", "decode ms", "GiB/s", "ratio")]
    for r in results:
        base = next(b for b in results if b["batch"] == r["batch"] and b["row"].startswith("default"))
        lines.append("%-10s %-34s %10.3f %8.1f %11.2fx %10.3f %8.1f %8.3f" % (r["batch"], r["row"], r["encode_ms"], r["encode_gib_s"], base["encode_ms"] / r["encode_ms"], r["decode_ms"],
                                                                              r["decode_gib_s"], r["ratio"]))
    print("\n" + "\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
