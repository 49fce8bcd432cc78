"""What packing a compressed batch costs: achip_pack_outputs next to the compress call that produced its input and next to the runtime's own device-to-device
copy of the same number of bytes, in one process, on the same buffers.

Three shapes, each at align 1 and 16: LZ4 compress of 65 536 x 64 KiB fragments blocks, of 65 536 x 64 KiB corpus blocks (bench.py's generators), and 4 194 304
items of 1..40 bytes with synthetic lengths (no compress call: the slots are filled with random bytes).  Before anything is timed the dense buffer is checked:
the LZ4 shapes are decoded from it (srcOff = packedOff, srcLen = packedLen) and compared with the plaintext, the synthetic shape is compared item by item on a
sample.  Then three warm-ups and --rounds alternating rounds, each call timed with device events on the context's stream; medians are reported.  The aim
 is pack within 1.5x of the copy on the two 64 KiB shapes, and a small fraction of the compress call.

    python tools/pack_rate.py [--rounds 7] [--scale 1.0] [--out profiles/pack_rate.txt]

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/pack_rate.py --rounds 1`.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("lz4 fragments", "fragments", 65536, 65536), ("lz4 corpus", "corpus", 65536, 65536), ("synthetic 1..40", None, 4194304, 40))
OP_LZ4_DECOMPRESS, OP_LZ4_COMPRESS = 0, 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0, help="development aid: items per shape times this")
    ap.add_argument("--shapes", default="0,1,2", help="which of the three shapes to run")
    ap.add_argument("--slot-align", type=int, default=1, help="round the compress call's slot size up to this: 16 gives the copy sources that are co-aligned with an align-16 stream")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    import aircompressor_amd as A
    import bench
    if not torch.cuda.is_available():
        sys.exit("pack_rate.py needs a GPU")
    codec = A.HipBatchCodec(0)
    stream = torch.cuda.ExternalStream(codec.native.stream)
    dev = torch.device("cuda", 0)
    lines, results = [], []

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for label, kind, n, size in [SHAPES[int(k)] for k in args.shapes.split(",")]:
        n = max(1, int(n * args.scale))
        i64 = lambda v: torch.full((n,), v, dtype=torch.int64, device=dev)  # noqa: E731
        i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dev)  # noqa: E731
        st, eo = i32(0), i64(0)
        compress_call = None
        if kind is not None:
            plain = bench.gen_data(torch, dev, kind, n, size, 0.5, 77)
            cap = (codec.lib.achip_lz4_max_compressed_length(size) + args.slot_align - 1) // args.slot_align * args.slot_align
            p_off = torch.arange(n, dtype=torch.int64, device=dev) * size
            p_len = i32(size)
            c_off = torch.arange(n, dtype=torch.int64, device=dev) * cap
            c_cap = i32(cap)
            slots = torch.empty(n * cap + 64, dtype=torch.uint8, device=dev)
            c_len = i32(0)

            def compress_call():
                codec.launch(OP_LZ4_COMPRESS, plain, p_off, p_len, slots, c_off, c_cap, c_len, st, eo, n)

            torch.cuda.synchronize()  # (the tensors are made on torch's stream, the calls run on the context's)
            compress_call()
            codec.synchronize()
            assert int((st != 0).sum().item()) == 0, "the encoder failed: statuses %s, first at block %d" % (torch.unique(st).tolist()[:8], int(torch.nonzero(st)[0].item()))
        else:
            cap = size + 3
            gen = torch.Generator(device=dev)
            gen.manual_seed(5)
            c_off = torch.arange(n, dtype=torch.int64, device=dev) * cap + 1
            c_len = torch.randint(1, size + 1, (n,), dtype=torch.int32, device=dev, generator=gen)
            slots = torch.randint(0, 256, (n * cap + 64,), dtype=torch.uint8, device=dev, generator=gen)
        for align in (1, 16):
            p_off_out, p_len_out, total = i64(-7), i32(-7), torch.full((3,), -7, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            codec.pack_outputs(slots, c_off, c_len, st, n, align, None, 0, p_off_out, p_len_out, total)
            codec.synchronize()
            dense_bytes = int(total[0].item())
            dense = torch.full((dense_bytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
            other = torch.empty(dense_bytes + 64, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()

            def pack_call():
                codec.pack_outputs(slots, c_off, c_len, st, n, align, dense, dense_bytes, p_off_out, p_len_out, total)

            def copy_call():
                with torch.cuda.stream(stream):
                    other[:dense_bytes].copy_(dense[:dense_bytes], non_blocking=True)

            pack_call()
            codec.synchronize()
            assert total.tolist()[1:] == [0, 1] and bool((dense[dense_bytes:] == 0xA5).all().item()), "the pack call did not copy, or wrote past the stream"
            if kind is not None:  # the dense buffer decodes to the plaintext
                out = torch.empty(n * size + 64, dtype=torch.uint8, device=dev)
                o_len, d_st = i32(-7), i32(-7)
                torch.cuda.synchronize()
                codec.launch(OP_LZ4_DECOMPRESS, dense, p_off_out, p_len_out, out, p_off, p_len, o_len, d_st, eo, n)
                codec.synchronize()
                assert int((d_st != 0).sum().item()) == 0 and bool((out[:n * size] == plain).all().item()), "the dense buffer does not decode to the plaintext"
                del out
            else:
                host_dense, host_slots = dense.cpu().numpy(), slots.cpu().numpy()
                offs, lens, src = p_off_out.cpu().numpy(), p_len_out.cpu().numpy(), c_off.cpu().numpy()
                assert (lens == c_len.cpu().numpy()).all()
                for i in list(range(0, n, max(1, n // 2000))) + [n - 1]:
                    assert (host_dense[offs[i]:offs[i] + lens[i]] == host_slots[src[i]:src[i] + lens[i]]).all(), "item %d differs" % i
            calls = [("pack", pack_call), ("copy", copy_call)] + ([("compress", compress_call)] if compress_call else [])
            for _ in range(3):
                for _, call in calls:
                    call()
            codec.synchronize()
            times = {what: [] for what, _ in calls}
            for _ in range(args.rounds):
                for what, call in calls:
                    times[what].append(timed(call))
            med = {what: statistics.median(v) for what, v in times.items()}
            r = {"shape": label, "items": n, "align": align, "dense_bytes": dense_bytes, "pack_ms": round(med["pack"], 4), "copy_ms": round(med["copy"], 4),
                 "compress_ms": round(med["compress"], 4) if "compress" in med else None, "pack_over_copy": round(med["pack"] / med["copy"], 3),
                 "pack_gib_s": round(dense_bytes / (med["pack"] / 1e3) / 2**30, 1), "copy_gib_s": round(dense_bytes / (med["copy"] / 1e3) / 2**30, 1),
                 "runs_ms": {what: [round(x, 4) for x in v] for what, v in times.items()}}
            results.append(r)
            print(json.dumps(r), flush=True)
            del dense, other
        del slots
        torch.cuda.empty_cache()
    lines.append("achip_pack_outputs (scan + copy) beside the same run's device-to-device copy of total[0] bytes and the compress call that made its input;")
    lines.append("medians of %d alternating rounds, device events on the context's stream (tools/pack_rate.py)" % args.rounds)
    lines.append("")
    lines.append("%-16s %8s %5s %13s %9s %9s %11s %10s %10s %10s" % ("shape", "items", "align", "dense bytes", "pack ms", "copy ms", "compress ms", "pack/copy", "pack GiB/s", "copy GiB/s"))
    for r in results:
        lines.append("%-16s %8d %5d %13d %9.3f %9.3f %11s %10.2f %10.1f %10.1f" % (r["shape"], r["items"], r["align"], r["dense_bytes"], r["pack_ms"], r["copy_ms"],
                     "%.3f" % r["compress_ms"] if r["compress_ms"] is not None else "-", r["pack_over_copy"], r["pack_gib_s"], r["copy_gib_s"]))
    aim = [r for r in results if r["compress_ms"] is not None]
    lines.append("")
    lines.append("aim (pack within 1.5x of the copy on the two 64 KiB shapes): %s" % ("met on every row" if all(r["pack_over_copy"] <= 1.5 for r in aim) else "MISSED on " + ", ".join(
        "%s/align %d (%.2fx)" % (r["shape"], r["align"], r["pack_over_copy"]) for r in aim if r["pack_over_copy"] > 1.5)))
    print("\n" + "\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
