"""What reading and writing a long stream a window at a time costs next to the one-shot call over the same stream: achip_window_decompress_batch /
achip_window_compress_batch over ONE device-resident stream, in windows of 4 / 16 / 64 / 256 MiB, against achip_*_decompress_batch / _compress_batch with the
whole stream as one item, in one process on the same buffers.

Streams: 1 GiB of plaintext as a Hadoop LZ4 stream and as an x-snappy-framed stream, each from fragments and from corpus data (bench.py's generators), written by the
one-shot writer on the device.  The window loop is the standard one -- call, read `consumed` / `outLen` / `stop` back (the only wait), advance -- so its time holds
one host round trip per window; it is taken with the host's clock around the whole loop, the one-shot call's with device events.  Before anything is timed the
windows' results are compared with the plaintext (reader) and with the one-shot writer's stream (writer).  Then one stream the one-shot calls cannot take: 3 GiB of
fragments written as a Hadoop LZ4 stream in 256 MiB windows and read back in 64 MiB windows.  Medians of --rounds runs.

    python tools/window_rate.py [--rounds 3] [--gib 1.0] [--long-gib 3.0] [--out profiles/window_rate.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIRST, LAST = 1, 2
STOP_END, STOP_NEED_INPUT, STOP_NEED_ROOM, STOP_FAILED = 0, 1, 2, 3
FORMATS = (("hadoop lz4", 10, 11), ("x-snappy-framed", 8, 9))  # (label, decode op, compress op)
WINDOWS_MIB = (4, 16, 64, 256)
INT_MAX_ROOM = 0x7FFFFF00


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0, help="plaintext of the streams the one-shot calls are compared on")
    ap.add_argument("--long-gib", type=float, default=3.0, help="plaintext of the stream only the windows can take (0: leave it out)")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    import aircompressor_amd as A
    import bench
    if not torch.cuda.is_available():
        sys.exit("window_rate.py needs a GPU")
    codec = A.HipBatchCodec(0)
    lib = codec.lib
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(codec.native.stream)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    with torch.cuda.stream(stream):
        wide = torch.zeros(5, dtype=torch.int64, device=dev)    # srcOff, dstOff, errOffset, consumed, need
        narrow = torch.zeros(6, dtype=torch.int32, device=dev)  # srcLen, dstCap, outLen, status, stop, flags
        wide_host = torch.zeros(5, dtype=torch.int64).pin_memory()
        narrow_host = torch.zeros(6, dtype=torch.int32).pin_memory()

        def item(src_off, src_len, dst_off, dst_cap, flags):
            wide_host[0], wide_host[1] = src_off, dst_off
            narrow_host[0], narrow_host[1], narrow_host[5] = src_len, dst_cap, flags
            wide.copy_(wide_host, non_blocking=True)
            narrow.copy_(narrow_host, non_blocking=True)
            w, n = wide.data_ptr(), narrow.data_ptr()
            return dict(src_off=w, dst_off=w + 8, err=w + 16, consumed=w + 24, need=w + 32, src_len=n, dst_cap=n + 4, out_len=n + 8, status=n + 12, stop=n + 16, flags=n + 20)

        def one_shot(op, src, src_len, dst):
            """-> (ms, outLen)"""
            p = item(0, src_len, 0, min(dst.numel(), INT_MAX_ROOM), 0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            codec.launch(op, src, p["src_off"], p["src_len"], dst, p["dst_off"], p["dst_cap"], p["out_len"], p["status"], p["err"], 1)
            e1.record(stream)
            e1.synchronize()
            got = narrow.cpu()
            assert int(got[3]) == 0, "one-shot op %d failed: status %d" % (op, int(got[3]))
            return e0.elapsed_time(e1), int(got[2])

        def windowed(op, compress, src, src_len, dst, window):
            """the standard loop over one stream -> (ms by the host's clock, bytes produced, calls)"""
            call = codec.window_compress if compress else codec.window_decompress
            pos = produced = calls = 0
            first = True
            codec.synchronize()
            t0 = time.perf_counter()
            while True:
                held = min(window, src_len - pos)
                last = pos + held == src_len
                p = item(pos, held, produced, min(dst.numel() - produced, INT_MAX_ROOM), (FIRST if first else 0) | (LAST if last else 0))
                call(op, p["flags"], src, p["src_off"], p["src_len"], dst, p["dst_off"], p["dst_cap"], p["out_len"], p["status"], p["err"], 1, p["consumed"], p["stop"], p["need"])
                w, n = wide.cpu(), narrow.cpu()  # (the loop's one wait per window)
                calls += 1
                consumed, out_len, status, stop = int(w[3]), int(n[2]), int(n[3]), int(n[4])
                assert status == 0 and stop != STOP_FAILED, "window op %d failed at %d: status %d" % (op, pos, status)
                assert consumed > 0 or out_len > 0 or (last and stop == STOP_END), "no progress at %d: stop %d need %d" % (pos, stop, int(w[4]))
                pos += consumed
                produced += out_len
                first = first and out_len == 0 and consumed == 0
                if last and stop == STOP_END:
                    break
            return (time.perf_counter() - t0) * 1e3, produced, calls

        def median(call):
            call()  # warm-up: scratch, staging
            runs = [call() for _ in range(args.rounds)]
            return statistics.median(r[0] for r in runs), runs[-1]

        gib = lambda nbytes, ms: nbytes / 2**30 / (ms / 1e3)  # noqa: E731
        n_blocks = max(1, int(args.gib * 16384))
        for kind in ("fragments", "corpus"):
            plain = bench.gen_data(torch, dev, kind, n_blocks, 65536, 0.5, 77)
            n_plain = plain.numel()
            torch.cuda.synchronize()
            for label, dec_op, enc_op in FORMATS:
                bound = lib.achip_snappyframed_max_compressed_length(n_plain) if enc_op == 9 else lib.achip_hadoop_max_compressed_length(0, n_plain, 262144)
                assert bound > 0
                packed = torch.empty(bound + 64, dtype=torch.uint8, device=dev)
                again = torch.empty(bound + 64, dtype=torch.uint8, device=dev)
                decoded = torch.empty(n_plain + 64, dtype=torch.uint8, device=dev)
                enc_ms, (_, n_stream) = median(lambda: one_shot(enc_op, plain, n_plain, packed))
                dec_ms, (_, n_back) = median(lambda: one_shot(dec_op, packed, n_stream, decoded))
                assert n_back == n_plain and torch.equal(decoded[:n_plain], plain)
                say("%s, %s: %.3f GiB of plaintext, stream %.3f GiB; one-shot decode %.1f ms = %.1f GiB/s, one-shot encode %.1f ms = %.1f GiB/s (GiB/s of plaintext)"
                    % (label, kind, n_plain / 2**30, n_stream / 2**30, dec_ms, gib(n_plain, dec_ms), enc_ms, gib(n_plain, enc_ms)))
                for mib in WINDOWS_MIB:
                    window = mib << 20
                    decoded.zero_()
                    ms, (_, n_back, calls) = median(lambda: windowed(dec_op, False, packed, n_stream, decoded, window))
                    assert n_back == n_plain and torch.equal(decoded[:n_plain], plain), "windowed decode differs"
                    say("    decode in %3d MiB windows: %8.1f ms = %6.1f GiB/s, %.2f of one-shot (%d calls, %.3f ms per call)" % (mib, ms, gib(n_plain, ms), dec_ms / ms, calls, ms / calls))
                    again.zero_()
                    ms, (_, n_again, calls) = median(lambda: windowed(enc_op, True, plain, n_plain, again, window))
                    assert n_again == n_stream and torch.equal(again[:n_stream], packed[:n_stream]), "windowed encode differs from the one-shot writer"
                    say("    encode in %3d MiB windows: %8.1f ms = %6.1f GiB/s, %.2f of one-shot (%d calls, %.3f ms per call)" % (mib, ms, gib(n_plain, ms), enc_ms / ms, calls, ms / calls))
                del packed, again, decoded
            del plain
        if args.long_gib > 0:
            n_blocks = int(args.long_gib * 16384)
            plain = bench.gen_data(torch, dev, "fragments", n_blocks, 65536, 0.5, 78)
            n_plain = plain.numel()
            torch.cuda.synchronize()
            packed = torch.empty(n_plain + n_plain // 128 + (1 << 20), dtype=torch.uint8, device=dev)
            decoded = torch.empty(n_plain + 64, dtype=torch.uint8, device=dev)
            enc_ms, (_, n_stream, enc_calls) = median(lambda: windowed(11, True, plain, n_plain, packed, 256 << 20))
            dec_ms, (_, n_back, dec_calls) = median(lambda: windowed(10, False, packed, n_stream, decoded, 64 << 20))
            assert n_back == n_plain and torch.equal(decoded[:n_plain], plain), "the long stream did not come back"
            say("hadoop lz4, fragments, %.2f GiB of plaintext (beyond the one-shot calls' int32 lengths), stream %.2f GiB: encode in 256 MiB windows %.1f ms = %.1f GiB/s (%d calls), "
                "decode in 64 MiB windows %.1f ms = %.1f GiB/s (%d calls)" % (n_plain / 2**30, n_stream / 2**30, enc_ms, gib(n_plain, enc_ms), enc_calls, dec_ms, gib(n_plain, dec_ms), dec_calls))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("tools/window_rate.py --rounds %d --gib %g --long-gib %g\n" % (args.rounds, args.gib, args.long_gib) + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
