"""Rates of the streaming hashers (achip_hash_states_*) on the GPU, with the one-shot batch over the same bytes IN THE SAME RUN beside each
line -- the one-shot figure of the run is the yardstick, not a number from another day.

Shapes: 65 536 states x 64 KiB in one update; the same in 16 updates of 4 KiB; 4 096 states x 1 MiB in 64 KiB pieces; 1 048 576 states x
64-byte pieces, four rounds; and, for each algorithm, the digest of 65 536 states alone.  For every shape and algorithm: device buffers of
random bytes (distinct for every state), a warm-up of both forms, then --rounds alternating rounds (stream, one-shot, stream, ...) timed
with device events on the context's stream; the states are reset outside the timed span.  GiB/s = bytes absorbed / median time.

    python tools/xxh_stream_rate.py [--shapes 64k,64k16,1m,64b,digest] [--rounds 5] [--out profiles/xxh_stream_rate.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALGOS = ["xxh32", "xxh64", "xxh3_64", "xxh3_128"]
# key: (title, states, bytes per state, piece)
SHAPES = {
    "64k": ("65536 states x 64 KiB, one update", 65536, 65536, 65536),
    "64k16": ("65536 states x 64 KiB, 16 updates of 4 KiB", 65536, 65536, 4096),
    "1m": ("4096 states x 1 MiB, 16 updates of 64 KiB", 4096, 1 << 20, 65536),
    "64b": ("1048576 states x 256 B, 4 updates of 64 B", 1048576, 256, 64),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="64k,64k16,1m,64b,digest")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xxh_stream_rate.txt"))
    args = ap.parse_args()
    import torch
    import aircompressor_amd as A
    if not torch.cuda.is_available():
        sys.exit("xxh_stream_rate.py needs a GPU")
    nat = A.HipNative(0)
    lib, ctx = nat.lib, nat.ctx
    stream = torch.cuda.ExternalStream(nat.stream)
    dev = torch.device("cuda", 0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    one_shot = [lib.achip_xxhash32_batch, lib.achip_xxhash64_batch, lib.achip_xxhash3_64_batch, lib.achip_xxhash3_128_batch]
    seed = 0x9E3779B1
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / 1e3

    say("%-46s %-9s %11s %9s %11s %9s %7s" % ("shape", "hash", "stream ms", "GiB/s", "one-shot ms", "GiB/s", "ratio"))
    for key in args.shapes.split(","):
        if key == "digest":
            continue
        title, n, size, piece = SHAPES[key]
        src = torch.randint(0, 256, (n * size + 64,), dtype=torch.uint8, device=dev)
        base = torch.arange(n, dtype=torch.int64, device=dev) * size
        offs = [base + piece * r for r in range(size // piece)]
        plen = torch.full((n,), piece, dtype=torch.int32, device=dev)
        wlen = torch.full((n,), size, dtype=torch.int32, device=dev)
        out = torch.empty(2 * n, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for algo, name in enumerate(ALGOS):
            st = A.HipHashStates(algo, n, native_ctx=nat)

            def run_stream():
                for o in offs:
                    st.update(src, o, plen)

            def run_one_shot():
                sd = ctypes.c_int32(seed - (1 << 32) if seed >> 31 else seed) if algo == 0 else ctypes.c_int64(seed)
                assert one_shot[algo](ctx, p(src), p(base), p(wlen), sd, p(out), n) == 0

            st.reset(seed)
            run_stream()
            run_one_shot()
            nat.synchronize()
            ts, to = [], []
            for _ in range(args.rounds):
                st.reset(seed)
                nat.synchronize()
                ts.append(timed(run_stream))
                to.append(timed(run_one_shot))
            a, b = statistics.median(ts), statistics.median(to)
            total = n * size
            say("%-46s %-9s %11.3f %9.1f %11.3f %9.1f %7.3f" % (title, name, a * 1e3, total / a / 2**30, b * 1e3, total / b / 2**30, b / a))
            st.close()
        del src, base, offs, plen, wlen, out
        torch.cuda.empty_cache()
    if "digest" in args.shapes.split(","):
        n = 65536
        say("")
        say("%-46s %-9s %11s %14s" % ("digest alone", "hash", "median ms", "states / s"))
        src = torch.randint(0, 256, (n * 1000 + 64,), dtype=torch.uint8, device=dev)
        base = torch.arange(n, dtype=torch.int64, device=dev) * 1000
        plen = torch.full((n,), 1000, dtype=torch.int32, device=dev)
        out = torch.empty(2 * n, dtype=torch.int64, device=dev)
        for algo, name in enumerate(ALGOS):
            st = A.HipHashStates(algo, n, native_ctx=nat)
            st.reset(seed).update(src, base, plen)
            st.digest(out)
            nat.synchronize()
            t = statistics.median([timed(lambda: st.digest(out)) for _ in range(args.rounds)])
            say("%-46s %-9s %11.4f %14.3e" % ("65536 states (1 000 bytes absorbed each)", name, t * 1e3, n / t))
            st.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    nat.close()


if __name__ == "__main__":
    main()
