"""What the history path of the LZ4 frame reader costs on an MI355X (achip_ctx_set_lz4frame_linked_blocks): 1 024 frames of 4 MiB decoded three ways in one run,

    linked        64 KiB blocks, the block-independence bit clear: matches reach across the block boundaries
    independent   64 KiB blocks, the same content, the bit set
    one block     the same content as a single 4 MiB block

on text (bench.py's corpus generator) and on fragments data (bench.py's generator, ratio 0.5).  All three come from one encoder -- the greedy one of
tests/lz4_linked_ref.py: one hash table over the whole content; confined to the block for the independent form -- so what differs between the rows is the linking
and nothing else.  One 4 MiB plaintext per kind is encoded on the CPU (a few seconds each; --cache keeps the frames in a file) and the frame stands 1 024 times
in the batch, each copy with source and destination of its own.

A frame of linked blocks has one path, the wavefront-per-item kernel (lz4frame_decompress_kernel).  The comparison that matters is therefore linked against the
independent frames FORCED ONTO THE SAME KERNEL -- context option lz4frame.decompress.variant 0 -- : that difference is the cost of the history (the ring primed
from memory once per block, matches read from the block in front).  The list path's rows (variant 2, the default for independent frames: their blocks as one
batch through the block decoders) stand beside it: what a parallel path for linked frames could gain.

Per row: three warm-up launches, then the mean of --launches timed launches (device events on the context's stream), GiB/s of plaintext; after the timing the
output of every copy is compared with the plaintext, once.  Nothing is asserted about speed.

    python tools/lz4_linked_rate.py [--launches 5] [--frames 1024] [--cache FILE] [--out profiles/lz4_linked_rate.txt]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OP_LZ4FRAME_DECOMPRESS = 6
FRAME_BYTES, BLOCK = 4 << 20, 65536
# (form, linked flag of the encoder and the frame, block size, the frame's block-maximum id)
FORMS = (("linked 64 KiB blocks", True, BLOCK, 4), ("independent 64 KiB blocks", False, BLOCK, 4), ("one 4 MiB block", False, FRAME_BYTES, 7))
# (form, reader variant, setting): the rows of the table
ROWS = ((0, 0, 1, "wavefront per item (the only path)"), (1, 0, 0, "wavefront per item (variant 0)"), (2, 0, 0, "wavefront per item (variant 0)"),
        (1, 2, 0, "list path (variant 2, default)"), (2, 2, 0, "list path (variant 2, default)"))


def frames_for(kind, cache):
    """-> (plaintext, [frame per form]) for one kind, encoded here or taken from the cache file"""
    from tests import lz4_linked_ref as ref
    if cache and os.path.exists(cache):
        z = np.load(cache)
        if "%s_plain" % kind in z:
            return z["%s_plain" % kind].tobytes(), [z["%s_%d" % (kind, k)].tobytes() for k in range(len(FORMS))]
    import torch
    import bench
    plain = bench.gen_data(torch, torch.device("cpu"), kind, FRAME_BYTES // BLOCK, BLOCK, 0.5, 77).numpy().tobytes()
    frames = []
    for _, linked, block, size_id in FORMS:
        f = ref.frame(ref.greedy_blocks(plain, block, linked=linked), linked=linked, size_id=size_id)
        assert f.plain == plain
        frames.append(f.data)
    return plain, frames


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--cache", help="an .npz file the encoded frames are kept in (made when missing)")
    ap.add_argument("--encode-only", action="store_true", help="fill the cache and stop (no GPU needed)")
    ap.add_argument("--out")
    args = ap.parse_args()
    kinds = ("corpus", "fragments")
    data = {kind: frames_for(kind, args.cache) for kind in kinds}
    if args.cache and not os.path.exists(args.cache):
        np.savez(args.cache, **{"%s_plain" % k: np.frombuffer(p, dtype=np.uint8) for k, (p, _) in data.items()},
                 **{"%s_%d" % (k, i): np.frombuffer(f, dtype=np.uint8) for k, (_, fs) in data.items() for i, f in enumerate(fs)})
    if args.encode_only:
        for kind, (plain, frames) in data.items():
            print(kind, [round(len(f) / len(plain), 4) for f in frames])
        return
    import torch
    import aircompressor_amd as A
    if not torch.cuda.is_available():
        sys.exit("lz4_linked_rate.py needs a GPU")
    codec = A.HipBatchCodec(0)
    stream = torch.cuda.ExternalStream(codec.native.stream)
    dev = torch.device("cuda", 0)
    n = args.frames
    i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dev)  # noqa: E731
    d_off = torch.arange(n, dtype=torch.int64, device=dev) * FRAME_BYTES
    d_cap, out_len, st = i32(FRAME_BYTES), i32(0), i32(0)
    eo = torch.zeros(n, dtype=torch.int64, device=dev)
    dst = torch.empty(n * FRAME_BYTES + 64, dtype=torch.uint8, device=dev)
    results = []
    for kind in kinds:
        plain, frames = data[kind]
        d_plain = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).to(dev)
        for form, variant, accept, path in ROWS:
            frame = frames[form]
            stride = (len(frame) + 15) // 16 * 16
            one = np.zeros(stride, dtype=np.uint8)
            one[:len(frame)] = np.frombuffer(frame, dtype=np.uint8)
            src = torch.from_numpy(one).to(dev).repeat(n)
            s_off = torch.arange(n, dtype=torch.int64, device=dev) * stride
            s_len = i32(len(frame))
            codec.native.set_option("lz4frame.decompress.variant", variant)
            codec.native.set_lz4frame_linked_blocks(accept)
            torch.cuda.synchronize()  # (the tensors are made on torch's stream, the calls run on the context's)

            def call():
                codec.launch(OP_LZ4FRAME_DECOMPRESS, src, s_off, s_len, dst, d_off, d_cap, out_len, st, eo, n)

            for _ in range(3):
                call()
            codec.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.launches):
                call()
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1) / args.launches
            assert int((st != 0).sum().item()) == 0 and int((out_len != FRAME_BYTES).sum().item()) == 0, "the reader failed: statuses %s" % torch.unique(st).tolist()[:8]
            assert bool((dst[:n * FRAME_BYTES].view(n, FRAME_BYTES) == d_plain.unsqueeze(0)).all().item()), "the output is not the plaintext"
            r = {"data": kind, "frames": n, "form": FORMS[form][0], "path": path, "compressed_ratio": round(len(frame) / FRAME_BYTES, 4), "ms": round(ms, 3),
                 "gib_s": round(n * FRAME_BYTES / (ms / 1e3) / 2**30, 1)}
            results.append(r)
            print(json.dumps(r), flush=True)
            del src
    codec.native.set_option("lz4frame.decompress.variant", 2)
    codec.native.set_lz4frame_linked_blocks(False)
    lines = ["LZ4 frame reader: frames of linked blocks against independent ones (tools/lz4_linked_rate.py)",
             "%d frames of 4 MiB per batch, one encoder for all forms (tests/lz4_linked_ref.py: greedy, one table over the content), %d timed launches per row, "
             "GiB/s of plaintext" % (n, args.launches), "",
             "%-10s %-28s %-38s %10s %9s %8s" % ("data", "form", "path", "compressed", "ms", "GiB/s")]
    for r in results:
        lines.append("%-10s %-28s %-38s %10.4f %9.3f %8.1f" % (r["data"], r["form"], r["path"], r["compressed_ratio"], r["ms"], r["gib_s"]))
    lines.append("")
    for kind in kinds:
        rate = {(r["form"], r["path"][:4]): r["gib_s"] for r in results if r["data"] == kind}
        linked, same = rate[(FORMS[0][0], "wave")], rate[(FORMS[1][0], "wave")]
        lines.append("%s: linked / independent on the same kernel = %.3f (the cost of the history path: %+.1f %%); the list path on the independent frames is %.2f x the "
                     "linked rate" % (kind, linked / same, 100.0 * (linked / same - 1.0), rate[(FORMS[1][0], "list")] / linked))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
