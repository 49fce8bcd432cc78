#!/usr/bin/env python3
"""bench.py -- headline measurement: batched LZ4 block decompress on MI355X through the C ABI.

    python bench.py --gpus N --steps K --warmup W          (N>1: launched by torch.distributed.run)
    python bench.py --gpus N --steps K --warmup W --full   (... and every secondary measurement after the headline)

A "step" is one pass of the hot path (achip_lz4_decompress_batch) over this rank's batch of
synthetic blocks (BASELINE.json configs[1]: 262144 x 64 KiB per GPU).  Blocks are independent, so ranks
own contiguous slices of the global batch (achip_partition_blocks) and there is NO data-path
collective; torch.distributed (gloo, CPU tensors) only provides the barrier and the max-over-ranks of the time.
Inputs (compressed blocks, offsets) and outputs are resident in HBM before the timed region.

Synthetic data: the reference's test generator shape (T/snappy/RandomGenerator.java:25-74): 100-byte
fragments made of max(1, 100*ratio) random bytes repeated; compressed ON THE GPU by the product's own
bit-exact LZ4 encoder (the oracle is never used to make inputs).  The oracle (oracle/liboracle.so, the C
restatement of the Java codec) is only timed as the `cpu_baseline` leg on rank 0 at N=1 (--full).

A plain run sets up, warms up, times the K steps, checks the last step's output bit-exact, writes it when --dump-outputs is given, and
prints the line.  Everything else -- the per-rank legs (Snappy, Zstd, the mixed corpus batch), the extras (real data, containers, xxHash,
Zstd streams), the ratio sweep, the host-facing numbers and the CPU baseline -- runs only with --full (each --no-* switch still drops its part).

Prints ONE JSON line on rank 0.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); 6290 GB/s is the measured copy ceiling


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10, help="timed steps (>= 1)")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--blocks", type=int, default=262144, help="blocks per GPU (BASELINE configs[1]: 262144)")
    p.add_argument("--block-size", type=int, default=65536)
    p.add_argument("--pool", type=int, default=4096, help="distinct blocks generated; the batch tiles them at distinct addresses")
    p.add_argument("--ratio", type=float, default=0.5, help="RandomGenerator compressibility (0.5 => LZ4 ratio ~1.9)")
    p.add_argument("--workload", default="lz4_decompress", choices=["lz4_decompress", "snappy_decompress", "lz4_compress", "snappy_compress"])
    p.add_argument("--data", default="fragments", choices=["fragments", "wordmix", "corpus", "mixed"])
    p.add_argument("--group", type=int, default=0, help="decoder lanes per block (0 = library default)")
    p.add_argument("--variant", type=int, default=-1, help="decoder variant: 5 = chosen on the device (default), 1 = LDS rings, 7 = two passes")
    p.add_argument("--parse", type=int, default=-1, help="two-pass decoders: 0 = the parser by the batch size (default), 1 = a lane per block, 2 = a wavefront per block")
    p.add_argument("--ring-class", type=int, default=-1, help="0 = compact LDS rings, 1 = large")
    p.add_argument("--compress-variant", type=int, default=-1, help="LZ4 / Snappy encoder variant: 4 = many matches per window (the default of both); LZ4 also 0 / 1, Snappy 0 .. 3 (see lz4.compress.variant / snappy.compress.variant)")
    p.add_argument("--ring-pad", type=int, default=-1, help="LDS bytes between the ring pairs of consecutive blocks (multiple of 16)")
    p.add_argument("--full", action="store_true", help="after the headline, also run the legs, extras, sweep, host-facing numbers and CPU baseline")
    p.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the timed path returned in its last step as DIR/*.npy (float64 per-block "
                   "out_len / status / err_off, float32 output bytes of a fixed seeded sample of blocks; rank 0's shard)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-extra", action="store_true")
    p.add_argument("--no-verify", action="store_true", help="DEBUG: skip the bit-exact check (kernel timing aids that leave work out); the line is then not a result")
    p.add_argument("--cpu-seconds", type=float, default=10.0, help="CPU time of the headline's cpu_baseline leg")
    p.add_argument("--cpu-leg-seconds", type=float, default=0.6, help="CPU time of each extra entry's CPU leg (per direction)")
    p.add_argument("--no-sweep", action="store_true")
    p.add_argument("--no-host-facing", action="store_true", help="skip the end_to_end (host buffers, PCIe-inclusive) and single_block_us measurements")
    p.add_argument("--no-legs", action="store_true", help="skip the per-rank legs (Snappy, Zstd configs[3], mixed corpus batch configs[4]) that run at any N")
    p.add_argument("--zstd-frames", type=int, default=65536, help="Zstd frames of 128 KiB per GPU in the configs[3] leg (a multiple of 1024)")
    p.add_argument("--dst-pad", type=int, default=0, help="development aid (decompress workloads): bytes between the outputs of consecutive blocks -- 0, the default and the headline's layout, is one contiguous output buffer; "
                   "a run with a pad is a layout experiment, not a result (the line says so in config.dst_pad)")
    p.add_argument("--option", action="append", default=[], help="development aid: a context option as name=value (repeatable), set on the bench's context before anything runs")
    p.add_argument("--no-mixed-large", action="store_true", help="skip the second mixed-batch measurement at 8 x --mixed-copies (N = 1 only)")
    p.add_argument("--mixed-copies", type=int, default=4, help="copies of the 668-line corpus job in the configs[4] leg")
    p.add_argument("--section", default="all", choices=["all", "zstd", "zstdstream", "xxhash", "lz4frame", "sweep"], help="zstd: run only the Zstd extra section and print its JSON (development aid)")
    p.add_argument("--zstd-exec", type=int, default=-1, help="zstd pipeline execute stage: 2 = chosen per item (default), 1 = wavefront per item through the record executor, 0 = LDS rings")
    p.add_argument("--zstd-kinds", default="fragments,wordmix,corpus", help="data kinds of the zstd section (development aid: tools/make_traffic_json.py measures one kind per run)")
    p.add_argument("--zstd-seq-waves", type=int, default=0, help="zstd pipeline sequence stage: wavefronts per workgroup (1, 2, 4; 0 = library default)")
    p.add_argument("--snappyframed-variant", type=int, default=-1, help="x-snappy-framed reader: 3 = ring or two-pass decoder by a probe (default), 1 = chunks through the ring decoders, 2 = through the two-pass decoder, 0 = a wavefront per stream")
    p.add_argument("--lz4frame-variant", type=int, default=-1, help="LZ4 frame reader: 2 = by a probe (default), 0 = a wavefront per item, 1 = the frames' blocks as one batch through the two-pass block decoder")
    p.add_argument("--hadoop-variant", type=int, default=-1, help="Hadoop block-stream reader: 3 = ring or two-pass decoders by a probe (default), 1 = chunks through the ring decoders, 2 = through the two-pass decoders, 0 = a wavefront per stream")
    p.add_argument("--zstd-compress-variant", type=int, default=-1, help="zstd encoder: 0 match kernel (batch probes) + entropy kernel, 3 match kernel (many matches per window) + entropy kernel, 1 serial probes, 2 one kernel")
    p.add_argument("--zstd-variant", type=int, default=-1, help="zstd decoder: 1 = five-stage pipeline (default), 0 = one-kernel decoder")
    return p.parse_args()


def gen_fragments(torch, dev, n_blocks, block_size, ratio, seed):
    """RandomGenerator.compressibleData for every 100-byte fragment, generated on the device."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    raw = max(1, int(100 * ratio))
    total = n_blocks * block_size
    n_frag = (total + 99) // 100
    frags = torch.randint(0, 256, (n_frag, raw), dtype=torch.uint8, device=dev, generator=g)
    reps = (100 + raw - 1) // raw
    data = frags.repeat(1, reps)[:, :100].reshape(-1)[:total].contiguous()
    return data


_corpus_blocks = {}


def corpus_blocks(block_size):
    """SURVEY 8d, C2 primary / C4: every FULL block_size slice (last partial slice dropped) of the calgary, canterbury, large and
    top-level files of the reference's test corpus in T/benchmark/DataSet.java:28-89 order -- 191 distinct 64 KiB blocks, 86 of 128 KiB
    (tests/golden/corpus_full.bin.xz: the corpus travels as a fixture; /root/reference does not exist on the GPU box)."""
    if block_size not in _corpus_blocks:
        import lzma
        gold = os.path.join(ROOT, "tests", "golden")
        blob = lzma.decompress(open(os.path.join(gold, "corpus_full.bin.xz"), "rb").read())
        out = []
        for e in json.load(open(os.path.join(gold, "corpus_full.json"))):
            if e["file"].startswith("artificial/"):
                continue
            for off in range(0, e["length"] - block_size + 1, block_size):
                out.append(blob[e["offset"] + off:e["offset"] + off + block_size])
        _corpus_blocks[block_size] = np.frombuffer(b"".join(out), dtype=np.uint8)
    return _corpus_blocks[block_size]


def gen_corpus(torch, dev, n_blocks, block_size):
    """Real data: the corpus blocks above tiled cyclically; every copy sits at its own address (distinct HBM traffic)."""
    sample = torch.from_numpy(corpus_blocks(block_size).copy()).to(dev)
    unit = sample.numel()
    total = n_blocks * block_size
    return sample.repeat((total + unit - 1) // unit)[:total].contiguous()


def java_random_generator(ratio, length=1048576):
    """T/snappy/RandomGenerator.java:25-74 restated: java.util.Random(301) (48-bit LCG), 100-byte fragments made of max(1, int(100 *
    ratio)) random bytes repeated.  nextInt(256) is bits 47..40 of the seed; the LCG is jumped ahead in closed form (numpy, wrapping
    uint64 arithmetic is exact modulo 2^48).  Checked against the oracle's generator in tests/test_host_logic.py."""
    raw = max(1, int(100 * ratio))
    n_frag = (length + 99) // 100
    n_calls = n_frag * raw
    A = np.uint64(0x5DEECE66D)
    C = np.uint64(0xB)
    mask = np.uint64((1 << 48) - 1)
    with np.errstate(over="ignore"):
        a = np.multiply.accumulate(np.full(n_calls, A, dtype=np.uint64))             # A^k, k = 1..n
        geo = np.cumsum(np.concatenate([np.ones(1, dtype=np.uint64), a[:-1]]))      # 1 + A + ... + A^(k-1)
        s0 = np.uint64((301 ^ 0x5DEECE66D) & ((1 << 48) - 1))
        seeds = (a * s0 + C * geo) & mask
    rnd = ((seeds >> np.uint64(40)) & np.uint64(0xFF)).astype(np.uint8).reshape(n_frag, raw)
    reps = (100 + raw - 1) // raw
    return np.tile(rnd, (1, reps))[:, :100].reshape(-1)[:length].copy()


def gen_random301(torch, dev, n_blocks, block_size, ratio):
    """SURVEY 8d C2 secondary: block k = generator bytes [(k * block_size) mod 1 MiB, + block_size) -- 16 distinct 64 KiB blocks."""
    data = torch.from_numpy(java_random_generator(ratio)).to(dev)
    total = n_blocks * block_size
    return data.repeat((total + data.numel() - 1) // data.numel())[:total].contiguous()


def gen_data(torch, dev, kind, n_blocks, block_size, ratio, seed):
    if kind == "fragments":
        return gen_fragments(torch, dev, n_blocks, block_size, ratio, seed)
    if kind == "wordmix":
        return gen_wordmix(torch, dev, n_blocks, block_size, seed)
    if kind == "mixed":
        # a batch of two kinds side by side: even blocks corpus-tiled (short sequences), odd blocks fragments (long copies) -- what the
        # decoders' batch-level choice has to get right (auto mode)
        half = (n_blocks + 1) // 2
        a = gen_corpus(torch, dev, half, block_size).view(half, block_size)
        b = gen_fragments(torch, dev, half, block_size, ratio, seed).view(half, block_size)
        return torch.stack([a, b], dim=1).reshape(-1)[:n_blocks * block_size].contiguous()
    return gen_corpus(torch, dev, n_blocks, block_size)


def gen_wordmix(torch, dev, n_blocks, block_size, seed):
    """Text-like data: Zipf-distributed words from a 4096-word vocabulary separated by spaces (short LZ4 sequences)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    vocab = 4096
    wl = torch.randint(2, 11, (vocab,), device=dev, generator=g)
    letters = torch.randint(97, 123, (vocab, 12), dtype=torch.uint8, device=dev, generator=g)
    pos = torch.arange(12, device=dev).unsqueeze(0)
    letters = torch.where(pos < wl.unsqueeze(1), letters, torch.where(pos == wl.unsqueeze(1), torch.full_like(letters, 32), torch.full_like(letters, 255)))
    total = n_blocks * block_size
    out = []
    produced = 0
    while produced < total:
        need = min(int((total - produced) / 6.0) + 4096, 1 << 26)  # masked-select chunks stay far below 2^31 elements
        u = torch.rand((need,), device=dev, generator=g)
        ids = (vocab ** u - 1).long().clamp_(0, vocab - 1)  # log-uniform ~ Zipf(1)
        w = letters[ids].reshape(-1)
        w = w[w != 255]
        out.append(w)
        produced += w.numel()
    return torch.cat(out)[:total].contiguous()


# ---- the legs every rank runs (any N): the rest of BASELINE's metric -- Snappy, Zstd configs[3], the mixed corpus batch configs[4] ----------

def reduce_leg(dist, world, rank, local_bytes, local_seconds, extra=None):
    """Whole-job GiB/s of one leg = the bytes of all ranks / the slowest rank's time (no data-path collective: the only traffic is this gather)."""
    mine = {"rank": rank, "bytes": int(local_bytes), "seconds": round(float(local_seconds), 6), "GiBps": round(local_bytes / max(local_seconds, 1e-12) / 2**30, 2)}
    if extra:
        mine.update(extra)
    per_rank = [mine]
    if world > 1:
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
    total = sum(p["bytes"] for p in per_rank)
    slowest = max(p["seconds"] for p in per_rank)
    return {"GiBps": round(total / max(slowest, 1e-12) / 2**30, 2), "per_rank": per_rank}


def mixed_job(copies):
    """BASELINE configs[4] as a list of work items (pure host arithmetic, the same on every rank): every file of the reference's corpus whole and
    in its 64 KiB (LZ4 / Snappy) / 128 KiB (Zstd) cuts -- the 668 lines of tests/golden/oracle_manifest.tsv, the committed SHA-256 of what the
    Java-equivalent encoders write -- each as one COMPRESS item and one DECOMPRESS item, `copies` times, shuffled with a fixed seed.
    Returns (rows, items, weights): items[k] = (row index, direction 0 = compress / 1 = decompress); weights = srcLen + dstCap per item."""
    import aircompressor_amd as A
    lib = A.load_library()
    gold = os.path.join(ROOT, "tests", "golden")
    rows = []
    for line in open(os.path.join(gold, "oracle_manifest.tsv")):
        f = line.rstrip("\n").split("\t")
        if len(f) == 6:
            rows.append((f[0], int(f[1]), int(f[2]), f[3], int(f[4]), f[5]))
    bound = {"lz4": lib.achip_lz4_max_compressed_length, "snappy": lib.achip_snappy_max_compressed_length, "zstd": lib.achip_zstd_max_compressed_length}
    items, weights = [], []
    for _ in range(copies):
        for r, (_, _, n, codec, clen, _) in enumerate(rows):
            items.append((r, 0))
            weights.append(n + bound[codec](n))
            if n > 0:
                items.append((r, 1))
                weights.append(clen + n)
    order = np.random.default_rng(20260925).permutation(len(items))
    return rows, [items[i] for i in order], np.asarray([weights[i] for i in order], dtype=np.int64)


MIXED_OPS = {"lz4": (1, 0), "snappy": (3, 2), "zstd": (5, 4)}  # codec -> (compress op, decompress op)


def corpus_files():
    import lzma
    gold = os.path.join(ROOT, "tests", "golden")
    blob = lzma.decompress(open(os.path.join(gold, "corpus_full.bin.xz"), "rb").read())
    return {e["file"]: blob[e["offset"]:e["offset"] + e["length"]] for e in json.load(open(os.path.join(gold, "corpus_full.json")))}


def mixed_leg(torch, A, codec, dev, args, rank, world, dist):
    """BASELINE configs[4]: the shuffled 3-codec x 2-direction corpus batch cut over the ranks by achip_partition_blocks (weights = bytes in +
    capacity out), every rank's slice ONE achip_mixed_batch call (bucketed by codec inside the library), device-resident, timed; then every
    item of every rank checked: a compress item's stream must hash to the manifest's line (= what the Java-equivalent encoder writes), a
    decompress item must restore the plaintext.  mixed_ok only if every item on every rank is byte-exact."""
    import hashlib
    from aircompressor_amd.sharding import shard_for_rank
    lib = codec.lib
    if os.environ.get("ACHIP_MIXED_CONCURRENT") in ("0", "1"):  # (measurement aid: the buckets one after the other instead of side by side)
        codec.native.set_option("mixed.concurrent", int(os.environ["ACHIP_MIXED_CONCURRENT"]))
    rows, items, weights = mixed_job(args.mixed_copies)
    lo, hi = shard_for_rank(weights, world, rank)
    mine = items[lo:hi]
    files = corpus_files()
    bound = {"lz4": lib.achip_lz4_max_compressed_length, "snappy": lib.achip_snappy_max_compressed_length, "zstd": lib.achip_zstd_max_compressed_length}
    plain_of = lambda r: files[rows[r][0]][rows[r][1]:rows[r][1] + rows[r][2]]  # noqa: E731
    i64 = dict(dtype=torch.int64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)

    def run(ops, blobs, caps, iters):
        """one achip_mixed_batch call over host blobs (uploaded first); returns (outputs, statuses, seconds per call)"""
        n = len(blobs)
        lens = np.asarray([len(b) for b in blobs], dtype=np.int64)
        pad = (lens + 15) // 16 * 16
        s_off = np.cumsum(pad) - pad
        buf = np.zeros(int(pad.sum()) + 16, dtype=np.uint8)
        for b, o_ in zip(blobs, s_off):
            buf[o_:o_ + len(b)] = np.frombuffer(b, dtype=np.uint8)
        caps = np.asarray(caps, dtype=np.int64)
        cpad = (caps + 15) // 16 * 16
        d_off = np.cumsum(cpad) - cpad
        d_src = torch.from_numpy(buf).to(dev)
        d_dst = torch.zeros(int(cpad.sum()) + 64, dtype=torch.uint8, device=dev)
        a_so, a_sl = torch.from_numpy(s_off).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev)
        a_do, a_dc = torch.from_numpy(d_off).to(dev), torch.from_numpy(caps.astype(np.int32)).to(dev)
        o_len, st, eo = torch.zeros(n, **i32), torch.zeros(n, **i32), torch.zeros(n, **i64)
        torch.cuda.synchronize()
        launch = lambda: codec.launch_mixed(ops, d_src, a_so, a_sl, d_dst, a_do, a_dc, o_len, st, eo, n)  # noqa: E731
        launch()
        codec.synchronize()
        seconds = 0.0
        if iters:
            if world > 1:
                dist.barrier()
            t0 = time.perf_counter()
            for _ in range(iters):
                launch()
            codec.synchronize()
            seconds = (time.perf_counter() - t0) / iters
        out = d_dst.cpu().numpy()
        o_len = o_len.cpu().numpy()
        return [out[o_:o_ + max(int(k), 0)].tobytes() for o_, k in zip(d_off, o_len)], st.cpu().numpy(), seconds

    # untimed setup: the compressed inputs of this rank's decompress items come from the product's own encoders (the oracle is never used to make
    # inputs), each checked against the manifest's SHA-256 before it is used
    need = sorted({r for r, d in mine if d == 1})
    streams = {}
    if need:
        outs, st, _ = run([MIXED_OPS[rows[r][3]][0] for r in need], [plain_of(r) for r in need], [bound[rows[r][3]](rows[r][2]) for r in need], 0)
        for r, c, s_ in zip(need, outs, st):
            assert s_ == 0 and hashlib.sha256(c).hexdigest() == rows[r][5], "setup: the GPU encoder's stream differs from the manifest (%s)" % (rows[r],)
            streams[r] = c
    ops = [MIXED_OPS[rows[r][3]][d] for r, d in mine]
    blobs = [plain_of(r) if d == 0 else streams[r] for r, d in mine]
    caps = [bound[rows[r][3]](rows[r][2]) if d == 0 else max(rows[r][2], 1) for r, d in mine]
    outs, st, seconds = run(ops, blobs, caps, 3) if mine else ([], np.zeros(0, dtype=np.int32), 0.0)
    bad = 0
    for (r, d), out, s_ in zip(mine, outs, st):
        good = s_ == 0 and ((hashlib.sha256(out).hexdigest() == rows[r][5] and len(out) == rows[r][4]) if d == 0 else out == plain_of(r))
        bad += 0 if good else 1
    plain_bytes = sum(rows[r][2] for r, _ in mine)  # the decompressed-side bytes of both directions (the metric's numerator convention)
    leg = reduce_leg(dist, world, rank, plain_bytes, seconds, {"items": len(mine), "slice": [lo, hi], "mismatches": bad, "codec_ops": len(set(ops))})
    leg.update({"mixed_ok": all(p["mismatches"] == 0 for p in leg["per_rank"]) and sum(p["items"] for p in leg["per_rank"]) == len(items),
                "items": len(items), "manifest_lines": len(rows), "copies": args.mixed_copies,
                "what": "BASELINE configs[4]: every corpus file whole + every 64 / 128 KiB cut x LZ4 / Snappy / Zstd x compress / decompress, shuffled, cut over the "
                        "ranks by achip_partition_blocks, one achip_mixed_batch call per rank; compress items checked against tests/golden/oracle_manifest.tsv's "
                        "SHA-256 (the Java-equivalent encoders' streams), decompress items against the plaintext"})
    return leg


def zstd_libzstd_batch(torch, dev, args, data_kind, pool_n, reps, seed):
    """65536 (pool_n x reps) Zstd level-3 frames of 128 KiB made on the host by libzstd (pyarrow): the pool's frames packed at 16-byte aligned
    starts and tiled, every copy at its own address."""
    import pyarrow as pa
    fs = 131072
    zc = pa.Codec("zstd", compression_level=3)
    plain = gen_data(torch, dev, data_kind, pool_n, fs, args.ratio, seed)
    host = plain.cpu().numpy()
    frames = [zc.compress(host[i * fs:(i + 1) * fs].tobytes(), asbytes=True) for i in range(pool_n)]
    lens = np.array([len(f) for f in frames], dtype=np.int64)
    pad = (lens + 15) // 16 * 16
    offs = np.cumsum(pad) - pad
    pack = np.zeros(int(pad.sum()), dtype=np.uint8)
    for f, o_ in zip(frames, offs):
        pack[o_:o_ + len(f)] = np.frombuffer(f, dtype=np.uint8)
    n = pool_n * reps
    i64 = dict(dtype=torch.int64, device=dev)
    d_pack = torch.from_numpy(pack).to(dev).repeat(reps)
    rep_idx = torch.arange(reps, **i64).repeat_interleave(pool_n)
    src_off = torch.from_numpy(offs).to(dev).repeat(reps) + rep_idx * int(pad.sum())
    src_len = torch.from_numpy(lens.astype(np.int32)).to(dev).repeat(reps)
    return {"plain": plain, "host": host, "pack": pack, "offs": offs, "lens": lens, "d_pack": d_pack, "src_off": src_off, "src_len": src_len, "n": n, "fs": fs,
            "cbytes": int(lens.sum()) * reps, "encoder": "libzstd level 3 via pyarrow %s" % pa.__version__}


def rank_legs(torch, A, codec, dev, args, rank, world, dist, n_local):
    """What `--gpus N` reports besides the LZ4 headline, on EVERY rank: Snappy decompress on the headline's batch shape, Zstd level-3 decompress of
    65536 x 128 KiB frames per GPU (BASELINE configs[3]; libzstd's frames and the GPU encoder's = the Java encoder's, corpus-tiled and fragments) and
    the mixed corpus batch (configs[4]).  Every leg: warm launch + byte-exact check, barrier, timed launches, the bytes of all ranks over the slowest
    rank's time.  Each unit is self-contained (M/zstd/ZstdFrameDecompressor.java:151, M/zstd/ZstdFrameCompressor.java:162): ranks own disjoint frames."""
    out = {}
    bs = args.block_size
    i64 = dict(dtype=torch.int64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)

    def timed(launch, iters):
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        for _ in range(iters):
            launch()
        codec.synchronize()
        return (time.perf_counter() - t0) / iters

    # -- Snappy decompress, fragments, the headline's batch shape (compressed on the GPU by the product's encoder) --
    n = n_local
    plain = gen_data(torch, dev, "fragments", min(n, 4096), bs, args.ratio, 1301 + rank)
    pool_n = plain.numel() // bs
    max_c = codec.lib.achip_snappy_max_compressed_length(bs)
    cstride = (max_c + 15) // 16 * 16
    comp = torch.empty(pool_n * cstride + 64, dtype=torch.uint8, device=dev)
    clen, st, eo = torch.zeros(pool_n, **i32), torch.zeros(pool_n, **i32), torch.zeros(pool_n, **i64)
    # (the library launches on the context's stream: every argument stays alive in a named tensor and torch's stream is drained before each first launch)
    p_off, p_len = torch.arange(pool_n, **i64) * bs, torch.full((pool_n,), bs, **i32)
    c_off, c_cap = torch.arange(pool_n, **i64) * cstride, torch.full((pool_n,), max_c, **i32)
    torch.cuda.synchronize()
    codec.launch(A.OP_SNAPPY_COMPRESS, plain, p_off, p_len, comp, c_off, c_cap, clen, st, eo, pool_n)
    codec.synchronize()
    assert int((st != 0).sum()) == 0, "snappy leg: encode failed"
    reps = n // pool_n
    n = reps * pool_n
    src = comp[:pool_n * cstride].repeat(reps)
    src_off = (torch.arange(pool_n, **i64) * cstride).repeat(reps) + torch.arange(reps, **i64).repeat_interleave(pool_n) * (pool_n * cstride)
    src_len = clen.repeat(reps)
    dst = torch.empty(n * bs + 64, dtype=torch.uint8, device=dev)
    dst_off, dst_cap = torch.arange(n, **i64) * bs, torch.full((n,), bs, **i32)
    olen, st, eo = torch.zeros(n, **i32), torch.zeros(n, **i32), torch.zeros(n, **i64)
    launch = lambda: codec.launch(A.OP_SNAPPY_DECOMPRESS, src, src_off, src_len, dst, dst_off, dst_cap, olen, st, eo, n)  # noqa: E731
    torch.cuda.synchronize()
    launch()
    codec.synchronize()
    assert int((st != 0).sum()) == 0 and bool((dst[:n * bs].view(reps, pool_n * bs) == plain.unsqueeze(0)).all()), "snappy leg: plaintext mismatch"
    t = timed(launch, 5)
    out["snappy"] = reduce_leg(dist, world, rank, n * bs, t, {"blocks": n, "ratio": round(pool_n * bs / int(clen.to(torch.int64).sum()), 3)})
    del src, dst, comp, plain
    torch.cuda.empty_cache()

    # -- Zstd configs[3] --
    try:
        import pyarrow  # noqa: F401
        have_pa = True
    except ImportError:
        have_pa = False
    for kind in ("fragments", "corpus"):
        suffix = "" if kind == "fragments" else "_corpus"
        fs = 131072
        if have_pa:
            b = zstd_libzstd_batch(torch, dev, args, kind, 512, args.zstd_frames // 512, 4242 + rank)
            n = b["n"]
            dst = torch.empty(n * fs + 64, dtype=torch.uint8, device=dev)
            dst_off, dst_cap = torch.arange(n, **i64) * fs, torch.full((n,), fs, **i32)
            olen, st, eo = torch.zeros(n, **i32), torch.zeros(n, **i32), torch.zeros(n, **i64)
            launch = lambda: codec.launch(A.OP_ZSTD_DECOMPRESS, b["d_pack"], b["src_off"], b["src_len"], dst, dst_off, dst_cap, olen, st, eo, n)  # noqa: E731
            torch.cuda.synchronize()
            launch()
            codec.synchronize()
            assert int((st != 0).sum()) == 0 and bool((dst[:n * fs].view(-1, 512 * fs) == b["plain"].unsqueeze(0)).all()), "zstd leg: plaintext mismatch"
            t = timed(launch, 3)
            out["zstd" + suffix] = reduce_leg(dist, world, rank, n * fs, t, {"frames": n, "ratio": round(n * fs / b["cbytes"], 3)})
            out["zstd" + suffix]["encoder"] = b["encoder"]
            plain = b["plain"]
            del dst, b
        else:
            plain = gen_data(torch, dev, kind, 512, fs, args.ratio, 4242 + rank)
        # frames of the GPU encoder (byte-identical to the Java encoder's, tests/test_gpu_corpus.py): encoded here, decoded, verified, timed
        nz = 512 * max(1, args.zstd_frames // 1024)
        zrep = nz // 512
        max_c = codec.lib.achip_zstd_max_compressed_length(fs)
        cstride = (max_c + 15) // 16 * 16
        zplain = plain.repeat(zrep)
        z_off, z_len = torch.arange(nz, **i64) * fs, torch.full((nz,), fs, **i32)
        z_dst = torch.empty(nz * cstride + 64, dtype=torch.uint8, device=dev)
        zc_off, zc_cap = torch.arange(nz, **i64) * cstride, torch.full((nz,), max_c, **i32)
        zc_len, st, eo = torch.zeros(nz, **i32), torch.zeros(nz, **i32), torch.zeros(nz, **i64)
        enc = lambda: codec.launch(A.OP_ZSTD_COMPRESS, zplain, z_off, z_len, z_dst, zc_off, zc_cap, zc_len, st, eo, nz)  # noqa: E731
        torch.cuda.synchronize()
        enc()
        codec.synchronize()
        assert int((st != 0).sum()) == 0, "zstd leg: encode failed"
        te = timed(enc, 1)
        back = torch.empty(nz * fs + 64, dtype=torch.uint8, device=dev)
        b_len = torch.zeros(nz, **i32)
        dec = lambda: codec.launch(A.OP_ZSTD_DECOMPRESS, z_dst, zc_off, zc_len, back, z_off, z_len, b_len, st, eo, nz)  # noqa: E731
        torch.cuda.synchronize()
        dec()
        codec.synchronize()
        assert int((st != 0).sum()) == 0 and bool((back[:nz * fs] == zplain).all()), "zstd leg: GPU encode -> GPU decode round trip failed"
        td = timed(dec, 3)
        zbytes = int(zc_len.to(torch.int64).sum())
        out["zstd_java_frames" + suffix] = reduce_leg(dist, world, rank, nz * fs, td, {"frames": nz, "ratio": round(nz * fs / zbytes, 3)})
        out["zstd_compress" + suffix] = reduce_leg(dist, world, rank, nz * fs, te, {"frames": nz})
        del z_dst, back, zplain, plain
        torch.cuda.empty_cache()

    out["mixed"] = mixed_leg(torch, A, codec, dev, args, rank, world, dist)
    return out


def relaunch_with_ranks(n):
    """`python bench.py --gpus N` without a launcher: start N ranks of this very command under torch.distributed.run (one process per GPU,
    rank r on cuda:r) and hand its exit code on.  The driver's own `python -m torch.distributed.run ... bench.py --gpus N` form sets WORLD_SIZE
    and never comes here."""
    import socket
    import subprocess
    with socket.socket() as sock:  # a free port for the rendezvous
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.call(cmd, env=env)


def stub_main(args, rank, world, dist):
    """ACHIP_BENCH_STUB_DEVICE=1: the control plane of an N-rank run WITHOUT a device -- launch, rendezvous, shard_for_rank, barrier, timed steps,
    MAX over ranks, per-rank gather, ONE line from rank 0 -- with a host memcpy standing in for the kernel.  tests/test_bench_launch.py runs it on
    the CPU; the line says "stub" and is never a result."""
    from aircompressor_amd.sharding import shard_for_rank
    bs = args.block_size
    n_global = args.blocks * world
    lo, hi = shard_for_rank(np.full(n_global, bs, dtype=np.int64), world, rank)
    n_local = hi - lo
    a = np.zeros(min(n_local, 256) * bs, dtype=np.uint8)
    b = np.empty_like(a)
    for _ in range(args.warmup):
        np.copyto(b, a)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        np.copyto(b, a)
    elapsed_local = time.perf_counter() - t0
    elapsed = elapsed_local
    per_rank = [elapsed_local]
    if world > 1:
        import torch
        dist.barrier()
        t = torch.tensor([elapsed_local], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        per_rank = [None] * world
        dist.all_gather_object(per_rank, elapsed_local)
    # the legs' control plane (reduce_leg's gather, the mixed job's partition over the ranks) with the same memcpy standing in for every kernel
    legs = {}
    if args.full and not args.no_legs:
        for name in ("snappy", "zstd", "zstd_corpus", "zstd_java_frames", "zstd_java_frames_corpus"):
            t0 = time.perf_counter()
            np.copyto(b, a)
            legs[name] = reduce_leg(dist, world, rank, a.nbytes, time.perf_counter() - t0)
        rows, items, weights = mixed_job(args.mixed_copies)
        mlo, mhi = shard_for_rank(weights, world, rank)
        t0 = time.perf_counter()
        np.copyto(b, a)
        legs["mixed"] = reduce_leg(dist, world, rank, sum(rows[r][2] for r, _ in items[mlo:mhi]), time.perf_counter() - t0, {"items": mhi - mlo, "slice": [mlo, mhi], "mismatches": 0})
        legs["mixed"].update({"mixed_ok": sum(p["items"] for p in legs["mixed"]["per_rank"]) == len(items), "items": len(items), "manifest_lines": len(rows)})
    if rank == 0:
        extra_keys = {}
        if legs:
            extra_keys = {"legs": legs, "value_mixed": legs["mixed"]["GiBps"], "mixed_ok": legs["mixed"]["mixed_ok"], "value_snappy": legs["snappy"]["GiBps"],
                          "value_zstd": legs["zstd"]["GiBps"], "value_zstd_corpus": legs["zstd_corpus"]["GiBps"]}
        print(json.dumps({**extra_keys, "metric": "GiB/s decompressed throughput (Zstd+LZ4) at 1/2/4/8 GPUs; % of HBM3E roofline", "value": 0.0, "unit": "GiB/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / max(args.steps, 1) * 1e3, 4), "higher_is_better": True,
                          "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "stub (ACHIP_BENCH_STUB_DEVICE=1: no device, control plane only -- not a result)",
                          "stub": True, "config": {"workload": "stub", "blocks_per_gpu": n_local, "shard": [lo, hi], "per_rank_seconds": per_rank}}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main():
    args = parse_args()
    if args.gpus < 1:
        print("bench.py: --gpus must be >= 1", file=sys.stderr)
        return 2
    if args.steps < 1:
        print("bench.py: --steps must be >= 1", file=sys.stderr)
        return 2
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return relaunch_with_ranks(args.gpus)  # --gpus N means N ranks: started here when no launcher did

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        # the line's n_gpus must be what was asked for: a launcher that started another number of ranks is an error, not a silent N
        if rank == 0:
            print("bench.py: --gpus %d but WORLD_SIZE=%d: refusing to report one under the other's name" % (args.gpus, world), file=sys.stderr)
        return 2
    dist = None
    if world > 1:
        # control plane only (barrier + MAX of the elapsed time, on CPU tensors): gloo -- the data path has no collective and needs no
        # RCCL (north_star: "per-GPU batch split, no RCCL needed")
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo")
    if os.environ.get("ACHIP_BENCH_STUB_DEVICE") == "1":
        return stub_main(args, rank, world, dist)
    import torch
    import aircompressor_amd as A

    share = os.environ.get("ACHIP_BENCH_SHARE_DEVICE") == "1"
    if share:
        # PATH CHECK ONLY (never a scaling number): every rank uses device 0, so that the N > 1 path -- rendezvous, shard_for_rank, barrier,
        # max-over-ranks, one JSON line from rank 0, verification on every rank -- can be executed end to end on a box with one GPU
        local_rank = 0
    n_dev = torch.cuda.device_count()
    if (not share and world > n_dev) or local_rank >= n_dev:  # (every rank sees the same counts: all of them leave, nobody waits in a collective)
        if rank == 0:
            print("bench.py: %d ranks but the node has %d device(s) (ACHIP_BENCH_SHARE_DEVICE=1 runs every rank on cuda:0 as a path check)" % (world, n_dev), file=sys.stderr)
        if world > 1:
            dist.destroy_process_group()
        return 3
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        # N ranks must sit on N distinct devices
        props = torch.cuda.get_device_properties(local_rank)
        ident = "%s/%s" % (getattr(props, "uuid", ""), getattr(props, "pci_bus_id", local_rank))
        idents = [None] * world
        dist.all_gather_object(idents, (local_rank, ident))
        if not share and len(set(idents)) != world:
            if rank == 0:
                print("bench.py: %d ranks on %d distinct devices %r" % (world, len(set(idents)), idents), file=sys.stderr)
            return 3

    bs = args.block_size
    n_local_target = args.blocks
    n_global = n_local_target * world
    # contiguous, byte-balanced shard of the global block index (no collective on the data path)
    from aircompressor_amd.sharding import shard_for_rank
    lo, hi = shard_for_rank(np.full(n_global, bs, dtype=np.int64), world, rank)
    n_local = hi - lo

    codec = A.HipBatchCodec(local_rank)
    for kv in args.option:
        k_, v_ = kv.split("=")
        codec.native.set_option(k_, int(v_))
    lib = codec.lib
    if args.group:
        codec.native.set_option("lz4.decompress.group", args.group)
        codec.native.set_option("snappy.decompress.group", args.group)
    if args.variant >= 0:
        codec.native.set_option("%s.decompress.variant" % ("lz4" if args.workload.startswith("lz4") else "snappy"), args.variant)
    if args.parse >= 0:
        codec.native.set_option("lz4.decompress.parse", args.parse)
        codec.native.set_option("snappy.decompress.parse", args.parse)
    if args.ring_class >= 0:
        codec.native.set_option("decompress.ring_class", args.ring_class)
    if args.compress_variant >= 0:
        # (one flag for both codecs' encoders: each takes the values it knows -- LZ4 0 / 1 / 4, Snappy 0 .. 4; 4 is the default of both)
        if args.compress_variant in (0, 1, 4):
            codec.native.set_option("lz4.compress.variant", args.compress_variant)
        if args.compress_variant <= 4:
            codec.native.set_option("snappy.compress.variant", args.compress_variant)
    if args.ring_pad >= 0:
        codec.native.set_option("decompress.ring_pad", args.ring_pad)
    codec.native.set_option("max_src_len_hint", bs)
    if args.hadoop_variant >= 0:
        codec.native.set_option("hadoop.decompress.variant", args.hadoop_variant)
    if args.snappyframed_variant >= 0:
        codec.native.set_option("snappyframed.decompress.variant", args.snappyframed_variant)
    if args.lz4frame_variant >= 0:
        codec.native.set_option("lz4frame.decompress.variant", args.lz4frame_variant)
    if args.section == "lz4frame":
        print(json.dumps(lz4frame_extra(torch, A, codec, torch.device("cuda", local_rank), args)), flush=True)
        return
    if args.section == "sweep":
        print(json.dumps(sweep_random301(torch, A, codec, torch.device("cuda", local_rank), args)), flush=True)
        return
    if args.section == "xxhash":
        print(json.dumps(xxhash_extra(torch, A, codec, torch.device("cuda", local_rank), args)), flush=True)
        return
    if args.section == "zstd":
        print(json.dumps(zstd_extra(torch, A, codec, torch.device("cuda", local_rank), args)), flush=True)
        return
    if args.section == "zstdstream":
        print(json.dumps(zstd_stream_extra(torch, A, codec, torch.device("cuda", local_rank), args)), flush=True)
        return

    wl = args.workload
    name = "lz4" if wl.startswith("lz4") else "snappy"
    compress_op = A.OP_LZ4_COMPRESS if name == "lz4" else A.OP_SNAPPY_COMPRESS
    decompress_op = A.OP_LZ4_DECOMPRESS if name == "lz4" else A.OP_SNAPPY_DECOMPRESS
    max_c = getattr(lib, "achip_%s_max_compressed_length" % name)(bs)

    # ---- untimed setup: pool of distinct blocks, compressed by the product's GPU encoder ----
    pool_n = min(args.pool, n_local)
    while n_local % pool_n:
        pool_n -= 1
    reps = n_local // pool_n
    seed = 301 + 7919 * (lo // max(pool_n, 1))
    pool_plain = gen_data(torch, dev, args.data, pool_n, bs, args.ratio, seed)
    cstride = (max_c + 15) // 16 * 16
    i64 = dict(dtype=torch.int64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    pool_src_off = torch.arange(pool_n, **i64) * bs
    pool_src_len = torch.full((pool_n,), bs, **i32)
    pool_dst_off = torch.arange(pool_n, **i64) * cstride
    pool_dst_cap = torch.full((pool_n,), max_c, **i32)
    pool_comp_wide = torch.zeros(pool_n * cstride, dtype=torch.uint8, device=dev)
    pool_clen = torch.zeros(pool_n, **i32)
    pool_st = torch.zeros(pool_n, **i32)
    pool_eo = torch.zeros(pool_n, **i64)
    torch.cuda.synchronize()
    codec.launch(compress_op, pool_plain, pool_src_off, pool_src_len, pool_comp_wide, pool_dst_off, pool_dst_cap, pool_clen, pool_st, pool_eo, pool_n)
    codec.synchronize()
    assert int((pool_st != 0).sum()) == 0, "GPU compressor reported errors while preparing the workload"
    # pack the compressed pool tightly (16-byte aligned starts) and tile it to the batch, each copy at its own address
    clen = pool_clen.to(torch.int64)
    cpad = (clen + 15) // 16 * 16
    pool_pack_off = torch.cumsum(cpad, 0) - cpad
    pool_pack_bytes = int(cpad.sum())
    idx_block = torch.repeat_interleave(torch.arange(pool_n, device=dev), cpad)
    within = torch.arange(pool_pack_bytes, device=dev) - pool_pack_off[idx_block]
    pool_pack = pool_comp_wide[pool_dst_off[idx_block] + within]
    del idx_block, within, pool_comp_wide
    comp_bytes_pool = int(clen.sum())
    plain_bytes_local = n_local * bs
    comp_bytes_local = comp_bytes_pool * reps

    rep_idx = torch.arange(reps, **i64).repeat_interleave(pool_n)
    if wl.endswith("decompress"):
        src = pool_pack.repeat(reps)
        src_off = pool_pack_off.repeat(reps) + rep_idx * pool_pack_bytes
        src_len = pool_clen.repeat(reps)
        dst_stride = bs + max(0, args.dst_pad)
        dst = torch.empty(n_local * dst_stride + 64, dtype=torch.uint8, device=dev)
        dst_off = torch.arange(n_local, **i64) * dst_stride
        dst_cap = torch.full((n_local,), bs, **i32)
        op = decompress_op
    else:
        src = pool_plain.repeat(reps)
        src_off = torch.arange(n_local, **i64) * bs
        src_len = torch.full((n_local,), bs, **i32)
        dst = torch.empty(n_local * cstride + 64, dtype=torch.uint8, device=dev)
        dst_off = torch.arange(n_local, **i64) * cstride
        dst_cap = torch.full((n_local,), max_c, **i32)
        op = compress_op
    out_len = torch.zeros(n_local, **i32)
    status = torch.zeros(n_local, **i32)
    err_off = torch.zeros(n_local, **i64)
    torch.cuda.synchronize()

    def step():
        codec.launch(op, src, src_off, src_len, dst, dst_off, dst_cap, out_len, status, err_off, n_local)

    def barrier():
        torch.cuda.synchronize()
        codec.synchronize()
        if world > 1:
            dist.barrier()

    for _ in range(args.warmup):
        step()
    barrier()
    ev = [(codec.event(), codec.event()) for _ in range(args.steps)]
    t0 = time.perf_counter()
    for k in range(args.steps):
        codec.record(ev[k][0])
        step()
        codec.record(ev[k][1])
    codec.synchronize()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    elapsed_local = elapsed
    if world > 1:
        dist.barrier()
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    kernel_ms = [codec.elapsed_ms(a, b) for a, b in ev]

    # ---- untimed verification: every block ok and bit-exact ----
    assert int((status != 0).sum()) == 0, "a block failed"
    if args.no_verify:
        print("DEBUG RUN: output not verified", file=sys.stderr)
    elif wl.endswith("decompress"):
        assert int((out_len != bs).sum()) == 0
        if args.dst_pad > 0:
            ok = bool((dst[:n_local * dst_stride].view(reps, pool_n, dst_stride)[:, :, :bs] == pool_plain.view(1, pool_n, bs)).all())
        else:
            ok = bool((dst[:n_local * bs].view(reps, pool_n * bs) == pool_plain.unsqueeze(0)).all())
        assert ok, "decompressed output differs from the plaintext"
    else:
        assert bool((out_len == pool_clen.repeat(reps)).all())
    if args.dump_outputs and rank == 0:
        dump_outputs(torch, args.dump_outputs, dst, dst_off, int(dst_cap[0]), out_len, status, err_off)

    twopass_fallback = codec.native.get_stat("decompress.twopass_fallback_blocks") if wl.endswith("decompress") else -1
    mixed_groups = codec.native.get_stat("lz4.decompress.mixed_groups") if wl.endswith("decompress") else -1
    choice = codec.native.get_stat("decompress.choice") if wl.endswith("decompress") else -1
    if choice < 0 and wl.endswith("decompress"):  # a forced decoder (no probe ran): 7 = the two passes, 1 = the rings
        choice = 3 if args.variant == 7 else 0
    decoder = "n/a" if not wl.endswith("decompress") else DECODER_NAMES.get(choice, "rings")
    ms_per_step = elapsed / args.steps * 1e3
    total_plain = plain_bytes_local * world  # weak scaling: every rank owns n_local blocks
    value = total_plain * args.steps / elapsed / 2**30
    kavg = float(np.mean(kernel_ms)) * 1e-3
    alg_bytes = plain_bytes_local + comp_bytes_local + n_local * 20  # U_i + C_i + 20 B metadata per block
    achieved = alg_bytes / kavg / 1e9
    result = {
        "metric": "GiB/s decompressed throughput (Zstd+LZ4) at 1/2/4/8 GPUs; % of HBM3E roofline",
        "value": round(value, 2),
        "unit": "GiB/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic",
        "config": {
            "workload": "%s, %d x %d B %s blocks per GPU (BASELINE configs[1]), %s data%s, LZ4 ratio %.3f, batched C-ABI launch, HBM-resident" % (
                wl, n_local, bs, name.upper(), args.data, (" ratio=%.2f" % args.ratio) if args.data == "fragments" else "", plain_bytes_local / comp_bytes_local),
            "blocks_per_gpu": n_local, "block_bytes": bs, "distinct_blocks": pool_n, "compression_ratio": round(plain_bytes_local / comp_bytes_local, 4),
            "parallelism": "block-sharded x%d, no collective" % world + (" -- ALL RANKS ON ONE DEVICE (ACHIP_BENCH_SHARE_DEVICE=1): a path check, not a scaling number" if world > 1 and os.environ.get("ACHIP_BENCH_SHARE_DEVICE") == "1" else ""),
            "decoder": decoder + (" (chosen on the device: %d of %d 16-block groups mixed)" % (mixed_groups, (n_local + 15) // 16) if mixed_groups >= 0 else ""),
            "twopass_fallback_blocks": twopass_fallback,
            **({"dst_pad": args.dst_pad, "LAYOUT_EXPERIMENT": "outputs %d bytes apart, not one contiguous buffer: not the headline" % (bs + args.dst_pad)} if args.dst_pad > 0 and wl.endswith("decompress") else {}),
        },
        "roofline": {
            "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
            "traffic": None, "kernel": kernel_symbol(wl, decoder), "kernel_ms_avg": round(kavg * 1e3, 4), "algorithmic_bytes_per_launch": alg_bytes,
            "frac_of_measured_copy_ceiling_6290": round(achieved / 6290.0, 4),
        },
    }
    # per rank: its own GiB/s and its kernel's fraction of the roofline (`value` is the whole job: all ranks' bytes over the slowest rank's time)
    mine = {"rank": rank, "device": local_rank, "GiBps": round(plain_bytes_local * args.steps / elapsed_local / 2**30, 2), "kernel_ms_avg": round(kavg * 1e3, 4),
            "roofline_frac": round(achieved / HBM_PEAK_GBS, 4)}
    per_rank = [mine]
    if world > 1:
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
    result["per_rank"] = per_rank
    # roofline.traffic: HBM bytes per launch from the PMC counters (FETCH_SIZE x 2 + WRITE_SIZE, separate rocprofv3 passes: tools/make_traffic_json.py
    # writes profiles/traffic.json with the hash of the kernel sources it measured).  Counters cannot be collected inside this process, so
    # the figure is the committed measurement -- and only if it was taken on THESE kernel sources and this batch size; otherwise null.
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    if os.path.exists(tpath):
        try:
            t = json.load(open(tpath)).get(wl)
            if t and t.get("blocks") == n_local and t.get("kernel_sources_sha256") == kernel_sources_hash():
                result["roofline"]["traffic"] = t["hbm_bytes_per_launch"]
                result["roofline"]["traffic_source"] = t.get("source")
            elif t:
                result["roofline"]["traffic_source"] = "profiles/traffic.json is for other kernel sources or another batch size: not reported"
        except Exception:
            pass

    # release the headline's buffers first: the legs and the extras allocate batches of the same size
    del src, dst
    torch.cuda.empty_cache()
    if args.full and not args.no_legs:
        codec.native.set_option("max_src_len_hint", 0)  # the legs' units are not the headline's 64 KiB blocks (whole files, 128 KiB frames)
        # the rest of the metric on EVERY rank: at N > 1 all legs (the extras below are N = 1 only); at N = 1 the extras carry Snappy / Zstd and
        # only the mixed corpus batch (configs[4]) is added here
        legs = rank_legs(torch, A, codec, dev, args, rank, world, dist, n_local) if world > 1 else {"mixed": mixed_leg(torch, A, codec, dev, args, rank, world, dist)}
        result["legs"] = legs
        result["value_mixed"] = legs["mixed"]["GiBps"]
        result["mixed_ok"] = legs["mixed"]["mixed_ok"]
        if world == 1 and not args.no_mixed_large:
            # the same job eight times over in one call (round 6): a mixed batch is as long as its longest serial chain -- a 4 MB file as ONE Zstd frame or
            # ONE LZ4 block is 0.4-0.7 s of a single wavefront --, so its rate is a matter of how much work lies beside that chain; both are in the line
            copies = args.mixed_copies
            try:
                args.mixed_copies = 8 * copies
                big = mixed_leg(torch, A, codec, dev, args, rank, world, dist)
                result["value_mixed_8x_batch"] = big["GiBps"]
                result["mixed_8x_batch"] = {"copies": big["copies"], "items": big["items"], "mixed_ok": big["mixed_ok"], "seconds": big["per_rank"][0]["seconds"],
                                            "what": "the configs[4] job with 8 x --mixed-copies: same longest chain, eight times the items beside it"}
            except Exception as e:  # (a secondary entry must not take the run's line with it)
                result["mixed_8x_batch"] = {"error": repr(e)}
            finally:
                args.mixed_copies = copies
        if world > 1:
            result["value_snappy"] = legs["snappy"]["GiBps"]                        # Snappy decompress, the headline's batch shape
            if "zstd" in legs:
                result["value_zstd"] = legs["zstd"]["GiBps"]                        # BASELINE configs[3]: libzstd level-3 frames of 128 KiB, fragments
                result["value_zstd_corpus"] = legs["zstd_corpus"]["GiBps"]          # ... corpus-tiled
            result["value_zstd_java_frames"] = legs["zstd_java_frames"]["GiBps"]    # the same plaintext in the GPU encoder's (= the Java encoder's) frames
            result["value_zstd_java_frames_corpus"] = legs["zstd_java_frames_corpus"]["GiBps"]
    codec.native.set_option("max_src_len_hint", bs)
    if rank == 0 and world == 1 and args.full and not args.no_extra:
        ex = extras(torch, A, codec, dev, args)
        ex.update(xxhash_extra(torch, A, codec, dev, args))
        ex.update(lz4frame_extra(torch, A, codec, dev, args))
        try:
            ex.update(zstd_extra(torch, A, codec, dev, args))
            try:
                torch.cuda.empty_cache()
                ex.update(zstd_stream_extra_isolated())
            except Exception as e:  # (a secondary entry must not take the run's line with it; the parity tests are the check)
                ex["zstdstream_error"] = repr(e)
        except ImportError:
            pass
        result["extra"] = ex
        # the same `roofline` object for the real-data entries: algorithmic bytes over the launch's time, and the HBM bytes the
        # launch's kernels moved by the counters -- profiles/traffic.json, only where it was measured on these kernel sources and this batch size
        try:
            tj = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
        except Exception:
            tj = {}
        for key, units, unit_bytes in (("lz4_corpus", "blocks", args.block_size), ("snappy_corpus", "blocks", args.block_size), ("zstd_corpus", "frames", 131072)):
            e = ex.get(key)
            if not e:
                continue
            n_units = e[units]
            alg = int(n_units * unit_bytes * (1.0 + 1.0 / e["ratio"])) + 20 * n_units
            seconds = n_units * unit_bytes / (e["decompress_GiBps"] * 2**30)
            roof = {"bound": "hbm", "achieved": round(alg / seconds / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(alg / seconds / 1e9 / HBM_PEAK_GBS, 4),
                    "traffic": None, "algorithmic_bytes_per_launch": alg}
            t = tj.get(key)
            if t and t.get("units") == n_units and t.get("kernel_sources_sha256") == kernel_sources_hash():
                roof["traffic"] = t["hbm_bytes_per_launch"]
                roof["traffic_per_kernel"] = t.get("per_kernel")
                roof["traffic_source"] = t.get("source")
            e["roofline"] = roof
        # the real-data and Zstd numbers next to `value` (same unit; the headline stays BASELINE configs[1] on synthetic blocks)
        result["value_corpus"] = ex["lz4_corpus"]["decompress_GiBps"]            # LZ4 decompress, corpus-tiled 64 KiB blocks (SURVEY 8d C2 primary)
        result["value_corpus_hbm_frac"] = ex["lz4_corpus"]["decompress_hbm_frac"]
        result["value_snappy"] = ex["snappy_fragments"]["decompress_GiBps"]
        result["value_snappy_corpus"] = ex["snappy_corpus"]["decompress_GiBps"]
        if "zstd_fragments" in ex:
            result["value_zstd"] = ex["zstd_fragments"]["decompress_GiBps"]      # Zstd level-3 128 KiB frames (BASELINE configs[3]), synthetic
            result["value_zstd_corpus"] = ex["zstd_corpus"]["decompress_GiBps"]  # the same on corpus-tiled data
        if "zstdstream_corpus" in ex:
            result["value_zstd_stream_corpus"] = ex["zstdstream_corpus"]["decompress_GiBps"]  # frames of several blocks (4 MiB streams), corpus-tiled
        if not args.no_sweep:
            result["sweep_random301"] = sweep_random301(torch, A, codec, dev, args)
    if rank == 0 and world == 1 and args.full and not args.no_host_facing and wl == "lz4_decompress":
        result.update(host_facing(torch, A, codec, pool_pack, pool_pack_off, pool_clen, pool_plain, bs))
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(torch, pool_pack, pool_pack_off, pool_clen, pool_plain, bs, op, wl, args.cpu_seconds)
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def dump_outputs(torch, path, dst, dst_off, cap, out_len, status, err_off):
    """--dump-outputs: the arrays the last timed step handed its caller, for comparing two builds output for output.  Per block (all of them up
    to 2^19, else a seeded sample; `blocks` names them): out_len, status, err_off.  Output bytes of a seeded sample of blocks (32 MiB as
    float32), `cap` bytes from each block's dst_off, -1 past its out_len (what lies there is not output).  Same arguments, same files."""
    os.makedirs(path, exist_ok=True)
    n = out_len.numel()
    rng = np.random.default_rng(301)
    blocks = np.arange(n) if n <= 1 << 19 else np.sort(rng.choice(n, 1 << 19, replace=False))
    sample = np.sort(rng.choice(n, min(n, max(1, (8 << 20) // cap)), replace=False))
    sel = torch.from_numpy(blocks).to(out_len.device)
    arrays = {"blocks": blocks, "out_len": out_len[sel], "status": status[sel], "err_off": err_off[sel], "sample_blocks": sample}
    pick = torch.from_numpy(sample).to(dst.device)
    col = torch.arange(cap, device=dst.device)
    got = dst[dst_off[pick].unsqueeze(1) + col].to(torch.float32)
    got[col.unsqueeze(0) >= out_len[pick].unsqueeze(1)] = -1.0
    arrays["sample_bytes"] = got
    for name, a in arrays.items():
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        np.save(os.path.join(path, name + ".npy"), a.astype(np.float32 if name == "sample_bytes" else np.float64))


def host_facing(torch, A, codec, pool_pack, pool_pack_off, pool_clen, pool_plain, bs):
    """SURVEY 8(d) "timing": the PCIe-inclusive numbers of the headline's workload -- host buffers in, host buffers out -- beside `value` (which is
    HBM-resident and stays the headline), and the latency of the literal drop-in call, one block per call (Lz4HipDecompressor.decompress(MemorySegment,
    MemorySegment) -> achip_lz4_decompress: M/lz4/Lz4JavaDecompressor.java:46-70 is what it replaces).  16384 blocks = 1 GiB of plaintext per call:
      pageable: achip_batch_host on ordinary (numpy) memory -- gather into pinned slots, upload, kernels, download, scatter, pipelined;
      pinned:   the caller keeps its segments in achip_host_alloc_pinned memory and brackets the device-resident batch call with achip_memcpy_h2d / _d2h."""
    import statistics
    lib = codec.lib
    ctx = codec.native.ctx
    pool_n = int(pool_clen.numel())
    n = 16384
    reps = (n + pool_n - 1) // pool_n
    pack = pool_pack.cpu().numpy()
    offs = pool_pack_off.cpu().numpy().astype(np.int64)
    lens = pool_clen.cpu().numpy().astype(np.int32)
    src = np.tile(pack, reps)
    so = (np.tile(offs, reps) + np.repeat(np.arange(reps, dtype=np.int64) * pack.size, pool_n))[:n].copy()
    sl = np.tile(lens, reps)[:n].copy()
    dst = np.zeros(n * bs, dtype=np.uint8)
    do = np.arange(n, dtype=np.int64) * bs
    dc = np.full(n, bs, dtype=np.int32)
    plain0 = pool_plain[:bs].cpu().numpy()
    times = []
    for it in range(6):  # the first call touches the destination's pages and allocates the staging slots: not timed; the median of five (the host's copies vary from call to call)
        t0 = time.perf_counter()
        ol, st, eo = codec.run_host(A.OP_LZ4_DECOMPRESS, src, so, sl, dst, do, dc)
        if it:
            times.append(time.perf_counter() - t0)
        assert (st == 0).all() and (ol == bs).all() and (dst[:bs] == plain0).all() and (dst[(pool_n * (reps - 1)) * bs:(pool_n * (reps - 1)) * bs + bs] == plain0).all()
    pageable = n * bs / statistics.median(times) / 2**30
    pageable_runs = [round(n * bs / t / 2**30, 2) for t in times]
    stages = {k: codec.native.get_stat("host." + k) for k in ("chunks", "total_us", "gather_us", "scatter_us", "wait_slot_us", "wait_download_us")}
    comp_bytes = int(sl.astype(np.int64).sum())
    # pinned segments + explicit copies around the device-resident call
    span = int(so[-1]) + int(sl[-1])
    meta = np.concatenate([so.view(np.uint8), sl.view(np.uint8), do.view(np.uint8), dc.view(np.uint8)])
    h_src, h_dst = lib.achip_host_alloc_pinned(span), lib.achip_host_alloc_pinned(n * bs)
    ctypes.memmove(h_src, src.ctypes.data, span)
    d_src, d_dst = lib.achip_device_alloc(ctx, span + 64), lib.achip_device_alloc(ctx, n * bs + 64)
    d_meta = lib.achip_device_alloc(ctx, meta.size + n * 16 + 64)
    assert h_src and h_dst and d_src and d_dst and d_meta
    lib.achip_memcpy_h2d(ctx, d_meta, meta.ctypes.data, meta.size)
    o_so, o_sl, o_do, o_dc, o_ol, o_st, o_eo = 0, n * 8, n * 12, n * 20, n * 24, n * 28, n * 32
    times = []
    for it in range(4):
        t0 = time.perf_counter()
        lib.achip_memcpy_h2d(ctx, d_src, h_src, span)
        r = lib.achip_lz4_decompress_batch(ctx, d_src, d_meta + o_so, d_meta + o_sl, d_dst, d_meta + o_do, d_meta + o_dc, d_meta + o_ol, d_meta + o_st, d_meta + o_eo, n)
        assert r == 0, r
        lib.achip_memcpy_d2h(ctx, h_dst, d_dst, n * bs)
        lib.achip_ctx_synchronize(ctx)
        if it:
            times.append(time.perf_counter() - t0)
    assert bytes((ctypes.c_uint8 * bs).from_address(h_dst + (n - 1) * bs)) == dst[(n - 1) * bs:].tobytes()
    pinned = n * bs / statistics.median(times) / 2**30
    for ptr in (d_src, d_dst, d_meta):
        lib.achip_device_free(ctx, ptr)
    lib.achip_host_free_pinned(h_src)
    lib.achip_host_free_pinned(h_dst)
    # one block per call through the single-block entry points (host pointers, synchronous): median of 100 calls each, every codec, the headline's
    # kind of data and a block of the reference's corpus (text)
    single = {"block_bytes": bs, "calls": 100,
              "what": "median latency in microseconds of ONE 64 KiB block per call through achip_<codec>_decompress / _compress (host pointers, synchronous): what "
                      "Lz4HipDecompressor.decompress(MemorySegment, MemorySegment) and its siblings cost per call; 'fragments': the headline's data, 'corpus': text"}
    files = corpus_files()
    corpus_blk = np.frombuffer((files.get("canterbury/alice29.txt") or files.get("large/bible.txt") or b"")[:bs], dtype=np.uint8).copy()  # (prose)
    for kind, blk in (("fragments", pool_plain[:bs].cpu().numpy()), ("corpus", corpus_blk if corpus_blk.size == bs else None)):
        if blk is None:
            continue
        for name in ("lz4", "snappy", "zstd"):
            bound = getattr(lib, "achip_%s_max_compressed_length" % name)
            comp_fn, dec_fn = getattr(lib, "achip_%s_compress" % name), getattr(lib, "achip_%s_decompress" % name)
            cap = bound(bs)
            cbuf = np.zeros(cap, dtype=np.uint8)
            back = np.zeros(bs, dtype=np.uint8)
            eo1 = ctypes.c_int64()
            tc, td = [], []
            for it in range(110):
                t0 = time.perf_counter()
                clen1 = comp_fn(ctx, blk.ctypes.data, cbuf.ctypes.data, bs, cap, ctypes.byref(eo1))
                t1 = time.perf_counter()
                r = dec_fn(ctx, cbuf.ctypes.data, back.ctypes.data, clen1, bs, ctypes.byref(eo1))
                t2 = time.perf_counter()
                assert clen1 > 0 and r == bs, (name, kind, clen1, r)
                if it >= 10:
                    tc.append(t1 - t0)
                    td.append(t2 - t1)
            assert (back == blk).all()
            suffix = "" if kind == "fragments" else "_corpus"
            single["%s_decompress%s" % (name, suffix)] = round(statistics.median(td) * 1e6, 1)
            single["%s_compress%s" % (name, suffix)] = round(statistics.median(tc) * 1e6, 1)
    return {
        "end_to_end": {"pageable_GiBps": round(pageable, 2), "pageable_runs_GiBps": pageable_runs, "pinned_GiBps": round(pinned, 2), "blocks": n, "block_bytes": bs, "plain_bytes": n * bs, "compressed_bytes": comp_bytes,
                       "pageable_stages_last_call": stages,
                       "what": "LZ4 decompress of the headline's blocks, host memory in and out (H2D + kernels + D2H): pageable = achip_batch_host on ordinary memory "
                               "(staged through pinned slots, pipelined); pinned = achip_host_alloc_pinned segments, achip_memcpy_h2d + achip_lz4_decompress_batch + "
                               "achip_memcpy_d2h.  PCIe-bound, never `value`"},
        "single_block_us": single,
    }


def kernel_sources_hash():
    """sha256 over the kernel sources (aircompressor_amd/csrc/*.hip, *.h, *.cpp): what profiles/traffic.json's measurement is tied to"""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "aircompressor_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h", ".cpp")):
            h.update(f.encode())
            h.update(open(os.path.join(csrc, f), "rb").read())
    return h.hexdigest()


DECODER_NAMES = {0: "rings", 3: "two-pass (parse to records, a wavefront per block executes)"}


def kernel_symbol(wl, decoder):
    """the dominant kernel of the timed launch as rocprofv3 names it (profiles/*_kernel_stats.csv)"""
    if wl.endswith("decompress") and decoder.startswith("two-pass"):
        return "achip::seq_execute2_kernel<4096, 0> (+ achip::%s_parse2_kernel)" % wl.split("_")[0]
    if wl == "lz4_decompress":
        return "achip::lz4_decompress_rings_kernel<4, 256, 256, 1, false, 4>"
    if wl == "snappy_decompress":
        return "achip::snappy_decompress_rings_kernel<4, 256, 256, 1, false, 1>"
    return "achip::lz4_compress_mw_kernel<unsigned short>" if wl == "lz4_compress" else "achip::snappy_compress_tiers_kernel<true>"


def run_pair(torch, codec, args, name, cop, dop, plain, n, bs, cpu_seconds):
    """One (codec, data) entry: GPU compress of `plain` (n blocks of bs bytes), GPU decompress of the result, verified; CPU legs beside it."""
    lib = codec.lib
    dev = plain.device
    max_c = getattr(lib, "achip_%s_max_compressed_length" % name)(bs)
    cstride = (max_c + 15) // 16 * 16
    i64 = dict(dtype=torch.int64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    p_off = torch.arange(n, **i64) * bs
    p_len = torch.full((n,), bs, **i32)
    c_off = torch.arange(n, **i64) * cstride
    c_cap = torch.full((n,), max_c, **i32)
    comp = torch.empty(n * cstride + 64, dtype=torch.uint8, device=dev)
    clen = torch.zeros(n, **i32)
    st = torch.zeros(n, **i32)
    eo = torch.zeros(n, **i64)
    back = torch.empty(n * bs + 64, dtype=torch.uint8, device=dev)
    blen = torch.zeros(n, **i32)
    torch.cuda.synchronize()

    def timed(fn, iters=3):
        fn()
        codec.synchronize()
        e0, e1 = codec.event(), codec.event()
        codec.record(e0)
        for _ in range(iters):
            fn()
        codec.record(e1)
        return codec.elapsed_ms(e0, e1) / iters * 1e-3

    tc = timed(lambda: codec.launch(cop, plain, p_off, p_len, comp, c_off, c_cap, clen, st, eo, n), iters=2)
    assert int((st != 0).sum()) == 0
    cbytes = int(clen.to(torch.int64).sum())
    td = timed(lambda: codec.launch(dop, comp, c_off, clen, back, p_off, p_len, blen, st, eo, n), iters=5)
    choice = codec.native.get_stat("decompress.choice")  # -1: no probe ran (fixed variant / small batch)
    assert int((st != 0).sum()) == 0 and bool((back[:n * bs] == plain).all())
    entry = {
        "ratio": round(n * bs / cbytes, 3),
        "compress_GiBps": round(n * bs / tc / 2**30, 2), "compress_hbm_frac": round((n * bs + cbytes) / tc / 1e9 / HBM_PEAK_GBS, 4),
        "decompress_GiBps": round(n * bs / td / 2**30, 2), "decompress_hbm_frac": round((n * bs + cbytes) / td / 1e9 / HBM_PEAK_GBS, 4),
        "blocks": n,
        "decoder": DECODER_NAMES.get(choice, "rings"),
    }
    if cpu_seconds > 0 and not args.no_cpu_baseline:
        entry.update(cpu_pair(torch, dop, cop, plain, comp, c_off, clen, min(n, 4096), bs, max_c, cpu_seconds))
    return entry


def extras(torch, A, codec, dev, args):
    """Secondary numbers in the same run (same measurement): the other codec / direction, text-like and corpus-tiled data -- each with the
    CPU rate of the same blocks beside it."""
    out = {}
    bs = args.block_size
    for data_kind in ("fragments", "wordmix", "corpus", "mixed"):
        # every kind at the headline's batch size (BASELINE configs[1]: 256K blocks) -- until round 4 the fragments entries ran 65 536 blocks, one
        # round of the ring decoders' wavefronts, and read 4-8 % below the same kernel on the headline batch
        n = args.blocks
        plain = gen_data(torch, dev, data_kind, n, bs, args.ratio, 977)
        for name, cop, dop in (("lz4", A.OP_LZ4_COMPRESS, A.OP_LZ4_DECOMPRESS), ("snappy", A.OP_SNAPPY_COMPRESS, A.OP_SNAPPY_DECOMPRESS)):
            out["%s_%s" % (name, data_kind)] = run_pair(torch, codec, args, name, cop, dop, plain, n, bs, args.cpu_leg_seconds)
        del plain
    return out


def sweep_random301(torch, A, codec, dev, args):
    """SURVEY 8d C2 secondary: the reference's own synthetic generator (java.util.Random(301), T/snappy/RandomGenerator.java:25-74) at
    compressibility 0.1 / 0.25 / 0.5 / 0.75 / 1.0; 65536 blocks (the generator's 1 MiB = 16 distinct 64 KiB blocks, tiled)."""
    out = {}
    bs, n = args.block_size, 65536
    for ratio in (0.1, 0.25, 0.5, 0.75, 1.0):
        plain = gen_random301(torch, dev, n, bs, ratio)
        for name, cop, dop in (("lz4", A.OP_LZ4_COMPRESS, A.OP_LZ4_DECOMPRESS), ("snappy", A.OP_SNAPPY_COMPRESS, A.OP_SNAPPY_DECOMPRESS)):
            out["%s_ratio_%s" % (name, ratio)] = run_pair(torch, codec, args, name, cop, dop, plain, n, bs, 0.0)
        del plain
    return out


def xxhash_extra(torch, A, codec, dev, args):
    """batched XXH64 / XXH32 of 65536 x 64 KiB device-resident buffers (read-once, HBM-bound)."""
    out = {}
    bs, n = args.block_size, 65536
    data = gen_fragments(torch, dev, n, bs, args.ratio, 555)
    off = torch.arange(n, dtype=torch.int64, device=dev) * bs
    ln = torch.full((n,), bs, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for name, Hasher, dt in (("xxh64", A.XxHash64HipHasher, torch.int64), ("xxh32", A.XxHash32HipHasher, torch.int32)):
        h = Hasher(native_ctx=codec.native)
        res = torch.zeros(n, dtype=dt, device=dev)
        h.hash_batch(data, off, ln, res, n, seed=7)
        codec.synchronize()
        e0, e1 = codec.event(), codec.event()
        codec.record(e0)
        for _ in range(5):
            h.hash_batch(data, off, ln, res, n, seed=7)
        codec.record(e1)
        t = codec.elapsed_ms(e0, e1) / 5 * 1e-3
        # spot check against the third-party xxhash module when it is there (the parity tests use the oracle)
        try:
            import xxhash
            b0 = data[:bs].cpu().numpy().tobytes()
            want = xxhash.xxh64(b0, seed=7).intdigest() if name == "xxh64" else xxhash.xxh32(b0, seed=7).intdigest()
            assert int(res[0].item()) & ((1 << (64 if name == "xxh64" else 32)) - 1) == want
        except ImportError:
            pass
        out[name] = {"GiBps": round(n * bs / t / 2**30, 2), "hbm_frac": round(n * bs / t / 1e9 / HBM_PEAK_GBS, 4), "buffers": n, "buffer_bytes": bs}
    return out


def lz4frame_extra(torch, A, codec, dev, args):
    """LZ4 frame container, one frame of 4 MiB blocks per item (what Lz4FrameJavaCompressor writes);
    GPU encode (byte-identical to the Java frame encoder), then GPU decode, verified against the plaintext.
    SURVEY 8f row 2: x-snappy-framed streams of 4 MiB (what SnappyFramedOutputStream writes: 64 KiB chunks with masked CRC-32C)."""
    out = container_extra(torch, A, codec, dev, args, "lz4frame", A.OP_LZ4FRAME_COMPRESS, A.OP_LZ4FRAME_DECOMPRESS)
    # the same container in a batch that can fill the chip (1024 frames of one 4 MiB block each are 1024 units of work for 1024 SIMDs): 16384
    # frames of 256 KiB -- still one block per frame (the writer's block size is 4 MiB: Lz4FrameCompression.java:93-133)
    out.update(container_extra(torch, A, codec, dev, args, "lz4frame", A.OP_LZ4FRAME_COMPRESS, A.OP_LZ4FRAME_DECOMPRESS, fs=256 << 10, n=16384, suffix="256k"))
    out.update(container_extra(torch, A, codec, dev, args, "snappyframed", A.OP_SNAPPYFRAMED_COMPRESS, A.OP_SNAPPYFRAMED_DECOMPRESS))
    # SURVEY 8f row 2, second half: Hadoop block streams of 4 MiB (what Lz4HadoopOutputStream / SnappyHadoopOutputStream write at the default
    # 256 KiB buffer: [BE length][BE length][block] per 259523 / 218422 plaintext bytes)
    out.update(container_extra(torch, A, codec, dev, args, "lz4hadoop", A.OP_LZ4HADOOP_COMPRESS, A.OP_LZ4HADOOP_DECOMPRESS, max_c=codec.lib.achip_hadoop_max_compressed_length(0, 4 << 20, 262144)))
    out.update(container_extra(torch, A, codec, dev, args, "snappyhadoop", A.OP_SNAPPYHADOOP_COMPRESS, A.OP_SNAPPYHADOOP_DECOMPRESS, max_c=codec.lib.achip_hadoop_max_compressed_length(1, 4 << 20, 262144)))
    return out


def container_extra(torch, A, codec, dev, args, name, cop, dop, max_c=None, fs=4 << 20, n=1024, suffix=""):
    out = {}
    lib = codec.lib
    if max_c is None:
        max_c = getattr(lib, "achip_%s_max_compressed_length" % name)(fs)
    cstride = (max_c + 15) // 16 * 16
    i64 = dict(dtype=torch.int64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    for data_kind in ("fragments", "corpus"):
        plain = gen_data(torch, dev, data_kind, n * (fs // args.block_size), args.block_size, args.ratio, 99)
        p_off = torch.arange(n, **i64) * fs
        p_len = torch.full((n,), fs, **i32)
        comp = torch.empty(n * cstride + 64, dtype=torch.uint8, device=dev)
        c_off = torch.arange(n, **i64) * cstride
        c_cap = torch.full((n,), max_c, **i32)
        clen = torch.zeros(n, **i32)
        st = torch.zeros(n, **i32)
        eo = torch.zeros(n, **i64)
        back = torch.empty(n * fs + 64, dtype=torch.uint8, device=dev)
        blen = torch.zeros(n, **i32)
        torch.cuda.synchronize()

        def timed(fn, iters):
            fn()
            codec.synchronize()
            e0, e1 = codec.event(), codec.event()
            codec.record(e0)
            for _ in range(iters):
                fn()
            codec.record(e1)
            return codec.elapsed_ms(e0, e1) / iters * 1e-3

        tc = timed(lambda: codec.launch(cop, plain, p_off, p_len, comp, c_off, c_cap, clen, st, eo, n), 1)
        assert int((st != 0).sum()) == 0
        cbytes = int(clen.to(torch.int64).sum())
        td = timed(lambda: codec.launch(dop, comp, c_off, clen, back, p_off, p_len, blen, st, eo, n), 2)
        assert int((st != 0).sum()) == 0 and bool((back[:n * fs] == plain).all())
        entry = {
            "ratio": round(n * fs / cbytes, 3), "compress_GiBps": round(n * fs / tc / 2**30, 2), "decompress_GiBps": round(n * fs / td / 2**30, 2),
            "decompress_hbm_frac": round((n * fs + cbytes) / td / 1e9 / HBM_PEAK_GBS, 4), "frames": n, "frame_bytes": fs,
        }
        if not args.no_cpu_baseline:
            # the CPU leg beside it: the oracle's writer / reader of the same container over the first streams of this
            # very batch (256 MiB of plaintext), all host threads, one stream per call
            entry.update(cpu_pair(torch, dop, cop, plain, comp, c_off, clen, min(n, max(host_threads(), (256 << 20) // fs)), fs, int(max_c), args.cpu_leg_seconds))
        out["%s%s_%s" % (name, suffix, data_kind)] = entry
        del comp, back, plain
    return out


def zstd_extra(torch, A, codec, dev, args):
    """Zstd level-3 frames of 128 KiB (BASELINE configs[3]), two encodings: frames made on the host by
    libzstd via pyarrow (a third-party encoder) and frames made by the product's GPU encoder (byte-identical to the
    Java encoder's); both decoded on the GPU and verified against the plaintext."""
    import pyarrow as pa
    out = {}
    fs = 131072
    pool_n, reps = 512, 128   # 65536 frames = 8 GiB of plaintext per launch
    if args.zstd_variant >= 0:
        codec.native.set_option("zstd.decompress.variant", args.zstd_variant)
    if args.zstd_exec >= 0:
        codec.native.set_option("zstd.decompress.exec", args.zstd_exec)
    if args.zstd_seq_waves > 0:
        codec.native.set_option("zstd.decompress.seq_waves", args.zstd_seq_waves)
    if args.zstd_compress_variant >= 0:
        codec.native.set_option("zstd.compress.variant", args.zstd_compress_variant)
    zc = pa.Codec("zstd", compression_level=3)
    for data_kind in [k for k in ("fragments", "wordmix", "corpus") if k in args.zstd_kinds.split(",")]:
        plain = gen_data(torch, dev, data_kind, pool_n, fs, args.ratio, 4242)
        host = plain.cpu().numpy()
        frames = [zc.compress(host[i * fs:(i + 1) * fs].tobytes(), asbytes=True) for i in range(pool_n)]
        lens = np.array([len(f) for f in frames], dtype=np.int64)
        pad = (lens + 15) // 16 * 16
        offs = np.cumsum(pad) - pad
        pack = np.zeros(int(pad.sum()), dtype=np.uint8)
        for f, o in zip(frames, offs):
            pack[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
        n = pool_n * reps
        i64 = dict(dtype=torch.int64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        d_pack = torch.from_numpy(pack).to(dev).repeat(reps)
        rep_idx = torch.arange(reps, **i64).repeat_interleave(pool_n)
        src_off = torch.from_numpy(offs).to(dev).repeat(reps) + rep_idx * int(pad.sum())
        src_len = torch.from_numpy(lens.astype(np.int32)).to(dev).repeat(reps)
        dst = torch.empty(n * fs + 64, dtype=torch.uint8, device=dev)
        dst_off = torch.arange(n, **i64) * fs
        dst_cap = torch.full((n,), fs, **i32)
        olen = torch.zeros(n, **i32)
        st = torch.zeros(n, **i32)
        eo = torch.zeros(n, **i64)
        torch.cuda.synchronize()
        launch = lambda: codec.launch(A.OP_ZSTD_DECOMPRESS, d_pack, src_off, src_len, dst, dst_off, dst_cap, olen, st, eo, n)  # noqa: E731
        launch()
        codec.synchronize()
        assert int((st != 0).sum()) == 0, "zstd decode failed"
        assert bool((dst[:n * fs].view(reps, pool_n * fs) == plain.unsqueeze(0)).all()), "zstd plaintext mismatch"
        fallback = codec.native.get_stat("zstd.decompress.fallback_items")
        e0, e1 = codec.event(), codec.event()
        iters = 3
        codec.record(e0)
        for _ in range(iters):
            launch()
        codec.record(e1)
        t = codec.elapsed_ms(e0, e1) / iters * 1e-3
        cbytes = int(lens.sum()) * reps
        entry = {
            "ratio": round(n * fs / cbytes, 3), "decompress_GiBps": round(n * fs / t / 2**30, 2),
            "decompress_hbm_frac": round((n * fs + cbytes) / t / 1e9 / HBM_PEAK_GBS, 4), "frames": n, "frame_bytes": fs,
            "encoder": "libzstd level 3 via pyarrow %s" % pa.__version__, "one_kernel_fallback_items": fallback,
        }
        del d_pack, dst
        # GPU level-3 encoder (bit-exact with the Java encoder) over the same plaintext, then GPU decode of its frames
        max_c = lib_max = codec.lib.achip_zstd_max_compressed_length(fs)
        cstride = (max_c + 15) // 16 * 16
        nz = pool_n * 64
        zplain = plain.repeat(64)
        z_src_off = torch.arange(nz, **i64) * fs
        z_src_len = torch.full((nz,), fs, **i32)
        z_dst = torch.empty(nz * cstride + 64, dtype=torch.uint8, device=dev)
        z_dst_off = torch.arange(nz, **i64) * cstride
        z_dst_cap = torch.full((nz,), max_c, **i32)
        z_len = torch.zeros(nz, **i32)
        z_st = torch.zeros(nz, **i32)
        z_eo = torch.zeros(nz, **i64)
        torch.cuda.synchronize()
        zl = lambda: codec.launch(A.OP_ZSTD_COMPRESS, zplain, z_src_off, z_src_len, z_dst, z_dst_off, z_dst_cap, z_len, z_st, z_eo, nz)  # noqa: E731
        zl()
        codec.synchronize()
        assert int((z_st != 0).sum()) == 0, "zstd encode failed"
        e0, e1 = codec.event(), codec.event()
        codec.record(e0)
        zl()
        codec.record(e1)
        tz = codec.elapsed_ms(e0, e1) * 1e-3
        zbytes = int(z_len.to(torch.int64).sum())
        back = torch.empty(nz * fs + 64, dtype=torch.uint8, device=dev)
        b_len = torch.zeros(nz, **i32)
        codec.launch(A.OP_ZSTD_DECOMPRESS, z_dst, z_dst_off, z_len, back, z_src_off, z_src_len, b_len, z_st, z_eo, nz)
        codec.synchronize()
        assert int((z_st != 0).sum()) == 0 and bool((back[:nz * fs] == zplain).all()), "zstd GPU encode -> GPU decode round trip failed"
        codec.record(e0)
        for _ in range(3):
            codec.launch(A.OP_ZSTD_DECOMPRESS, z_dst, z_dst_off, z_len, back, z_src_off, z_src_len, b_len, z_st, z_eo, nz)
        codec.record(e1)
        tj = codec.elapsed_ms(e0, e1) / 3 * 1e-3
        entry.update({"java_frames_decompress_GiBps": round(nz * fs / tj / 2**30, 2), "java_frames": nz,
                      "java_frames_fallback_items": codec.native.get_stat("zstd.decompress.fallback_items")})
        entry.update({"gpu_encoder_ratio": round(nz * fs / zbytes, 3), "compress_GiBps": round(nz * fs / tz / 2**30, 2),
                      "compress_hbm_frac": round((nz * fs + zbytes) / tz / 1e9 / HBM_PEAK_GBS, 5), "compress_frames": nz})
        if not args.no_cpu_baseline and args.cpu_leg_seconds > 0:
            # CPU legs: the oracle's Zstd decoder over the same libzstd frames (pool x 8 per pass) and its level-3 encoder over the same plaintext
            T = host_threads()
            d, _ = cpu_rate(A.OP_ZSTD_DECOMPRESS, pack, np.tile(offs, 8), np.tile(lens.astype(np.int32), 8), fs, T, args.cpu_leg_seconds)
            c, _ = cpu_rate(A.OP_ZSTD_COMPRESS, host, np.tile(np.arange(pool_n, dtype=np.int64) * fs, 8), np.full(pool_n * 8, fs, dtype=np.int32), int(max_c), T, args.cpu_leg_seconds)
            entry.update({"cpu_decompress_GiBps": round(d, 2), "cpu_compress_GiBps": round(c, 2), "cpu_threads": T, "cpu_sample_blocks": pool_n * 8})
        out["zstd_%s" % data_kind] = entry
        del z_dst, back, zplain
    return out


def zstd_stream_extra_isolated():
    """zstd_stream_extra in a process of its own (this command line + --section zstdstream): the defaults of the multi-block stages were
    last touched after the round's GPU minutes were spent (CPU-emulator-verified only), and a device fault there must not take the run's
    line with it -- an exception can be caught, an aborted process cannot."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ["--section", "zstdstream"], capture_output=True, text=True, timeout=1200)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        raise RuntimeError("exit %d: %s" % (r.returncode, r.stderr[-400:]))
    return json.loads(lines[-1])


def zstd_stream_extra(torch, A, codec, dev, args):
    """Zstd frames of SEVERAL blocks (what ZstdOutputStream / ZstdFrameCompressor / libzstd write beyond 128 KiB):
    1024 frames of 4 MiB (32 blocks each, libzstd level 3 on the host) decoded through the pipeline's multi-block stages, and -- one
    launch -- through the one-kernel decoder that took such frames before (zstd.decompress.stream_blocks = 0)."""
    import pyarrow as pa
    out = {}
    fs, pool_n, reps = 4 << 20, 16, 64
    zc = pa.Codec("zstd", compression_level=3)
    i64 = dict(dtype=torch.int64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    for data_kind in ("fragments", "corpus"):
        plain = gen_data(torch, dev, data_kind, pool_n * (fs // args.block_size), args.block_size, args.ratio, 515)
        host = plain.cpu().numpy()
        frames = [zc.compress(host[i * fs:(i + 1) * fs].tobytes(), asbytes=True) for i in range(pool_n)]
        lens = np.array([len(f) for f in frames], dtype=np.int64)
        pad = (lens + 15) // 16 * 16
        offs = np.cumsum(pad) - pad
        pack = np.zeros(int(pad.sum()), dtype=np.uint8)
        for f, o in zip(frames, offs):
            pack[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
        n = pool_n * reps
        d_pack = torch.from_numpy(pack).to(dev).repeat(reps)
        rep_idx = torch.arange(reps, **i64).repeat_interleave(pool_n)
        src_off = torch.from_numpy(offs).to(dev).repeat(reps) + rep_idx * int(pad.sum())
        src_len = torch.from_numpy(lens.astype(np.int32)).to(dev).repeat(reps)
        dst = torch.empty(n * fs + 64, dtype=torch.uint8, device=dev)
        dst_off = torch.arange(n, **i64) * fs
        dst_cap = torch.full((n,), fs, **i32)
        olen = torch.zeros(n, **i32)
        st = torch.zeros(n, **i32)
        eo = torch.zeros(n, **i64)
        torch.cuda.synchronize()
        launch = lambda: codec.launch(A.OP_ZSTD_DECOMPRESS, d_pack, src_off, src_len, dst, dst_off, dst_cap, olen, st, eo, n)  # noqa: E731

        def check():
            codec.synchronize()
            assert int((st != 0).sum()) == 0, "zstd multi-block decode failed"
            assert bool((dst[:n * fs].view(reps, pool_n * fs) == plain.unsqueeze(0)).all()), "zstd multi-block plaintext mismatch"

        def timed(iters):
            e0, e1 = codec.event(), codec.event()
            codec.record(e0)
            for _ in range(iters):
                launch()
            codec.record(e1)
            return codec.elapsed_ms(e0, e1) / iters * 1e-3

        launch()
        check()
        fast = codec.native.get_stat("zstd.decompress.multiblock_fast_items")
        blocks = codec.native.get_stat("zstd.decompress.multiblock_blocks")
        t = timed(3)
        dst.zero_()
        codec.native.set_option("zstd.decompress.stream_blocks", 0)
        t1 = timed(1)
        check()
        codec.native.set_option("zstd.decompress.stream_blocks", 65536)
        cbytes = int(lens.sum()) * reps
        entry = {
            "ratio": round(n * fs / cbytes, 3), "decompress_GiBps": round(n * fs / t / 2**30, 2), "decompress_hbm_frac": round((n * fs + cbytes) / t / 1e9 / HBM_PEAK_GBS, 4),
            "one_kernel_decoder_GiBps": round(n * fs / t1 / 2**30, 2), "frames": n, "frame_bytes": fs, "blocks": blocks, "multiblock_fast_items": fast,
            "encoder": "libzstd level 3 via pyarrow %s" % pa.__version__,
        }
        if not args.no_cpu_baseline and args.cpu_leg_seconds > 0:
            # CPU leg: the oracle's decoder (the Java frame decoder restated) over the same frames, one frame per call, all host threads
            T = host_threads()
            tile = max(1, (T + pool_n - 1) // pool_n)
            d, _ = cpu_rate(A.OP_ZSTD_DECOMPRESS, pack, np.tile(offs, tile), np.tile(lens.astype(np.int32), tile), fs, T, args.cpu_leg_seconds)
            entry.update({"cpu_decompress_GiBps": round(d, 2), "cpu_threads": min(T, pool_n * tile), "cpu_sample_blocks": pool_n * tile})
        out["zstdstream_%s" % data_kind] = entry
        del d_pack, dst, plain
    return out


_oracle = None


def oracle_bench_lib():
    """oracle/liboracle.so (the C restatement of the Java codecs; no JVM on the box) -- ONLY the cpu_baseline legs come here."""
    global _oracle
    if _oracle is None:
        from tests import oracle_lib
        lib = oracle_lib.load().lib
        lib.orc_bench.restype = ctypes.c_double
        lib.orc_bench.argtypes = [ctypes.c_int32] + [ctypes.c_void_p] * 6 + [ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
                                                                             ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]
        _oracle = lib
    return _oracle


def cpu_rate(op, src, src_off, src_len, cap, threads, seconds):
    """GiB/s of plaintext for `op` over the given host blocks: T pthreads inside the oracle library, each on its own contiguous range of
    blocks with its own output ranges, passes repeated for `seconds` (oracle/misc.c orc_bench -- no Python in the timed loop)."""
    lib = oracle_bench_lib()
    n = len(src_off)
    stride = (cap + 63) // 64 * 64
    dst = np.empty(n * stride + 64, dtype=np.uint8)
    dst_off = np.arange(n, dtype=np.int64) * stride
    dst_cap = np.full(n, cap, dtype=np.int32)
    src = np.ascontiguousarray(src)
    src_off = np.ascontiguousarray(src_off, dtype=np.int64)
    src_len = np.ascontiguousarray(src_len, dtype=np.int32)
    passes, failures = ctypes.c_double(), ctypes.c_int64()
    rate = lib.orc_bench(op, src.ctypes.data, src_off.ctypes.data, src_len.ctypes.data, dst.ctypes.data, dst_off.ctypes.data, dst_cap.ctypes.data,
                         n, threads, seconds, ctypes.byref(passes), ctypes.byref(failures))
    assert failures.value == 0, "the CPU baseline failed on %d blocks" % failures.value
    return rate / 2**30, passes.value


def host_threads():
    return max(1, min(os.cpu_count() or 1, 1024))


def cpu_pair(torch, dop, cop, plain, comp, c_off, clen, n_sample, bs, max_c, seconds):
    """CPU rates of one extra entry: the first n_sample blocks of the same batch, decompress and compress, all host threads."""
    if seconds <= 0:
        return {}
    T = host_threads()
    k = int(n_sample)
    h_plain = plain[:k * bs].cpu().numpy()
    offs = c_off[:k].cpu().numpy().astype(np.int64)
    lens = clen[:k].cpu().numpy().astype(np.int32)
    end = int(offs[-1]) + int(lens[-1])
    h_comp = comp[:end].cpu().numpy()
    d, _ = cpu_rate(dop, h_comp, offs, lens, bs, T, seconds)
    c, _ = cpu_rate(cop, h_plain, np.arange(k, dtype=np.int64) * bs, np.full(k, bs, dtype=np.int32), max_c, T, seconds)
    return {"cpu_decompress_GiBps": round(d, 2), "cpu_compress_GiBps": round(c, 2), "cpu_threads": min(T, k), "cpu_sample_blocks": k}


def cpu_baseline(torch, pool_pack, pool_pack_off, pool_clen, pool_plain, bs, op, wl, seconds):
    """The headline's CPU leg: the oracle (C restatement of the Java codec -- no JVM on this box) on the GPU box's host cores over the
    SAME blocks: the pool's distinct blocks repeated to >= 1 GiB of plaintext per pass, one codec state per thread."""
    n = int(pool_clen.numel())
    reps = max(1, (16384 + n - 1) // n)
    T = host_threads()
    codec = "lz4" if wl.startswith("lz4") else "snappy"
    if wl.endswith("decompress"):
        src = pool_pack.cpu().numpy()
        src_off = np.tile(pool_pack_off.cpu().numpy().astype(np.int64), reps)
        src_len = np.tile(pool_clen.cpu().numpy().astype(np.int32), reps)
        cap = bs
    else:
        src = pool_plain.cpu().numpy()
        src_off = np.tile(np.arange(n, dtype=np.int64) * bs, reps)
        src_len = np.full(n * reps, bs, dtype=np.int32)
        from tests import oracle_lib
        cap = int(oracle_lib.load().max_compressed_length(codec, bs))
    r1, p1 = cpu_rate(op, src, src_off[:max(64, n // 16)], src_len[:max(64, n // 16)], cap, 1, seconds * 0.2)
    # ONE number for north_star's ">= 4x aggregate over the CPU baseline at 8 GPUs": the 4096-block sample (256 MiB of plaintext per pass: 16
    # blocks per thread on 256 threads, cache-resident -- the CPU at its best, the conservative bar; it is also the sample of every
    # `extra` entry's CPU leg).  The >= 1 GiB sample, which on this host is bound by its memory system, is reported beside it.
    k = min(4096, n * reps)
    rC, pC = cpu_rate(op, src, src_off[:k], src_len[:k], cap, T, seconds * 0.4)
    rN, pN = cpu_rate(op, src, src_off, src_len, cap, T, seconds * 0.4)
    return {
        "value": round(rC, 3), "unit": "GiB/s", "cores": T, "kind": "port",
        "value_1_thread": round(r1, 3), "value_1GiB_sample": round(rN, 3),
        "criterion": "north_star's >= 4x at 8 GPUs is evaluated against `value` (the cache-resident 4096-block sample: the higher of the two CPU figures)",
        "sample": "%d blocks of %d bytes per pass (%d distinct %s blocks, %s), %.1f passes per thread on %d pthreads for %.1f s; value_1GiB_sample: %d blocks per pass, %.1f passes; "
                  "oracle/liboracle.so = C restatement of the Java codec (no JVM on the box; pinned against the transliterated reference sources, tests/test_ref_pin.py), "
                  "one codec state per thread, disjoint block ranges" % (k, bs, n, codec.upper(), wl, pC, T, seconds * 0.4, n * reps, pN),
    }


if __name__ == "__main__":
    sys.exit(main() or 0)
