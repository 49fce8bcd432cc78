"""The LZO1X block codec on the GPU (lzo_decompress.hip, lzo_compress.hip, the LZO lines of decoded_size.hip and pack_outputs.hip) against the pure-Python
model tests/lzo_ref.py over the catalog tests/lzo_cases.py: the decoders at every variant and at the lane parser's wavefront edge, the two-pass condition and
the hand-over of an exhausted arena, the encoder byte for byte, sizing and planning, the single calls, the Python classes, mixed and host batches, and a
short differential fuzz run."""
import random

import numpy as np
import pytest

from tests import common, lzo_cases as cases, lzo_ref as ref

pytestmark = pytest.mark.gpu

MALFORMED = -(1 + 16 * 111)   # ACHIP_CLASS_MALFORMED / ACHIP_D_LZO_MALFORMED
MAX_OUTPUT = -(2 + 16 * 113)  # ACHIP_CLASS_OUTPUT_TOO_SMALL / ACHIP_D_LZO_MAX_OUTPUT
OP_DEC, OP_ENC = 16, 17


@pytest.fixture(scope="module")
def g():
    from tests.gpu_harness import GpuBatch
    return GpuBatch(0)


@pytest.fixture(scope="module")
def runs():
    """[(label, stream, capacity, the model's verdict)]: every decode case with exact and with generous room (computed once, never changed)"""
    out = []
    for case in cases.decode_cases():
        for cap, exp in cases.runs(case):
            out.append((case[0], case[1], cap, exp))
    return tuple(out)


def check(batch, outs, status, err, tag):
    wrong = []
    for (label, stream, cap, exp), got, st, eo in zip(batch, outs, status, err):
        if exp[0] == "ok":
            ok = st == 0 and got == exp[1]
        else:
            ok = st == MALFORMED and eo == exp[1] and got == b""
        if not ok:
            wrong.append((tag, label, cap, st, eo, len(got), exp[0], exp[1] if exp[0] != "ok" else len(exp[1])))
    assert not wrong, wrong[:6]


@pytest.mark.parametrize("size", [1, 63, 64, 65])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_decode_catalog(g, runs, variant, size):
    """the whole catalog in batches of `size` items (the last one filled up from the catalog's start): plaintext, length, status and offset are the
    model's for every item -- malformed items sit between valid ones in every batch"""
    g.set_option("lzo.decompress.variant", variant)
    g.set_option("lzo.decompress.max_chunks", 0)
    for first in range(0, len(runs), size):
        batch = [runs[(first + k) % len(runs)] for k in range(size)]
        outs, status, err = g.run(OP_DEC, [b[1] for b in batch], [b[2] for b in batch], unaligned=(first // size) % 2 == 1)
        check(batch, outs, status, err, "variant %d, items %d.." % (variant, first))
        if variant == 1:  # the two-pass condition, batch by batch: the parser hands nothing of the tiled catalog to the wavefront decoder
            assert g.codec.native.get_stat("lzo.decompress.fallback_blocks") == 0, first
    g.set_option("lzo.decompress.variant", 0)


def test_auto_takes_the_two_passes_from_its_line_on(g, runs):
    g.set_option("lzo.decompress.variant", 0)
    g.set_option("lzo.decompress.auto_min_blocks", 100)
    try:
        outs, status, err = g.run(OP_DEC, [b[1] for b in runs], [b[2] for b in runs])
        assert g.codec.native.get_stat("lzo.decompress.fallback_blocks") == 0
        check(runs, outs, status, err, "auto, two passes")
        outs, status, err = g.run(OP_DEC, [b[1] for b in runs[:99]], [b[2] for b in runs[:99]])
        check(runs[:99], outs, status, err, "auto, a wavefront per item")
    finally:
        g.set_option("lzo.decompress.auto_min_blocks", 8192)


@pytest.mark.parametrize("variant", [1, 2])
def test_long_run_item(g, runs, variant):
    """a match-length extension of more than 16 383 bytes (the record's skip field): ~4 MiB at offset 1, beside ordinary items"""
    label, stream, _ = cases.long_run_case()
    n = ref.decoded_size(stream)
    assert n > 4000000 and len(stream) > 16383 + 16
    plain = ref.decompress(stream, n)
    batch = list(runs[:5]) + [(label, stream, n, ("ok", plain)), (label, stream, n - 1, cases.expected(stream, n - 1))] + list(runs[5:9])
    g.set_option("lzo.decompress.variant", variant)
    outs, status, err = g.run(OP_DEC, [b[1] for b in batch], [b[2] for b in batch])
    g.set_option("lzo.decompress.variant", 0)
    check(batch, outs, status, err, "long run, variant %d" % variant)


def test_two_pass_condition_and_the_exhausted_arena(g, runs):
    """with the default arena the two passes decode the whole catalog themselves (no item is handed to the wavefront decoder); with the arena squeezed to 24
    chunks items are handed over, and the bytes are the same"""
    g.set_option("lzo.decompress.variant", 1)
    try:
        outs, status, err = g.run(OP_DEC, [b[1] for b in runs], [b[2] for b in runs])
        assert g.codec.native.get_stat("lzo.decompress.fallback_blocks") == 0
        check(runs, outs, status, err, "two passes")
        g.set_option("lzo.decompress.max_chunks", 24)
        outs2, status2, err2 = g.run(OP_DEC, [b[1] for b in runs], [b[2] for b in runs])
        handed = g.codec.native.get_stat("lzo.decompress.fallback_blocks")
        print("handed over with an arena of 24 chunks: %d of %d items" % (handed, len(runs)))
        assert 0 < handed < len(runs)
        check(runs, outs2, status2, err2, "two passes, squeezed arena")
        assert outs2 == outs and status2 == status and err2 == err
    finally:
        g.set_option("lzo.decompress.max_chunks", 0)
        g.set_option("lzo.decompress.variant", 0)


@pytest.fixture(scope="module")
def encoded():
    inputs = [(label, data) for label, data, _ in cases.encode_cases()]
    return inputs, [ref.compress(d) for _, d in inputs]


def test_encode_catalog(g, encoded):
    inputs, want = encoded
    blocks = [d for _, d in inputs]
    bounds = [ref.max_compressed_length(len(d)) for d in blocks]
    outs, status, err = g.run(OP_ENC, blocks, bounds, unaligned=True)
    wrong = [(label, len(d), st, len(o), len(w)) for (label, d), o, w, st in zip(inputs, outs, want, status) if st != 0 or o != w]
    assert not wrong, wrong[:6]
    assert all(e == 0 for e in err)
    # a capacity one below the bound is refused -- for the empty input too (the reference checks the bound before "nothing compresses to nothing")
    outs1, status1, _ = g.run(OP_ENC, blocks, [b - 1 for b in bounds])
    assert status1 == [MAX_OUTPUT] * len(blocks) and all(o == b"" for o in outs1)
    # ... and the GPU decoder restores every plaintext from the GPU encoder's bytes
    for variant in (1, 2):
        g.set_option("lzo.decompress.variant", variant)
        plain, status2, _ = g.run(OP_DEC, outs, [len(d) for d in blocks])
        g.set_option("lzo.decompress.variant", 0)
        assert status2 == [0] * len(blocks) and plain == blocks, variant


def to_device(g, a):
    return g.torch.from_numpy(np.ascontiguousarray(a)).to(g.dev)


def upload(g, items, misalign=3):
    offs, pos = [], misalign
    for b in items:
        offs.append(pos)
        pos += len(b) + (len(b) % 5) + 1
    src = np.zeros(pos + 64, dtype=np.uint8)
    for b, so in zip(items, offs):
        src[so:so + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return to_device(g, src), to_device(g, np.array(offs, dtype=np.int64)), to_device(g, np.array([len(b) for b in items], dtype=np.int32))


def test_size_plan_decode(g, runs):
    """size -> achip_plan_outputs -> decode for a mixed valid / malformed batch: sizes, statuses and offsets are the model's for a capacity of INT32_MAX; the
    valid items decode to their plaintext at the planned places, the malformed ones are left out"""
    torch = g.torch
    streams = [b[1] for b in runs if b[2] != 0][::2]
    d_src, d_off, d_len = upload(g, streams)
    alloc = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=g.dev)  # noqa: E731
    r = g.codec.decompress_unsized(OP_DEC, d_src, d_off, d_len, len(streams), alloc, align=16)
    g.codec.synchronize()
    n = len(streams)
    view = lambda t, dt: t.cpu().numpy().view(dt)[:n]  # noqa: E731
    size, sst, serr = view(r["out_size"], np.int64), view(r["size_status"], np.int32), view(r["size_err_off"], np.int64)
    off, out_len, status = view(r["dst_off"], np.int64), view(r["out_len"], np.int32), view(r["status"], np.int32)
    dst = r["dst"].cpu().numpy()
    left_out = 0
    for i, s in enumerate(streams):
        try:
            plain = ref.decompress(s, ref.INT_MAX)
        except ref.Malformed as e:
            left_out += 1
            assert (size[i], sst[i], serr[i]) == (0, MALFORMED, e.offset), (i, size[i], sst[i], serr[i], e.offset)
            continue
        assert (size[i], sst[i]) == (len(plain), 0), i
        assert status[i] == 0 and out_len[i] == len(plain) and dst[off[i]:off[i] + len(plain)].tobytes() == plain, i
        assert off[i] % 16 == 0
    assert 0 < left_out < n and r["left_out"] == left_out


def test_bound_compress_pack(g, encoded):
    torch = g.torch
    inputs, want = encoded
    blocks = [d for _, d in inputs]
    d_src, d_off, d_len = upload(g, blocks)
    alloc = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=g.dev)  # noqa: E731
    r = g.codec.compress_packed(OP_ENC, d_src, d_off, d_len, len(blocks), alloc, align=1)
    g.codec.synchronize()
    n = len(blocks)
    bound = r["bound"].cpu().numpy().view(np.int64)[:n]
    assert bound.tolist() == [ref.max_compressed_length(len(d)) for d in blocks]
    assert r["total_bytes"] == sum(len(w) for w in want) and r["left_out"] == 0
    assert r["packed"].cpu().numpy()[:r["total_bytes"]].tobytes() == b"".join(want)


def test_python_classes_and_single_calls(g, encoded):
    """LzoHipCompressor / LzoHipDecompressor over achip_lzo_compress / achip_lzo_decompress: the model's bytes, the Java classes' exceptions"""
    import aircompressor_amd as A
    c, d = A.LzoHipCompressor(), A.LzoHipDecompressor()
    inputs, want = encoded
    for (label, data), w in list(zip(inputs, want))[::5]:
        out = bytearray(c.max_compressed_length(len(data)) + 5)
        n = c.compress(data, 0, len(data), out, 2, len(out) - 2)
        assert bytes(out[2:2 + n]) == w, label
        back = bytearray(len(data) + 3)
        assert d.decompress(w, 0, len(w), back, 1, len(data)) == len(data) and bytes(back[1:1 + len(data)]) == data, label
        assert d.decompress_segment(memoryview(w), back) == len(data)
    assert c.max_compressed_length(65536) == 65536 + 257 + 16 and c.get_retained_size_in_bytes(1) == 4096
    assert c.compress_segment(b"hello hello hello hello hello", bytearray(64)) == len(ref.compress(b"hello hello hello hello hello"))
    with pytest.raises(A.IllegalArgumentException, match="Max output length"):
        c.compress(b"x" * 100, 0, 100, bytearray(115), 0, 115)
    with pytest.raises(A.IllegalArgumentException, match="Invalid offset or length"):
        c.compress(b"x" * 100, 0, 101, bytearray(200), 0, 200)
    w = want[-1]
    plain_len = len(inputs[-1][1])
    with pytest.raises(A.MalformedInputException) as e:
        d.decompress(w, 0, len(w), bytearray(plain_len), 0, plain_len - 1)  # "output too small" is a MalformedInputException in this decoder
    assert e.value.offset == cases.expected(w, plain_len - 1)[1]
    with pytest.raises(A.MalformedInputException) as e:
        d.decompress(w, 0, len(w) - 3, bytearray(plain_len), 0, plain_len)
    assert e.value.offset == cases.expected(w[:-3], plain_len)[1]
    assert d.decompress(b"", 0, 0, bytearray(4), 0, 4) == 0


def test_mixed_batch_with_every_block_codec(g, encoded):
    """LZ4, Snappy, Zstd and LZO items interleaved in one achip_mixed_batch, encodes and decodes"""
    from tests import oracle_lib
    o = oracle_lib.load()
    inputs, want = encoded
    texts = [d for _, d, _ in common.corpus_sample()[:4]] + [d for _, d in inputs if 20 < len(d) < 30000][:12]
    ops, blocks, caps, expect = [], [], [], []
    for k, data in enumerate(texts):
        for codec, cop, dop in (("lz4", 1, 0), ("snappy", 3, 2), ("zstd", 5, 4)):
            comp = o.compress(codec, data)
            ops += [cop, dop]
            blocks += [data, comp]
            caps += [o.max_compressed_length(codec, len(data)), len(data)]
            expect += [comp if codec != "zstd" else b"", data]  # (the Zstd encoder's bytes are tests/test_gpu_zstd.py's business: here its status)
        comp = ref.compress(data)
        ops += [OP_ENC, OP_DEC, OP_DEC]
        blocks += [data, comp, comp[:-4]]
        caps += [ref.max_compressed_length(len(data)), len(data), len(data)]
        expect += [comp, data, None]
    outs, status, err = g.run(ops, blocks, caps)
    for i, (op, want_bytes) in enumerate(zip(ops, expect)):
        if want_bytes is None:
            assert status[i] == MALFORMED and err[i] == cases.expected(blocks[i], caps[i])[1], i
        else:
            assert status[i] == 0 and (op == 5 or outs[i] == want_bytes), (i, op, status[i])


def test_batch_host(g, encoded, runs):
    inputs, want = encoded
    blocks = [d for _, d in inputs]
    outs, status, _ = g.run_host(OP_ENC, blocks, [ref.max_compressed_length(len(d)) for d in blocks])
    assert status == [0] * len(blocks) and outs == want
    batch = runs[:120]
    outs, status, err = g.run_host(OP_DEC, [b[1] for b in batch], [b[2] for b in batch])
    check(batch, outs, status, err, "achip_batch_host")


def test_differential_fuzz(g, runs):
    """a few thousand items: mutated valid streams against the model's status and offset (both decoders), random and structured plaintexts against the
    model's bytes"""
    rng = random.Random(20261021)
    seeds = [b[1] for b in runs if b[3][0] == "ok" and 8 < len(b[1]) < 2500]
    batch = []
    for k in range(3000):
        s = bytearray(rng.choice(seeds))
        for _ in range(rng.randrange(1, 4)):
            how = rng.randrange(4)
            at = rng.randrange(len(s))
            if how == 0:
                s[at] = rng.getrandbits(8)
            elif how == 1:
                s[at] ^= 1 << rng.randrange(8)
            elif how == 2 and len(s) > 4:
                del s[at:at + rng.randrange(1, 4)]
            else:
                s = s[:max(at, 1)]
        s = bytes(s)
        cap = rng.choice((4096, 600, 70000))
        batch.append(("fuzz %d" % k, s, cap, cases.expected(s, cap)))
    assert 300 < sum(1 for b in batch if b[3][0] == "ok") < 2700  # (both verdicts are well represented)
    for variant in (1, 2):
        g.set_option("lzo.decompress.variant", variant)
        outs, status, err = g.run(OP_DEC, [b[1] for b in batch], [b[2] for b in batch], unaligned=True)
        g.set_option("lzo.decompress.variant", 0)
        check(batch, outs, status, err, "fuzz, variant %d" % variant)
    plain = []
    words = [bytes(rng.getrandbits(8) for _ in range(rng.randrange(1, 12))) for _ in range(40)]
    for k in range(1500):
        n = rng.choice((0, 5, 13, 14, 60, 300, 1500, 5000))
        kind = k % 4
        if kind == 0:
            d = bytes(rng.getrandbits(8) for _ in range(n))
        elif kind == 1:
            d = bytes(rng.choice(b"abc") for _ in range(n))
        elif kind == 2:
            d = b"".join(rng.choice(words) for _ in range(n // 4 + 1))[:n]
        else:
            unit = bytes(rng.getrandbits(8) for _ in range(rng.randrange(1, 40)))
            d = (unit * (n // len(unit) + 1))[:n]
        plain.append(d)
    outs, status, _ = g.run(OP_ENC, plain, [ref.max_compressed_length(len(d)) for d in plain], unaligned=True)
    wrong = [(i, len(d), st) for i, (d, o, st) in enumerate(zip(plain, outs, status)) if st != 0 or o != ref.compress(d)]
    assert not wrong, wrong[:6]
