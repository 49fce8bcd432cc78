"""The x-snappy-framed streams with the constructor arguments of their reference classes on the GPU, through the C ABI (achip_ctx_set_snappyframed_writer,
achip_ctx_set_snappyframed_verify_checksums): bytes, lengths, statuses and offsets against the pure-Python model (tests/snf_params_ref.py, pinned by
tests/golden/snf_params_vectors.json and by the oracle at the defaults).  Inputs: tests/snf_params_cases.py -- the smallest shapes at which each mechanism can go
wrong, all of a parameter set's streams in one batch.
  writers   the catalog and the pairs at the ratio's edge through both writer variants; a batch whose blocks overflow the list (the serial kernel inside one call)
  windows   the window writer across cuts, with ample room and with room for one block
  bounds    achip_compress_bound_batch against achip_snappyframed_max_compressed_length_for; a capacity a byte short
  scope     mixed batches, achip_batch_host, a second context at the defaults, what the parameters leave alone
  readers   checksum-free streams, a damaged CRC field and structural damage with verify on and off, every reader variant and the window reader
"""
import io
import math

import numpy as np
import pytest

from tests import oracle_lib, snf_params_cases as cases, snf_params_ref as ref, window_cases
from tests.gpu_harness import GpuBatch

pytestmark = pytest.mark.gpu

SNAPPY_C, SNF_D, SNF_C, SNAPPYHADOOP_C, LZ4_C = 3, 8, 9, 13, 1
BAD_ARGUMENT = -(3 + 16 * 102)  # INVALID_ARGUMENT / ACHIP_D_BAD_ARGUMENT


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


@pytest.fixture(scope="module")
def gpu():
    return GpuBatch()


@pytest.fixture
def g(gpu):
    """the module's context with everything these tests touch at its default, before and after"""
    def reset():
        gpu.set_option("snappyframed.compress.variant", 1)
        gpu.set_option("snappyframed.decompress.variant", 3)
        gpu.codec.native.set_snappyframed_writer(*ref.DEFAULT_PARAMS)
        gpu.codec.native.set_snappyframed_verify_checksums(True)
    reset()
    yield gpu
    reset()


def bound(g, n, block_size):
    return g.codec.lib.achip_snappyframed_max_compressed_length_for(n, block_size)


def configure(g, params, variant=None):
    if variant is not None:
        g.set_option("snappyframed.compress.variant", variant)
    g.codec.native.set_snappyframed_writer(*params)
    assert g.codec.native.get_snappyframed_writer() == (bool(params[0]), params[1], params[2])


def encode_and_check(g, params, named, want, what):
    """one batch through achip_snappyframed_compress_batch at exact capacities: outputs, lengths, statuses, offsets; then the GPU reader on every output"""
    block_size = params[1]
    outs, status, err = g.run(SNF_C, [d for _, d in named], [bound(g, len(d), block_size) for _, d in named], unaligned=True)
    assert status == [0] * len(named) and err == [0] * len(named), what
    for (name, _), c, w in zip(named, outs, want):
        assert len(c) == len(w) and c == w, (what, name, len(c), len(w))
    g.codec.native.set_snappyframed_verify_checksums(bool(params[0]))  # (a checksum-free stream does not verify)
    back, status, _ = g.run(SNF_D, outs, [len(d) for _, d in named])
    assert status == [0] * len(named) and all(b == d for b, (_, d) in zip(back, named)), what


@pytest.mark.parametrize("block_size", cases.BLOCK_SIZES)
@pytest.mark.parametrize("variant", (0, 1))
def test_writers_give_the_models_bytes(g, variant, block_size):
    named = cases.inputs(block_size)
    for params in cases.parameter_sets():
        if params[1] == block_size:
            configure(g, params, variant)
            encode_and_check(g, params, named, [cases.expected(params, name) for name, _ in named], (variant, cases.params_name(params)))


@pytest.mark.parametrize("variant", (0, 1))
def test_the_division_is_javas_at_the_ratios_edge(g, variant):
    """a block the oracle compresses from l to c bytes: kept at c / l, stored at the double below it"""
    pairs = cases.edge_pairs()
    assert len(pairs) >= 3
    for name, block_size, data, kept, raw in pairs:
        for ratio, flag in ((kept, ref.COMPRESSED_DATA_FLAG), (raw, ref.UNCOMPRESSED_DATA_FLAG)):
            params = (True, block_size, ratio)
            configure(g, params, variant)
            want = ref.compress(data, *params)
            assert want[10] == flag
            encode_and_check(g, params, [(name, data)], [want], (variant, name, ratio))


def test_a_batch_whose_blocks_overflow_the_list(g):
    """1 024 streams of 1 025 bytes at block size 1: 1 049 600 blocks against 2^20 list entries -- the streams at the end take the serial kernel inside the same call"""
    streams = cases.overflow_streams()
    block_size = cases.OVERFLOW_BLOCK_SIZE
    assert len(streams) * cases.OVERFLOW_LENGTH > 1 << 20
    for params in ((True, block_size, 0.85), (False, block_size, 1.0)):
        configure(g, params, 1)
        want = [ref.compress(d, *params) for d in streams[:4]]
        outs, status, err = g.run(SNF_C, streams, [bound(g, cases.OVERFLOW_LENGTH, block_size)] * len(streams), unaligned=True)
        assert status == [0] * len(streams) and err == [0] * len(streams)
        wrong = [i for i, c in enumerate(outs) if c != want[i % 4]]
        assert not wrong, (params, wrong[:10], len(wrong))


WINDOW_PARAMS = ((True, 63, 0.85), (False, 64, 0.5), (True, 1, 0.85), (True, 2, 1.0), (True, 4096, 0.5), (False, 65535, 0.85), (True, 65536, 1.0))


def window_run(g, compress):
    """-> run(fmt, compress, buffer_size, windows, flags, caps): one achip_window_*_batch call over device buffers; nothing may be written beyond a window's room"""
    torch = g.torch
    FILL = 0xA5

    def run(_fmt, _compress, _buffer_size, windows, flags, caps):
        n = len(windows)
        src, src_off, src_len = g.pack(windows, align=1)
        caps = np.asarray(caps, dtype=np.int32)
        dst_off = np.zeros(n, dtype=np.int64)
        pos = 0
        for i, c in enumerate(caps):
            dst_off[i] = pos
            pos += int(c) + 8
        to = lambda a: torch.from_numpy(a).to(g.dev)  # noqa: E731
        d_src, d_src_off, d_src_len, d_dst_off, d_dst_cap, d_flags = to(src), to(src_off), to(src_len), to(dst_off), to(caps), to(np.asarray(flags, dtype=np.int32))
        d_dst = torch.full((max(pos, 16) + 64,), FILL, dtype=torch.uint8, device=g.dev)
        i32 = lambda: torch.full((n,), -7, dtype=torch.int32, device=g.dev)  # noqa: E731
        i64 = lambda: torch.full((n,), -7, dtype=torch.int64, device=g.dev)  # noqa: E731
        d_out_len, d_status, d_stop, d_err, d_consumed, d_need = i32(), i32(), i32(), i64(), i64(), i64()
        torch.cuda.synchronize()
        call = g.codec.window_compress if compress else g.codec.window_decompress
        call(SNF_C if compress else SNF_D, d_flags, d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_out_len, d_status, d_err, n, d_consumed, d_stop, d_need)
        g.codec.synchronize()
        out = d_dst.cpu().numpy()
        out_len, status, stop, err, consumed, need = (t.cpu().numpy() for t in (d_out_len, d_status, d_stop, d_err, d_consumed, d_need))
        for i in range(n):
            assert (out[dst_off[i] + caps[i]:dst_off[i] + caps[i] + 8] == FILL).all(), "window %d wrote past its room" % i
        assert (out[max(pos, 16):] == FILL).all(), "wrote past the end of the destination buffer"
        return [{"consumed": int(consumed[i]), "out": out[dst_off[i]:dst_off[i] + max(int(out_len[i]), 0)].tobytes(), "stop": int(stop[i]), "need": int(need[i]),
                 "status": int(status[i]), "err": int(err[i])} for i in range(n)]
    return run


@pytest.mark.parametrize("params", WINDOW_PARAMS, ids=cases.params_name)
def test_the_window_writer_across_cuts(g, params):
    """every stream handed over in two pieces at each cut, with ample room and with room for one block (8 + blockSize + 10): the pieces, one behind the other, are
    the one-shot bytes at the same parameters; a partial block asks for need = blockSize (window_cases.write_stream asserts it)"""
    block_size = params[1]
    configure(g, params)
    loops, what = [], []
    for name, plain in cases.inputs(block_size):
        if name.startswith("random") and len(plain) > block_size + 1:
            continue
        for room in (2 * ref.max_compressed_length(len(plain), block_size) + 64, 8 + block_size + 10):
            for cut in cases.cut_positions(len(plain), block_size):
                loops.append(window_cases.write_stream(plain, cut, room, block_size))
                what.append((name, cut, room))
    assert len(loops) > 50
    results = window_cases.lockstep(window_run(g, True), "snappyframed", True, 0, loops)
    want = dict((name, ref.compress(plain, *params)) for name, plain in cases.inputs(block_size))
    wrong = [(name, cut, room) for (name, cut, room), got in zip(what, results) if got != want[name]]
    assert not wrong, wrong[:10]


def test_window_plan_counts_in_blocks_of_the_block_size(g):
    """consumed, need and the worst-case room at block size 100: full blocks only without LAST, need = blockSize on the partial block, need = 8 + blockSize (+ 10
    where the stream identifier does not fit either) on want of room"""
    params = (True, 100, 0.85)
    configure(g, params)
    run = window_run(g, True)
    plain = cases.data("text", 350)
    FIRST, LAST = window_cases.FIRST, window_cases.LAST
    NEED_INPUT, NEED_ROOM, END = window_cases.NEED_INPUT, window_cases.NEED_ROOM, window_cases.END
    r = run(None, True, 0, [plain, plain, plain, plain[:100], plain[:100], plain], [FIRST, FIRST, 0, FIRST, 0, FIRST | LAST], [4000, 10 + 108 + 107, 107, 9, 108, 4000])
    whole = ref.compress(plain, *params)
    first_three = ref.compress(plain[:300], *params)
    assert (r[0]["consumed"], r[0]["stop"], r[0]["need"], r[0]["out"]) == (300, NEED_INPUT, 100, first_three)
    assert (r[1]["consumed"], r[1]["stop"], r[1]["need"]) == (100, NEED_ROOM, 108) and r[1]["out"] == ref.compress(plain[:100], *params)
    assert (r[2]["consumed"], r[2]["stop"], r[2]["need"], r[2]["out"]) == (0, NEED_ROOM, 108, b"")
    assert (r[3]["consumed"], r[3]["stop"], r[3]["need"], r[3]["out"]) == (0, NEED_ROOM, 118, b"")
    assert (r[4]["consumed"], r[4]["stop"], r[4]["need"]) == (100, END, 0) and r[4]["out"] == ref.compress(plain[:100], *params)[10:]
    assert (r[5]["consumed"], r[5]["stop"], r[5]["out"]) == (350, END, whole)
    assert all(x["status"] == 0 for x in r)


def test_windows_with_more_blocks_than_the_list_has_entries(g):
    """128 windows of 70 000 bytes at block size 4: 2 240 000 blocks against 2^20 list entries.  Every window takes its share (2^20 / 128 = 8 192 blocks) and stops
    with NEED_ROOM, need 0; the loop calls again and the pieces are the one-shot bytes -- no window fails.  (Four different plaintexts in turn: the model runs 17 500
    blocks four times.)"""
    params = (True, 4, 0.85)
    configure(g, params)
    kinds = [cases.data("text", 70000, 10), cases.data("run", 70000, 4), cases.data("random", 70000, 2), cases.data("text", 70000, 123456)]
    plains = [kinds[i % 4] for i in range(128)]
    want = [ref.compress(d, *params) for d in kinds]
    run = window_run(g, True)
    room = 2 * ref.max_compressed_length(70000, 4)
    first = run(None, True, 0, plains, [window_cases.FIRST] * 128, [room] * 128)
    assert all((r["status"], r["stop"], r["need"], r["consumed"]) == (0, window_cases.NEED_ROOM, 0, 8192 * 4) for r in first), first[0]
    assert all(r["out"] == want[i % 4][:len(r["out"])] and len(r["out"]) > 8192 * 4 for i, r in enumerate(first))
    results = window_cases.lockstep(run, "snappyframed", True, 0, [window_cases.write_stream(d, len(d), room, 4) for d in plains])
    wrong = [i for i, got in enumerate(results) if got != want[i % 4]]
    assert not wrong, wrong[:10]


def test_compress_bound_batch_uses_the_contexts_block_size(g):
    torch = g.torch
    lengths = np.array([0, 1, 62, 63, 64, 4095, 4096, 4097, 65535, 65536, 65537, 1000003, 1 << 28, 1 << 30, 0x7FFFFFFF, -1], dtype=np.int32)
    for block_size in (1, 63, 4096, 65536):
        configure(g, (True, block_size, 0.85))
        d_len = torch.from_numpy(lengths).to(g.dev)
        d_size = torch.full((len(lengths),), -7, dtype=torch.int64, device=g.dev)
        d_status = torch.full((len(lengths),), -7, dtype=torch.int32, device=g.dev)
        g.codec.compress_bounds(SNF_C, d_len, d_size, d_status, len(lengths))
        g.codec.synchronize()
        for n, size, st in zip(lengths.tolist(), d_size.cpu().tolist(), d_status.cpu().tolist()):
            want = bound(g, n, block_size)
            if want < 0:
                assert (size, st) == (0, BAD_ARGUMENT), (block_size, n)
                assert n < 0 or ref.max_compressed_length(n, block_size) > 0x7FFFFFFF
            else:
                assert (size, st) == (want, 0) and want == ref.max_compressed_length(n, block_size), (block_size, n)
        # the other ops' lines do not move
        d_size2 = torch.full((len(lengths),), -7, dtype=torch.int64, device=g.dev)
        g.codec.compress_bounds(SNAPPY_C, d_len, d_size2, d_status, len(lengths))
        g.codec.synchronize()
        assert d_size2.cpu().tolist()[:6] == [32 + n + n // 6 for n in lengths.tolist()[:6]]
    assert bound(g, 1 << 30, 1) < 0 < bound(g, 1 << 30, 65536)


@pytest.mark.parametrize("variant", (0, 1))
def test_a_capacity_below_the_bound_is_refused(g, variant):
    """the kernels' ACHIP_D_SNF_MAX_OUTPUT check asks for the bound at the context's block size: what was enough at 64 KiB is a byte short at 4096"""
    data = cases.data("text", 3 * 4096 + 7)
    params = (True, 4096, 0.85)
    configure(g, params, variant)
    enough, default_bound = bound(g, len(data), 4096), g.codec.lib.achip_snappyframed_max_compressed_length(len(data))
    assert enough == default_bound + 8 * 3
    outs, status, err = g.run(SNF_C, [data, data, data], [enough, enough - 1, default_bound])
    assert status == [0, cases.MAX_OUTPUT, cases.MAX_OUTPUT] and err == [0, 0, 0]
    assert outs == [ref.compress(data, *params), b"", b""]


def test_mixed_batches_and_batch_host_honour_the_contexts_parameters(g, o):
    plain = GpuBatch()  # a second context, at the defaults: two contexts hold different values side by side
    params = (False, 4096, 0.5)
    configure(g, params)
    g.codec.native.set_snappyframed_verify_checksums(False)
    assert plain.codec.native.get_snappyframed_writer() == ref.DEFAULT_PARAMS and plain.codec.native.get_snappyframed_verify_checksums() is True
    lib = g.codec.lib
    text, other = cases.data("text", 30000, 5), cases.data("text", 70000, 777)
    free = ref.compress(text, False, 4096, 0.85)  # a checksum-free stream: only a reader that does not verify can read it
    items = [(SNF_C, text, bound(g, len(text), 4096)), (SNAPPY_C, text, lib.achip_snappy_max_compressed_length(len(text))),
             (SNAPPYHADOOP_C, text, lib.achip_hadoop_max_compressed_length(1, len(text), 262144)), (SNF_D, free, len(text)),
             (LZ4_C, text, lib.achip_lz4_max_compressed_length(len(text))), (SNF_C, other, bound(g, len(other), 4096))]
    ops, blocks, caps = [i[0] for i in items], [i[1] for i in items], [i[2] for i in items]
    for run in ("run", "run_host"):  # achip_mixed_batch, achip_mixed_batch_host
        mine, st_mine, err_mine = getattr(g, run)(ops, blocks, caps)
        theirs, st_theirs, err_theirs = getattr(plain, run)(ops, blocks, caps)
        assert st_mine == [0] * len(items), run
        assert mine[0] == ref.compress(text, *params) and mine[5] == ref.compress(other, *params) and mine[3] == text, run
        # the context at the defaults still writes today's bytes, and refuses the checksum-free stream at its first chunk
        assert st_theirs == [0, 0, 0, cases.CHECKSUM, 0, 0] and err_theirs[3] == 10, run
        assert theirs[0] == o.compress("snappyframed", text) and theirs[5] == o.compress("snappyframed", other), run
        assert mine[0] != theirs[0]
        # raw Snappy, the Hadoop Snappy writer and LZ4 do not know the parameters
        assert [mine[i] for i in (1, 2, 4)] == [theirs[i] for i in (1, 2, 4)] and mine[1] == o.compress("snappy", text), run
    # achip_batch_host
    outs, status, _ = g.run_host(SNF_C, [text, other], [caps[0], caps[5]])
    assert status == [0, 0] and outs == [ref.compress(text, *params), ref.compress(other, *params)]
    outs, status, _ = g.run_host(SNF_D, [free], [len(text)])
    assert status == [0] and outs == [text]
    outs, status, err = plain.run_host(SNF_D, [free], [len(text)])
    assert status == [cases.CHECKSUM] and err == [10]
    # the Hadoop Snappy writer in window form writes what it writes at the defaults
    A = g.A
    both = A.native.WINDOW_FIRST | A.native.WINDOW_LAST
    assert g.codec.window_host(A.OP_SNAPPYHADOOP_COMPRESS, both, text, caps[2], compress=True) == plain.codec.window_host(A.OP_SNAPPYHADOOP_COMPRESS, both, text, caps[2], compress=True)
    # the window writer of the context at the defaults: today's bytes
    assert plain.codec.window_host(A.OP_SNAPPYFRAMED_COMPRESS, both, text, 2 * len(text), compress=True)[1] == o.compress("snappyframed", text)
    assert g.codec.window_host(A.OP_SNAPPYFRAMED_COMPRESS, both, text, 2 * len(text), compress=True)[1] == ref.compress(text, *params)


def test_multi_batch_host_each_context_its_own_parameters(g, o):
    plain = GpuBatch()
    params = (True, 63, 1.0)
    configure(g, params)
    multi = g.A.HipMultiContextCodec(contexts=[g.codec.native, plain.codec.native])
    text = cases.data("text", 60000, 31)
    blocks = [text[k * 4000:(k + 1) * 4000 + 2000] for k in range(10)]
    src, src_off, src_len = g.pack(blocks, align=1)
    caps = np.array([bound(g, len(b), 63) for b in blocks], dtype=np.int32)
    dst_off = np.concatenate([[0], np.cumsum(caps[:-1])]).astype(np.int64)
    dst = np.zeros(int(caps.sum()) + 16, dtype=np.uint8)
    out_len, status, _ = multi.run_host(SNF_C, src, src_off, src_len, dst, dst_off, caps)
    assert status.tolist() == [0] * len(blocks)
    starts = multi.slice_starts.tolist()
    assert starts[0] == 0 and starts[2] == len(blocks) and 0 < starts[1] < len(blocks)
    for i, b in enumerate(blocks):
        want = ref.compress(b, *params) if i < starts[1] else o.compress("snappyframed", b)
        assert dst[dst_off[i]:dst_off[i] + out_len[i]].tobytes() == want, i


@pytest.mark.parametrize("variant", (0, 1, 2, 3))
def test_readers_with_and_without_verification(g, variant):
    """checksum-free streams and one damaged CRC field fail with ACHIP_D_SNF_CHECKSUM at the chunk's position with verify on and decode with verify off; structural
    damage reports the same status and offset under both settings"""
    streams = cases.reader_streams()
    g.set_option("snappyframed.decompress.variant", variant)
    for verify in (True, False):
        g.codec.native.set_snappyframed_verify_checksums(verify)
        assert g.codec.native.get_snappyframed_verify_checksums() is verify
        outs, status, err = g.run(SNF_D, [s for _, s, *_ in streams], [len(p) + 9 if p is not None else 20000 for _, _, p, *_ in streams], unaligned=True)
        for (name, _, plain, st_on, eo_on, st_off, eo_off), got, st, eo in zip(streams, outs, status, err):
            want_st, want_eo = (st_on, eo_on) if verify else (st_off, eo_off)
            assert (st, eo) == (want_st, want_eo), (variant, verify, name)
            assert got == (plain if want_st == 0 else b""), (variant, verify, name)
    assert any(s[3] == cases.CHECKSUM for s in streams) and any(s[3] != 0 and s[3] == s[5] for s in streams)


@pytest.mark.parametrize("variant", (1, 2, 3))
def test_the_window_reader_with_and_without_verification(g, variant):
    streams = cases.reader_streams()
    g.set_option("snappyframed.decompress.variant", variant)
    FIRST, LAST, FAILED, END = window_cases.FIRST, window_cases.LAST, window_cases.FAILED, window_cases.END
    run = window_run(g, False)
    for verify in (True, False):
        g.codec.native.set_snappyframed_verify_checksums(verify)
        got = run(None, False, 0, [s for _, s, *_ in streams], [FIRST | LAST] * len(streams), [len(p) + 9 if p is not None else 20000 for _, _, p, *_ in streams])
        for (name, stream, plain, st_on, eo_on, st_off, eo_off), r in zip(streams, got):
            want_st, want_eo = (st_on, eo_on) if verify else (st_off, eo_off)
            assert r["status"] == want_st, (variant, verify, name, r["status"])
            if want_st == 0:
                assert (r["stop"], r["consumed"], r["out"]) == (END, len(stream), plain), (variant, verify, name)
            else:
                assert (r["stop"], r["err"]) == (FAILED, want_eo), (variant, verify, name)
            if want_st == cases.CHECKSUM:  # a window delivers what lies in front of the chunk that failed
                assert r["consumed"] == want_eo and r["out"] == ref.decompress(stream[:want_eo], verify_checksums=False), (variant, verify, name)
    # a checksum-free stream in windows of a chunk and a bit, verify off: the plaintext
    name, stream, plain = streams[4][:3]
    assert name == "checksum-free"
    pos, out, first = 0, b"", True
    while pos < len(stream):
        w = stream[pos:pos + 5000]
        last = pos + len(w) == len(stream)
        r = run(None, False, 0, [w], [(FIRST if first else 0) | (LAST if last else 0)], [20000])[0]
        assert r["status"] == 0 and (r["consumed"] > 0 or last)
        out += r["out"]
        pos += r["consumed"]
        first = False
        if last:
            break
    assert out == plain


def test_setters_on_a_live_context(g):
    A, n = g.A, g.codec.native
    assert n.get_snappyframed_writer() == (True, 65536, 0.85) and n.get_snappyframed_verify_checksums() is True  # the defaults
    edge = math.nextafter(0.5, 0.0)
    n.set_snappyframed_writer(False, 4096, edge)
    assert n.get_snappyframed_writer() == (False, 4096, edge)
    for bad, text in (((True, 0, 1.5), "minCompressionRatio 1.5 must be between (0,1.0]."), ((True, 100, float("nan")), "minCompressionRatio NaN must be between (0,1.0]."),
                      ((True, 0, 0.85), "blockSize must be in (0, 65536]"), ((True, 65537, 1.0), "blockSize must be in (0, 65536]")):
        with pytest.raises(A.IllegalArgumentException) as e:
            n.set_snappyframed_writer(*bad)
        assert str(e.value) == text
        assert n.get_snappyframed_writer() == (False, 4096, edge)  # a refused set keeps every value
    lib = g.codec.lib
    assert lib.achip_ctx_set_snappyframed_writer(n.ctx, 2, 63, ref.ratio_bits(1.0)) == BAD_ARGUMENT and n.get_snappyframed_writer() == (False, 4096, edge)
    n.set_snappyframed_verify_checksums(False)
    assert lib.achip_ctx_set_snappyframed_verify_checksums(n.ctx, 2) == BAD_ARGUMENT and n.get_snappyframed_verify_checksums() is False
    n.set_snappyframed_writer(True, 65536, ref.SMALLEST_RATIO)
    assert n.get_snappyframed_writer() == (True, 65536, ref.SMALLEST_RATIO)


def test_python_classes_take_the_arguments(g, o):
    A = g.A
    text = cases.data("text", 20000, 9)
    src = np.frombuffer(text, dtype=np.uint8)
    for params in ((True, 65536, 0.85), (False, 4096, 0.5), (True, 63, 1.0)):
        c = A.SnappyFramedHipCompressor(native_ctx=g.codec.native, write_checksums=params[0], block_size=params[1], min_compression_ratio=params[2])
        assert c.max_compressed_length(len(text)) == ref.max_compressed_length(len(text), params[1])
        out = np.zeros(c.max_compressed_length(len(text)), dtype=np.uint8)
        stream = out[:c.compress_segment(src, out)].tobytes()
        assert stream == ref.compress(text, *params)
        back = np.zeros(len(text), dtype=np.uint8)
        d = A.SnappyFramedHipDecompressor(native_ctx=g.codec.native, verify_checksums=params[0])  # (the same context: each object brings its own values)
        assert d.decompress_segment(np.frombuffer(stream, dtype=np.uint8), back) == len(text) and back.tobytes() == text
        if not params[0]:
            with pytest.raises(A.MalformedInputException):
                A.SnappyFramedHipDecompressor(native_ctx=g.codec.native).decompress_segment(np.frombuffer(stream, dtype=np.uint8), back)
        # the stream twins
        sink = io.BytesIO()
        w = A.SnappyFramedHipOutputStream(sink, native_ctx=g.codec.native, window_bytes=3000, write_checksums=params[0], block_size=params[1], min_compression_ratio=params[2])
        for i in range(0, len(text), 1300):
            w.write(text[i:i + 1300])
        w.close()
        assert sink.getvalue() == stream
        assert A.SnappyFramedHipInputStream(io.BytesIO(stream), native_ctx=g.codec.native, window_bytes=5000, verify_checksums=params[0]).readall() == text
    free = A.SnappyFramedHipCompressor.new_checksum_free_benchmark_compressor(native_ctx=g.codec.native)
    out = np.zeros(free.max_compressed_length(len(text)), dtype=np.uint8)
    assert out[:free.compress_segment(src, out)].tobytes() == ref.compress(text, False, 65536, 0.85)
    plain = A.SnappyFramedHipCompressor(native_ctx=g.codec.native)
    assert (plain.write_checksums, plain.block_size, plain.min_compression_ratio) == ref.DEFAULT_PARAMS
    assert out[:plain.compress_segment(src, out)].tobytes() == o.compress("snappyframed", text)
