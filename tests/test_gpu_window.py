"""achip_window_* on the GPU: windows of x-snappy-framed and Hadoop LZ4 / Snappy streams against the model of tests/window_cases.py (the oracle's one-shot readers
and writers and a header-only unit splitter; nothing from the code under test).
  1  every cut      every case stream, every window [a:b] with a at a unit boundary and b at every byte, with and without LAST at the end, three rooms: one batch per format
  2  drive          the standard loop (call, advance by consumed, refill, grow to need) to the end of every case, the streams side by side
  3  writers        plaintexts around the block size handed over in two pieces cut at 40 positions, ample room and room for one block: the one-shot writer's bytes
  4  stream twins   the Python stream classes in small reads and writes; a damaged stream raises behind the bytes in front of the damage
  5  one realistic shape   24 MiB per format at the default buffer size in 4 MiB windows, against the one-shot call on the same data
"""
import io

import numpy as np
import pytest

from tests import common, oracle_lib, window_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


@pytest.fixture(scope="module")
def g():
    from tests.gpu_harness import GpuBatch
    return GpuBatch(0)


@pytest.fixture(scope="module")
def all_cases(o):
    return cases.all_cases(o)


@pytest.fixture(scope="module")
def run(g):
    torch = g.torch
    FILL = 0xA5

    def run(fmt, compress, buffer_size, windows, flags, caps):
        """one achip_window_*_batch call over device buffers -> [result dict]; nothing may be written beyond a window's room"""
        n = len(windows)
        if buffer_size:
            g.set_option("hadoop.buffer_size", buffer_size)
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
        op = (cases.COMPRESS_OP if compress else cases.DECOMPRESS_OP)[fmt]
        call = g.codec.window_compress if compress else g.codec.window_decompress
        call(op, d_flags, d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_dst_cap, d_out_len, d_status, d_err, n, d_consumed, d_stop, d_need)
        g.codec.synchronize()
        out = d_dst.cpu().numpy()
        out_len, status, stop, err, consumed, need = (t.cpu().numpy() for t in (d_out_len, d_status, d_stop, d_err, d_consumed, d_need))
        for i in range(n):
            assert (out[dst_off[i] + caps[i]:dst_off[i] + caps[i] + 8] == FILL).all(), "window %d wrote past its room" % i
        assert (out[max(pos, 16):] == FILL).all(), "wrote past the end of the destination buffer"
        return [{"consumed": int(consumed[i]), "out": out[dst_off[i]:dst_off[i] + max(int(out_len[i]), 0)].tobytes(), "stop": int(stop[i]), "need": int(need[i]),
                 "status": int(status[i]), "err": int(err[i])} for i in range(n)]
    yield run
    g.set_option("hadoop.buffer_size", 262144)


def test_every_cut(run, o, all_cases):
    total, wrong = cases.check_every_cut(run, o, all_cases)
    print("every cut: %d windows, %d wrong" % (total, len(wrong)))
    assert total > 10000 and not wrong, wrong[:10]


def test_drive_to_the_end(run, o, all_cases):
    total, wrong = cases.check_drive(run, o, all_cases)
    print("drive to the end: %d loops, %d wrong" % (total, len(wrong)))
    assert total == 6 * len(all_cases) and not wrong, wrong[:10]


def test_writers(run, o):
    total, wrong = cases.check_writers(run, o)
    print("writers: %d streams, %d wrong" % (total, len(wrong)))
    assert total > 1000 and not wrong, wrong[:10]


TWINS = {"snappyframed": ("SnappyFramedHipInputStream", "SnappyFramedHipOutputStream"), "lz4hadoop": ("Lz4HadoopHipInputStream", "Lz4HadoopHipOutputStream"),
         "snappyhadoop": ("SnappyHadoopHipInputStream", "SnappyHadoopHipOutputStream")}


@pytest.mark.parametrize("fmt", cases.FORMATS)
def test_python_stream_twins(g, o, fmt):
    import aircompressor_amd as A
    reader, writer = (getattr(A, name) for name in TWINS[fmt])
    kw = {"buffer_size": 256} if fmt != "snappyframed" else {}
    plain = b"".join(d for _, d, _ in common.corpus_sample())[:3000] if fmt != "snappyframed" else b"".join(d for _, d, _ in common.corpus_sample())[:150000]
    want = cases.one_shot_compress(o, fmt, plain, kw.get("buffer_size", 0))
    sink = io.BytesIO()
    w = writer(sink, native_ctx=g.codec.native, window_bytes=1000 if fmt != "snappyframed" else 70000, **kw)
    for i in range(0, len(plain), 13 if fmt != "snappyframed" else 1300):
        w.write(plain[i:i + (13 if fmt != "snappyframed" else 1300)])
    w.finish()
    w.close()
    assert sink.getvalue() == want
    r = reader(io.BytesIO(want), native_ctx=g.codec.native, window_bytes=300 if fmt != "snappyframed" else 40000, **kw)
    got = b""
    while True:
        piece = r.read(7 if fmt != "snappyframed" else 700)
        if not piece:
            break
        got += piece
    assert got == plain
    assert reader(io.BytesIO(want), native_ctx=g.codec.native, **kw).readall() == plain
    # a damaged stream: the bytes in front of the damage, then the exception
    damaged = bytearray(want)
    model = cases.Model(o)
    if fmt == "snappyframed":
        damaged[len(want) * 2 // 3] ^= 0x40
    else:  # a chunk length far beyond the stream, two thirds in
        units = cases.split(model, fmt, want, True)
        at = units[len(units) * 2 // 3].start + 4
        damaged[at:at + 4] = b"\x7f\xff\xff\xf0"
    before = cases.expect(model, fmt, kw.get("buffer_size", 0), bytes(damaged), cases.FIRST | cases.LAST, 1 << 20)
    assert before["status"] != 0 and 0 < len(before["out"]) < len(plain)
    r = reader(io.BytesIO(bytes(damaged)), native_ctx=g.codec.native, window_bytes=300 if fmt != "snappyframed" else 40000, **kw)
    got = b""
    with pytest.raises(A.MalformedInputException):
        while True:
            piece = r.read(7 if fmt != "snappyframed" else 700)
            assert piece, "the stream ended without its error"
            got += piece
    assert got == before["out"]


@pytest.mark.parametrize("fmt", cases.FORMATS)
def test_one_realistic_shape(g, o, fmt):
    """24 MiB at the default buffer size in 4 MiB windows: the windows' results, one behind the other, are the one-shot call's on the same data -- and the oracle's"""
    g.set_option("hadoop.buffer_size", 262144)
    text = b"".join(d for _, d, _ in common.corpus_sample())
    plain = (text * (24 * 1048576 // len(text) + 1))[:24 * 1048576]
    stream = cases.one_shot_compress(o, fmt, plain, 262144)
    window = 4 << 20
    # one-shot, on the GPU
    outs, status, _ = g.run(cases.DECOMPRESS_OP[fmt], [stream], [len(plain)])
    assert status == [0] and outs[0] == plain
    bound = {"snappyframed": lambda n: int(g.codec.lib.achip_snappyframed_max_compressed_length(n))}.get(fmt, lambda n: o.hadoop_max_compressed_length(cases.codec_of(fmt), n, 262144))
    outs, status, _ = g.run(cases.COMPRESS_OP[fmt], [plain], [bound(len(plain))])
    assert status == [0] and outs[0] == stream
    # the reader in 4 MiB windows
    pos, got, first, calls = 0, [], True, 0
    while True:
        w = stream[pos:pos + window]
        last = pos + len(w) == len(stream)
        consumed, out, stop, need, st, _ = g.codec.window_host(cases.DECOMPRESS_OP[fmt], (cases.FIRST if first else 0) | (cases.LAST if last else 0), w, 16 << 20)
        calls += 1
        assert st == 0 and stop != cases.FAILED and (consumed > window // 2 or last), (stop, consumed, need)
        got.append(out)
        pos += consumed
        first = False
        if last and stop == cases.END:
            break
    assert b"".join(got) == plain and calls <= len(stream) // (window // 2) + 2
    # the writer in 4 MiB windows
    held, got, first, pos = b"", [], True, 0
    while pos < len(plain) or held:
        held += plain[pos:pos + window]
        pos = min(pos + window, len(plain))
        closing = pos == len(plain)
        consumed, out, stop, need, st, _ = g.codec.window_host(cases.COMPRESS_OP[fmt], (cases.FIRST if first else 0) | (cases.LAST if closing else 0), held, 2 * window + 65536,
                                                                compress=True)
        assert st == 0 and stop in (cases.END, cases.NEED_INPUT), (stop, need)
        got.append(out)
        held = held[consumed:]
        first = False
    assert b"".join(got) == stream
