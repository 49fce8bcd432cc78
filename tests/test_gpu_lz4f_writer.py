"""The LZ4 frame writer with the frame settings of achip_ctx_set_lz4frame_writer on the GPU, through the C ABI: bytes, lengths and statuses against the
pure-Python model (tests/lz4f_writer_ref.py, held to the oracle by tests/test_lz4f_writer_ref.py).  Inputs: tests/lz4f_writer_cases.py, a setting's cases in one batch
of 300 items -- empty and large frames side by side, sources and destinations at the four misalignments, canaries around every destination.
  writer      the catalog at exact capacities; a capacity a byte short; accelerations 1, 7 and 65537; the block list at the Java writer's settings
  entry points the batch call, the single-buffer call, achip_batch_host, the mixed batch in both forms
  readers     every frame back through the GPU reader (checksums verified) at lz4frame.decompress.variant 0 and the default; with a content size, sized and
              planned on the device
  bounds      achip_compress_bound_batch follows the settings
"""
import numpy as np
import pytest

from tests import lz4f_writer_cases as cases, lz4f_writer_ref as ref, oracle_lib
from tests.gpu_harness import GpuBatch

pytestmark = pytest.mark.gpu

LZ4_C, LZ4F_D, LZ4F_C, SNAPPY_C = 1, 6, 7, 3
ITEMS = 300
FILL = 0xA5


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
        gpu.set_option("lz4frame.compress.variant", 0)
        gpu.set_option("lz4frame.decompress.variant", 2)
        gpu.codec.native.set_lz4frame_writer(*ref.DEFAULT)
        gpu.codec.native.set_lz4_acceleration(1)
    reset()
    yield gpu
    reset()


def configure(g, settings, acceleration=1, variant=0):
    g.set_option("lz4frame.compress.variant", variant)
    g.codec.native.set_lz4frame_writer(*settings)
    g.codec.native.set_lz4_acceleration(acceleration)
    assert g.codec.native.get_lz4frame_writer() == (settings[0], bool(settings[1]), bool(settings[2]), bool(settings[3]))


def place(lengths, misalign, lead=48, gap=32):
    """offsets 16 k + misalign(i), with at least `gap` bytes between an item's end and the next item"""
    off = np.zeros(len(lengths), dtype=np.int64)
    pos = lead
    for i, n in enumerate(lengths):
        pos = (pos + 15) // 16 * 16 + misalign(i)
        off[i] = pos
        pos += int(n) + gap
    return off, pos + 64


def write(g, items, caps, op=LZ4F_C):
    """one launch over device buffers: item i at source misalignment i % 4 and destination misalignment (i // 4) % 4 beyond a 16-byte boundary -> (outputs, statuses,
    offsets).  Nothing but an item's own capacity may have changed, and an item with a status must have left even that untouched."""
    torch = g.torch
    n = len(items)
    src_len = np.array([len(d) for d in items], dtype=np.int32)
    caps = np.asarray(caps, dtype=np.int32)
    src_off, src_end = place(src_len, lambda i: cases.MISALIGNMENTS[i % 4])
    dst_off, dst_end = place(caps, lambda i: cases.MISALIGNMENTS[(i // 4) % 4])
    src = np.full(src_end, 0x5A, dtype=np.uint8)
    for off, d in zip(src_off, items):
        src[off:off + len(d)] = np.frombuffer(d, dtype=np.uint8)
    to = lambda a: torch.from_numpy(a).to(g.dev)  # noqa: E731
    d_src, d_src_off, d_src_len, d_dst_off, d_cap = to(src), to(src_off), to(src_len), to(dst_off), to(caps)
    d_dst = torch.full((dst_end,), FILL, dtype=torch.uint8, device=g.dev)
    d_out_len, d_status = (torch.full((n,), -7, dtype=torch.int32, device=g.dev) for _ in range(2))
    d_err = torch.full((n,), -7, dtype=torch.int64, device=g.dev)
    torch.cuda.synchronize()
    if isinstance(op, list):
        g.codec.launch_mixed(op, d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_cap, d_out_len, d_status, d_err, n)
    else:
        g.codec.launch(op, d_src, d_src_off, d_src_len, d_dst, d_dst_off, d_cap, d_out_len, d_status, d_err, n)
    g.codec.synchronize()
    out, out_len, status, err = d_dst.cpu().numpy(), d_out_len.cpu().numpy(), d_status.cpu().numpy(), d_err.cpu().numpy()
    mask = np.ones(dst_end, dtype=bool)  # the canaries: everything outside the capacities of the items that were written
    for i in range(n):
        if status[i] == 0:
            mask[dst_off[i]:dst_off[i] + caps[i]] = False
    touched = np.nonzero(mask & (out != FILL))[0]
    assert touched.size == 0, "bytes outside the written items' capacities changed, first at %d" % touched[0]
    return [out[dst_off[i]:dst_off[i] + max(int(out_len[i]), 0)].tobytes() for i in range(n)], status.tolist(), err.tolist()


def batch_of(settings):
    """-> [(name, data)]: the setting's cases, 300 items in all.  At 64 KiB the cases in turn; at the large sizes the three cases once (up to 4 MiB each) among
    the empty and short frames of the 64 KiB inputs, which at a large block size are frames of one block or none."""
    cs = cases.by_settings()[settings]
    named = [(c.name, c.data) for c in cs]
    if settings[0] == 65536:
        return [named[i % len(named)] for i in range(ITEMS)]
    small = [("%s %d" % (kind, n), cases.data(kind, n, 7 * n)) for kind, n in cases.inputs_64k() if n <= 65537]
    filler = [small[i % len(small)] for i in range(ITEMS - len(named))]
    return filler[:100] + named[:1] + filler[100:200] + named[1:] + filler[200:]


_want = {}


def want_for(settings, named, acceleration=1):
    out = []
    for name, d in named:
        key = (settings, name, acceleration)
        if key not in _want:
            _want[key] = ref.compress(d, *settings, acceleration=acceleration)
        out.append(_want[key])
    return out


def read_back(g, frames, plains, what):
    for variant in (0, 2):
        g.set_option("lz4frame.decompress.variant", variant)
        back, status, err = g.run(LZ4F_D, frames, [len(d) for d in plains])
        assert status == [0] * len(frames) and err == [0] * len(frames), (what, variant)
        assert all(b == d for b, d in zip(back, plains)), (what, variant)


SETTINGS = list(cases.by_settings())


@pytest.mark.parametrize("settings", SETTINGS, ids=cases.settings_name)
def test_the_catalog_in_one_batch(g, settings):
    named = batch_of(settings)
    assert len(named) == ITEMS and min(len(d) for _, d in named) == 0 and max(len(d) for _, d in named) > settings[0]
    configure(g, settings)
    want = want_for(settings, named)
    caps = [ref.max_compressed_length(len(d), *settings) for _, d in named]
    outs, status, err = write(g, [d for _, d in named], caps)
    assert status == [0] * ITEMS and err == [0] * ITEMS
    wrong = [(i, name, len(c), len(w)) for i, ((name, _), c, w) in enumerate(zip(named, outs, want)) if c != w]
    assert not wrong, wrong[:10]
    read_back(g, outs, [d for _, d in named], cases.settings_name(settings))


@pytest.mark.parametrize("settings", [(65536, 1, 1, 1), (65536, 0, 0, 0), (1048576, 1, 1, 1)], ids=cases.settings_name)
def test_a_capacity_a_byte_below_the_bound_is_refused_untouched(g, settings):
    """every other item a byte short: OUTPUT_TOO_SMALL with not one byte of its destination written (write() holds a refused item's whole capacity to the fill), the
    items between them written"""
    named = [(c.name, c.data) for c in cases.by_settings()[settings]][:24]
    configure(g, settings)
    want = want_for(settings, named)
    caps = [ref.max_compressed_length(len(d), *settings) - (i % 2) for i, (_, d) in enumerate(named)]
    outs, status, err = write(g, [d for _, d in named], caps)
    assert status == [cases.MAX_OUTPUT if i % 2 else 0 for i in range(len(named))] and err == [0] * len(named)
    assert outs == [b"" if i % 2 else w for i, w in enumerate(want)]


@pytest.mark.parametrize("acceleration", (1, 7, 65537))
def test_accelerations_under_non_default_settings(g, acceleration):
    settings = (65536, 1, 0, 1)
    named = [(c.name, c.data) for c in cases.by_settings()[settings] if len(c.data) <= 131072 and not c.name.startswith("random")]
    wide = (262144, 0, 1, 0)
    for s, items in ((settings, named), (wide, [("text 262145", cases.data("text", 262145, 3)), ("zeros 70000", cases.data("zeros", 70000))])):
        configure(g, s, acceleration)
        want = want_for(s, items, acceleration)
        outs, status, err = write(g, [d for _, d in items], [ref.max_compressed_length(len(d), *s) for _, d in items])
        assert status == [0] * len(items) and outs == want, (s, acceleration)
        read_back(g, outs, [d for _, d in items], (s, acceleration))
    if acceleration > 1:
        assert want_for(settings, named, acceleration) != want_for(settings, named, 1)


def test_the_block_list_at_the_java_writers_settings(g, o):
    """lz4frame.compress.variant 1 at (4 MiB, 0, 0, 0): the oracle's Java writer's bytes, and variant 0's -- which asks Java's bound only"""
    named = [(c.name, c.data) for c in cases.by_settings()[(4194304, 0, 0, 0)]] + [(c.name, c.data) for c in cases.by_settings()[(65536, 0, 0, 0)]]
    items = [d for _, d in named]
    want = [o.compress("lz4frame", d) for d in items]
    configure(g, ref.DEFAULT, variant=0)
    lib = g.codec.lib
    outs0, status0, _ = write(g, items, [lib.achip_lz4frame_max_compressed_length(len(d)) for d in items])
    configure(g, ref.DEFAULT, variant=1)
    outs1, status1, err1 = write(g, items, [ref.max_compressed_length(len(d), *ref.DEFAULT) for d in items])
    assert status0 == status1 == [0] * len(items) and err1 == [0] * len(items)
    assert outs1 == want and outs0 == want
    # Java's bound is less than the block list asks: under variant 1 it is refused, under variant 0 it is enough
    short, status, _ = write(g, items[:3], [lib.achip_lz4frame_max_compressed_length(len(d)) for d in items[:3]])
    assert status == [cases.MAX_OUTPUT] * 3 and short == [b""] * 3


def test_every_entry_point_writes_the_contexts_frames(g, o):
    settings = (65536, 1, 1, 1)
    configure(g, settings)
    lib = g.codec.lib
    plain = GpuBatch()  # a second context, at the defaults: two contexts hold different values side by side
    assert plain.codec.native.get_lz4frame_writer() == (4194304, False, False, False)
    text, zeros, mix = cases.data("text", 70000, 5), cases.data("zeros", 65537), cases.data("text/random/text", 3 * 65536 + 777, 9)
    bound = lambda d: lib.achip_lz4frame_max_compressed_length_for(len(d), *settings)  # noqa: E731
    frames = [ref.compress(d, *settings) for d in (text, zeros, mix)]
    # achip_batch_host
    outs, status, err = g.run_host(LZ4F_C, [text, zeros, mix, b""], [bound(text), bound(zeros), bound(mix) - 1, bound(b"")])
    assert status == [0, 0, cases.MAX_OUTPUT, 0] and outs == [frames[0], frames[1], b"", ref.compress(b"", *settings)]
    # mixed batches in both forms: the LZ4 frame items by the settings, the items beside them as ever
    items = [(LZ4F_C, text, bound(text)), (LZ4_C, text, lib.achip_lz4_max_compressed_length(len(text))), (LZ4F_D, frames[2], len(mix)), (LZ4F_C, mix, bound(mix)),
             (SNAPPY_C, zeros, lib.achip_snappy_max_compressed_length(len(zeros))), (LZ4F_C, zeros, bound(zeros))]
    ops, blocks, caps = [i[0] for i in items], [i[1] for i in items], [i[2] for i in items]
    for run in ("device", "host"):
        mine, st, _ = write(g, blocks, caps, op=ops) if run == "device" else g.run_host(ops, blocks, caps)
        assert st == [0] * len(items), run
        assert (mine[0], mine[3], mine[5], mine[2]) == (frames[0], frames[2], frames[1], mix), run
        assert mine[1] == o.compress("lz4", text) and mine[4] == o.compress("snappy", zeros), run
        theirs, st, _ = plain.run(ops, blocks, caps) if run == "device" else plain.run_host(ops, blocks, caps)
        assert st == [0] * len(items) and theirs[0] == o.compress("lz4frame", text) and theirs[5] == o.compress("lz4frame", zeros), run
    # the single-buffer call, through the class that owns the settings
    A = g.A
    c = A.Lz4FrameHipCompressor(block_size=65536, block_checksum=True, content_checksum=True, content_size=True)
    for d, frame in zip((text, zeros, mix), frames):
        assert c.max_compressed_length(len(d)) == bound(d)
        out = np.full(bound(d) + 8, FILL, dtype=np.uint8)
        n = c.compress(d, 0, len(d), out, 4, bound(d))
        assert out[4:4 + n].tobytes() == frame and (out[:4] == FILL).all() and (out[4 + bound(d):] == FILL).all()
    with pytest.raises(A.IllegalArgumentException):
        c.compress(text, 0, len(text), np.zeros(bound(text) - 1, dtype=np.uint8), 0, bound(text) - 1)
    default = A.Lz4FrameHipCompressor()
    assert default.max_compressed_length(len(text)) == lib.achip_lz4frame_max_compressed_length(len(text))
    out = np.zeros(default.max_compressed_length(len(text)), dtype=np.uint8)
    assert out[:default.compress(text, 0, len(text), out, 0, len(out))].tobytes() == o.compress("lz4frame", text)


def test_frames_with_a_content_size_are_sized_and_planned_on_the_device(g):
    settings = (65536, 1, 1, 1)
    named = [(c.name, c.data) for c in cases.by_settings()[settings]]
    frames = want_for(settings, named)
    torch = g.torch
    src, src_off, src_len = g.pack(frames, align=1)
    to = lambda a: torch.from_numpy(a).to(g.dev)  # noqa: E731
    held = []

    def alloc(nbytes):
        held.append(torch.zeros(int(nbytes), dtype=torch.uint8, device=g.dev))
        return held[-1]
    r = g.codec.decompress_unsized(LZ4F_D, to(src), to(src_off), to(src_len), len(frames), alloc, align=16)
    g.codec.synchronize()
    view = lambda t, dt, n: t.cpu().numpy().view(dt)[:n]  # noqa: E731
    n = len(frames)
    assert view(r["out_size"], np.int64, n).tolist() == [len(d) for _, d in named] and not view(r["size_status"], np.int32, n).any()
    assert r["left_out"] == 0 and not view(r["status"], np.int32, n).any()
    dst, off, out_len = r["dst"].cpu().numpy(), view(r["dst_off"], np.int64, n), view(r["out_len"], np.int32, n)
    assert all(dst[off[i]:off[i] + out_len[i]].tobytes() == d for i, (_, d) in enumerate(named))


def test_compress_bound_batch_follows_the_settings(g):
    torch = g.torch
    lengths = np.array([0, 1, 12, 65535, 65536, 65537, 262145, 1000003, (4 << 20) + 1, 1 << 28, 1 << 30, 0x7FFFFFFF - 100000, 0x7FFFFFFF, -1], dtype=np.int32)
    lib = g.codec.lib

    def bounds(op=LZ4F_C):
        d_len = torch.from_numpy(lengths).to(g.dev)
        d_size = torch.full((len(lengths),), -7, dtype=torch.int64, device=g.dev)
        d_status = torch.full((len(lengths),), -7, dtype=torch.int32, device=g.dev)
        g.codec.compress_bounds(op, d_len, d_size, d_status, len(lengths))
        g.codec.synchronize()
        return list(zip(d_size.cpu().tolist(), d_status.cpu().tolist()))

    def held_to(f):
        for n, (size, st) in zip(lengths.tolist(), bounds()):
            want = f(n)
            assert (size, st) == ((want, 0) if want >= 0 else (0, cases.BAD_ARGUMENT)), n
    for settings in ((65536, 0, 0, 0), (65536, 1, 1, 1), (262144, 1, 0, 0), (4194304, 0, 1, 1)):
        configure(g, settings)
        held_to(lambda n: lib.achip_lz4frame_max_compressed_length_for(n, *settings))
        assert [s for s, _ in bounds()][:6] == [ref.max_compressed_length(int(n), *settings) for n in lengths[:6]]
        assert [s for s, _ in bounds(LZ4_C)][:6] == [n + n // 255 + 16 for n in lengths.tolist()[:6]]  # the other ops' lines do not move
    configure(g, ref.DEFAULT, variant=1)  # the block list at the Java writer's settings: its bound
    held_to(lambda n: lib.achip_lz4frame_max_compressed_length_for(n, *ref.DEFAULT))
    configure(g, ref.DEFAULT, variant=0)  # the Java writer: Java's formula
    held_to(lambda n: lib.achip_lz4frame_max_compressed_length(n))
