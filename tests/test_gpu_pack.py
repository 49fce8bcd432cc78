"""achip_compress_bound_batch and achip_pack_outputs on the GPU (tests/pack_cases.py has the cases and the numpy statement of the contract): the bounds of all
eight compress ops against the host functions and into the planner; the pack call alone against numpy, byte for byte with the prefill around it; a stream that
does not fit; keep-the-smaller; and HipBatchCodec.compress_packed per op against the oracle's encoders and back through the decoders."""
import numpy as np
import pytest

from tests import common, oracle_lib, pack_cases as cases

pytestmark = pytest.mark.gpu

OP_NAMES = list(cases.COMPRESS_OPS)


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


@pytest.fixture(scope="module")
def g():
    from tests.gpu_harness import GpuBatch
    return GpuBatch(0)


@pytest.fixture(scope="module")
def tile(g):
    t = g.codec.native.get_stat("pack.tile_bytes")
    assert t > 0 and t % 4096 == 0
    return t


@pytest.fixture(scope="module")
def sets(tile):
    """(a) .. (d) per alignment, made once"""
    memo = {}

    def get(align):
        if align not in memo:
            memo[align] = cases.pack_cases(tile, align)
        return memo[align]
    return get


def pack_on_gpu(g, case, align, use_raw=False, cap_delta=0, plan_only=False):
    """one pack call over `case`; -> the mismatches against numpy"""
    torch = g.torch
    to = lambda a: torch.from_numpy(a).to(g.dev)  # noqa: E731
    want_total = case.expect(align, use_raw)[3]
    cap = want_total + cap_delta
    d_src, d_off, d_len, d_status = to(case.src), to(case.src_off), to(case.out_len), to(case.status)
    raw = dict(raw=to(case.raw), raw_off=to(case.raw_off), raw_len=to(case.raw_len), stored=torch.full((case.n,), -7, dtype=torch.int32, device=g.dev)) if use_raw else {}
    d_packed = torch.full((max(cap, 0) + cases.GUARD,), cases.PREFILL, dtype=torch.uint8, device=g.dev)
    assert d_src.data_ptr() % 16 == 0 and d_packed.data_ptr() % 16 == 0  # (case (b)'s residues and tile boundaries are laid out for aligned buffers)
    d_poff = torch.full((case.n,), -7, dtype=torch.int64, device=g.dev)
    d_plen = torch.full((case.n,), -7, dtype=torch.int32, device=g.dev)
    d_total = torch.full((3,), -7, dtype=torch.int64, device=g.dev)
    torch.cuda.synchronize()
    g.codec.pack_outputs(d_src, d_off, d_len, d_status, case.n, align, None if plan_only else d_packed, cap, d_poff, d_plen, d_total, **raw)
    g.codec.synchronize()
    stored = raw["stored"].cpu().numpy() if use_raw else None
    return cases.mismatches(case, align, use_raw, not plan_only and cap_delta >= 0, d_packed.cpu().numpy(), 0, d_poff.cpu().numpy(), d_plen.cpu().numpy(), stored,
                            d_total.cpu().numpy())


@pytest.mark.parametrize("name", OP_NAMES)
def test_bounds_equal_the_host_functions_and_feed_the_planner(g, name):
    torch = g.torch
    lib = g.codec.lib
    lengths = np.array(cases.BOUND_LENGTHS + list(range(250, 262)) * 30, dtype=np.int32)  # (more than one workgroup)
    n = len(lengths)
    d_len = torch.from_numpy(lengths).to(g.dev)
    buffers = (cases.HADOOP_DEFAULT_BUFFER, cases.HADOOP_OTHER_BUFFER) if "hadoop" in name else (cases.HADOOP_DEFAULT_BUFFER,)
    try:
        for buffer_size in buffers:
            g.set_option("hadoop.buffer_size", buffer_size)
            d_size = torch.full((n,), -7, dtype=torch.int64, device=g.dev)
            d_status = torch.full((n,), -7, dtype=torch.int32, device=g.dev)
            torch.cuda.synchronize()  # (torch fills on its own stream, the library runs on the context's)
            g.codec.compress_bounds(cases.COMPRESS_OPS[name], d_len, d_size, d_status, n)
            g.codec.synchronize()
            size, status = d_size.cpu().numpy(), d_status.cpu().numpy()
            wrong = cases.check_bounds(lib, name, lengths, size, status, lib.achip_status_class, buffer_size)
            assert not wrong, wrong[:8]
            assert (status[lengths < 0] != 0).all() and (status == 0).sum() >= n - 14  # the set is not hollow: most lengths have a bound
            # ... and the pair feeds the planner unchanged
            d_off = torch.full((n,), -7, dtype=torch.int64, device=g.dev)
            d_cap = torch.full((n,), -7, dtype=torch.int32, device=g.dev)
            d_total = torch.full((2,), -7, dtype=torch.int64, device=g.dev)
            torch.cuda.synchronize()
            g.codec.plan_outputs(d_size, d_status, n, 16, d_off, d_cap, d_total)
            g.codec.synchronize()
            cap = np.where(status != 0, 0, size)
            room = (cap + 15) // 16 * 16
            assert (d_cap.cpu().numpy() == cap).all() and (d_off.cpu().numpy() == np.cumsum(room) - room).all()
            assert d_total.cpu().numpy().tolist() == [int(room.sum()), int((status != 0).sum())]
    finally:
        g.set_option("hadoop.buffer_size", cases.HADOOP_DEFAULT_BUFFER)
    with pytest.raises(g.A.IllegalArgumentException):
        g.codec.compress_bounds(cases.COMPRESS_OPS[name] - 1 if name != "zstdstream" else 15, d_len, d_size, d_status, n)


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["a-one-item", "b-mixed", "c-many-short", "d-all-left-out"])
@pytest.mark.parametrize("align", cases.ALIGNS)
def test_pack_alone_against_numpy(g, sets, align, which):
    case = sets(align)[which]
    total = case.expect(align)[3]
    print("%s, align %d: %d items, %d dense bytes" % (case.name, align, case.n, total))
    assert (total == 0) == (which == 3)
    wrong = pack_on_gpu(g, case, align)
    assert not wrong, wrong


@pytest.mark.parametrize("align", cases.ALIGNS)
def test_a_stream_that_does_not_fit_is_not_copied(g, sets, align):
    b = sets(align)[1]
    wrong = pack_on_gpu(g, b, align, cap_delta=-1)  # total[2] == 0, the buffer still all prefill, offsets / lengths / total[0..1] as ever
    assert not wrong, wrong
    wrong = pack_on_gpu(g, b, align, plan_only=True)
    assert not wrong, wrong


@pytest.mark.parametrize("align", cases.ALIGNS)
def test_keep_the_smaller(g, tile, align):
    rng = np.random.default_rng(23 + align)
    b = cases.case_b(rng, tile, align).with_raw(rng)
    _, _, stored, _, _, _ = b.expect(align, True)
    packed = int(b.packed.sum())
    assert packed // 3 < stored.sum() < 2 * packed // 3 and ((b.out_len == b.raw_len) & b.packed).sum() > 20 and (stored[~b.packed] == 0).all()
    wrong = pack_on_gpu(g, b, align, use_raw=True)
    assert not wrong, wrong


def _plaintexts():
    text = b"".join(bytes(d) for _, d, _ in common.corpus_sample())
    rng = np.random.default_rng(41)
    out = [b"", b"x", bytes(text[:65536])]
    out += [bytes(d[:(977 * (i + 3)) % 20000 + 1]) for i, (_, d, _) in enumerate(common.corpus_sample()[:8])]
    out += [bytes(b) for b in common.synthetic_blocks(5, 12, block_size=8192)]
    out += [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (3000, 65536)]  # incompressible
    out.append((text * ((1 << 20) // len(text) + 1))[:1 << 20])
    out += [bytes(text[k:k + 1500 + 37 * k]) for k in range(1, 8)]
    return out


def _encode(o, name, data):
    if name == "zstdstream":
        return o.zstd_stream_compress(data)
    if name.endswith("hadoop"):
        return o.hadoop_compress(name[:-6], data)
    return o.compress(name, data)


@pytest.mark.parametrize("name", OP_NAMES)
def test_compress_packed_equals_the_oracle_and_decodes(o, g, name):
    torch = g.torch
    A = g.A
    plain = _plaintexts()
    n = len(plain)
    assert 35 <= n <= 50 and {0, 1, 65536, 1 << 20} <= {len(p) for p in plain}
    want = [_encode(o, name, p) for p in plain]
    src, off, ln = [], [], []
    pos = 3
    for p in plain:  # odd offsets, gaps
        off.append(pos)
        src.append(p)
        pos += len(p) + (len(p) % 5) + 1
    buf = np.full(pos + 64, 0x5A, dtype=np.uint8)
    for p, at in zip(plain, off):
        buf[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
    d_src = torch.from_numpy(buf).to(g.dev)
    d_off = torch.from_numpy(np.array(off, dtype=np.int64)).to(g.dev)
    d_len = torch.from_numpy(np.array([len(p) for p in plain], dtype=np.int32)).to(g.dev)

    def alloc(nbytes):  # prefilled, and the fill (on torch's stream) done before the library (on the context's) writes
        t = torch.full((nbytes + cases.GUARD,), cases.PREFILL, dtype=torch.uint8, device=g.dev)
        torch.cuda.synchronize()
        return t

    as_np = lambda t, dtype: t.cpu().numpy()[:t.numel() - cases.GUARD].view(dtype)[:n]  # noqa: E731
    op = cases.COMPRESS_OPS[name]

    r = g.codec.compress_packed(op, d_src, d_off, d_len, n, alloc, align=1)
    g.codec.synchronize()
    status, packed_off, packed_len = as_np(r["status"], np.int32), as_np(r["packed_off"], np.int64), as_np(r["packed_len"], np.int32)
    assert (status == 0).all() and (as_np(r["bound_status"], np.int32) == 0).all() and r["left_out"] == 0 and r["stored"] is None
    dense = b"".join(want)  # the oracle's compressed bytes of the items, concatenated: an independent producer pins the copy
    assert r["total_bytes"] == len(dense)
    lengths = np.array([len(w) for w in want], dtype=np.int64)
    assert (packed_len == lengths).all() and (packed_off == np.cumsum(lengths) - lengths).all()
    got = r["packed"].cpu().numpy()
    assert got[:len(dense)].tobytes() == dense
    assert (got[len(dense):] == cases.PREFILL).all()  # exact extents: nothing at or beyond total[0]

    # the dense buffer through the op's decoder, srcOff = packedOff and srcLen = packedLen (ZSTDSTREAM writes Zstd frames)
    dop = A.OP_ZSTD_DECOMPRESS if name == "zstdstream" else op - 1
    caps = np.array([max(len(p), 1) for p in plain], dtype=np.int32)
    room = (caps.astype(np.int64) + 15) // 16 * 16
    dst_off = np.cumsum(room) - room
    d_dst = torch.full((int(room.sum()) + 64,), cases.PREFILL, dtype=torch.uint8, device=g.dev)
    d_out_len = torch.full((n,), -7, dtype=torch.int32, device=g.dev)
    d_st = torch.full((n,), -7, dtype=torch.int32, device=g.dev)
    d_eo = torch.zeros((n,), dtype=torch.int64, device=g.dev)
    d_dst_off, d_caps = torch.from_numpy(dst_off).to(g.dev), torch.from_numpy(caps).to(g.dev)
    torch.cuda.synchronize()
    g.codec.launch(dop, r["packed"], r["packed_off"], r["packed_len"], d_dst, d_dst_off, d_caps, d_out_len, d_st, d_eo, n)
    g.codec.synchronize()
    out, out_len, st = d_dst.cpu().numpy(), d_out_len.cpu().numpy(), d_st.cpu().numpy()
    for i, p in enumerate(plain):
        if len(p) == 0:  # (what a decoder makes of an empty plaintext's stream is its own tests' business)
            continue
        assert st[i] == 0 and out_len[i] == len(p) and out[dst_off[i]:dst_off[i] + len(p)].tobytes() == p, (i, len(p), st[i])

    # raw fallback: an incompressible item is kept as its plaintext, a compressible one as the oracle's bytes
    r = g.codec.compress_packed(op, d_src, d_off, d_len, n, alloc, align=16, raw_fallback=True)
    g.codec.synchronize()
    stored, packed_off, packed_len = as_np(r["stored"], np.int32), as_np(r["packed_off"], np.int64), as_np(r["packed_len"], np.int32)
    got = r["packed"].cpu().numpy()
    assert (packed_off % 16 == 0).all()
    seen = [0, 0]
    for i, (p, w) in enumerate(zip(plain, want)):
        keep_raw = len(w) >= len(p)
        seen[keep_raw] += 1
        assert stored[i] == (1 if keep_raw else 0), (i, len(p), len(w))
        assert got[packed_off[i]:packed_off[i] + packed_len[i]].tobytes() == (p if keep_raw else w), i
    assert stored[plain.index(plain[-9])] == 1 and min(seen) >= 3, seen  # (the 65 536 bytes of noise; both kinds occur)
    assert (got[r["total_bytes"]:] == cases.PREFILL).all()
