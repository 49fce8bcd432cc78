"""achip_decoded_size_batch and achip_plan_outputs on the GPU, the oracle as the checker (tests/decoded_size_cases.py has the inputs and the rules R1 / R2):
clean items of all seven ops are sized exactly; size -> plan -> decode reaches the plaintext at exact offsets with nothing but the total read back; seeded
damaged items fall under R1, R2 or R3 "a reported fault is the reader's fault"; the planner alone against numpy; HipBatchCodec.decompress_unsized."""
import numpy as np
import pytest

from tests import decoded_size_cases as cases, oracle_lib

pytestmark = pytest.mark.gpu

OP_NAMES = list(cases.OPS)


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


@pytest.fixture(scope="module")
def g():
    from tests.gpu_harness import GpuBatch
    return GpuBatch(0)


@pytest.fixture(scope="module")
def clean(o):
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = cases.clean_items(o, name)
        return memo[name]
    return get


def upload(g, items, misalign=3):
    """the items packed at odd offsets from a misaligned base; returns the device tensors (src, srcOff, srcLen)"""
    torch = g.torch
    offs, pos = [], misalign
    for b in items:
        offs.append(pos)
        pos += len(b) + (len(b) % 5) + 1
    src = np.zeros(pos + 64, dtype=np.uint8)
    for b, so in zip(items, offs):
        src[so:so + len(b)] = np.frombuffer(b, dtype=np.uint8)
    to = lambda a: torch.from_numpy(a).to(g.dev)  # noqa: E731
    return to(src), to(np.array(offs, dtype=np.int64)), to(np.array([len(b) for b in items], dtype=np.int32))


def size_on_gpu(g, op, items):
    """(outSize, status, errOffset) as numpy arrays, and the device tensors behind them"""
    torch = g.torch
    n = len(items)
    d_src, d_off, d_len = upload(g, items)
    d_size = torch.full((n,), -7, dtype=torch.int64, device=g.dev)
    d_status = torch.full((n,), -7, dtype=torch.int32, device=g.dev)
    d_err = torch.full((n,), -7, dtype=torch.int64, device=g.dev)
    torch.cuda.synchronize()
    g.codec.decoded_sizes(op, d_src, d_off, d_len, d_size, d_status, d_err, n)
    g.codec.synchronize()
    return d_size.cpu().numpy(), d_status.cpu().numpy(), d_err.cpu().numpy(), (d_src, d_off, d_len, d_size, d_status)


@pytest.mark.parametrize("name", OP_NAMES)
def test_clean_items_are_sized_exactly(o, g, clean, name):
    items = clean(name)
    for label, comp, n in items:  # the set is not hollow: the oracle decodes every one of them at exact capacity
        assert cases.exact_length(o, name, comp, n + 64) == n, (name, label)
    size, status, err, _ = size_on_gpu(g, cases.OPS[name], [c for _, c, _ in items])
    wrong = [(label, n, int(s), int(z)) for (label, _, n), s, z in zip(items, status, size) if s != 0 or z != n]
    print("%s: %d clean items, %d wrong" % (name, len(items), len(wrong)))
    assert not wrong, wrong[:8]
    assert (err == 0).all()


@pytest.mark.parametrize("align", [1, 16, 4096])
@pytest.mark.parametrize("name", OP_NAMES)
def test_unsized_flow_reaches_the_plaintext_at_exact_offsets(o, g, clean, name, align):
    torch = g.torch
    items = clean(name)
    n = len(items)
    op = cases.OPS[name]
    plain = [cases.decode(o, name, comp, length) for _, comp, length in items]
    _, _, _, (d_src, d_off, d_len, d_size, d_status) = size_on_gpu(g, op, [c for _, c, _ in items])
    d_dst_off = torch.full((n,), -7, dtype=torch.int64, device=g.dev)
    d_dst_cap = torch.full((n,), -7, dtype=torch.int32, device=g.dev)
    d_total = torch.full((2,), -7, dtype=torch.int64, device=g.dev)
    g.codec.plan_outputs(d_size, d_status, n, align, d_dst_off, d_dst_cap, d_total)
    total = d_total.cpu().numpy()  # the one readback
    lengths = np.array([len(p) for p in plain], dtype=np.int64)
    room = (lengths + align - 1) // align * align
    assert (d_dst_cap.cpu().numpy() == lengths).all()
    assert (d_dst_off.cpu().numpy() == np.cumsum(room) - room).all()
    assert total[0] == room.sum() and total[1] == 0
    d_dst = torch.full((int(total[0]) + 64,), 0xA5, dtype=torch.uint8, device=g.dev)
    d_out_len = torch.full((n,), -7, dtype=torch.int32, device=g.dev)
    d_st = torch.full((n,), -7, dtype=torch.int32, device=g.dev)
    d_eo = torch.zeros((n,), dtype=torch.int64, device=g.dev)
    torch.cuda.synchronize()
    g.codec.launch(op, d_src, d_off, d_len, d_dst, d_dst_off, d_dst_cap, d_out_len, d_st, d_eo, n)
    g.codec.synchronize()
    assert (d_st.cpu().numpy() == 0).all(), d_st.cpu().numpy().tolist()
    assert (d_out_len.cpu().numpy() == lengths).all()
    want = np.full(int(total[0]) + 64, 0xA5, dtype=np.uint8)  # plaintext at the planned places, the fill everywhere else
    for p, at in zip(plain, np.cumsum(room) - room):
        want[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
    assert (d_dst.cpu().numpy() == want).all()


# what the seeded generator delivers per op, as tools/hostemu/check_size.py prints it for the same seeds (the emulator, no GPU): a category an op cannot produce
# is not asked for -- x-snappy-framed checks a CRC of every chunk, so a damaged copy decodes only where the damage wrote the byte that was there; a Hadoop LZ4 chunk
# whose block length says more than it holds is decoded into the stream's own buffer, with room to spare, so the LZ4 end-of-block rules never bite.
EXPECTED_CATEGORIES = {
    "lz4": {"exact", "r2", "fault"},
    "snappy": {"exact", "r2", "fault"},
    "zstd": {"exact", "r2", "fault"},
    "lz4frame": {"exact", "r2", "fault"},
    "snappyframed": {"r2", "fault"},
    "lz4hadoop": {"exact", "fault"},
    "snappyhadoop": {"exact", "r2", "fault"},
}


@pytest.mark.parametrize("name", OP_NAMES)
def test_damaged_items_obey_r1_and_r2(o, g, name):
    """... and R3: a fault sizing reports is the fault the op's reader reports, status and offset (tests/decoded_size_cases.py)"""
    op = cases.OPS[name]
    items = cases.damaged_items(o, name, 100 + op, 400)
    data = [d for _, d, _ in items]
    size, status, err, _ = size_on_gpu(g, op, data)
    seen = {"exact": 0, "r2": 0, "fault": 0, "payload": 0}
    wrong = []
    for (kind, d, room), z, s, e in zip(items, size, status, err):
        category, what = cases.judge(o, name, d, room, int(z), int(s), int(e))
        seen[category] += 1
        if what:
            wrong.append((kind, len(d), what))
    print("%s: %s" % (name, seen))
    assert not wrong, wrong[:8]
    assert cases.payload_share_wrong(name, seen) is None, seen
    assert {c for c, k in seen.items() if k > 0} >= EXPECTED_CATEGORIES[name], seen
    if name == "lz4":  # the same items often enough for the lane-per-block shape: the two shapes agree item by item
        reps = 16384 // len(data) + 2
        size2, status2, _, _ = size_on_gpu(g, op, data * reps)
        assert (size2.reshape(reps, -1) == size[None, :]).all() and (status2.reshape(reps, -1) == status[None, :]).all()


def test_planner_alone(g):
    torch = g.torch
    rng = np.random.default_rng(17)
    for n in (1, 1000, 1_000_003):
        sizes = rng.integers(0, 70000, n).astype(np.int64)
        status = np.where(rng.integers(0, 9, n) == 0, -(1 + 16 * 2), 0).astype(np.int32)
        sizes[n // 2] = (1 << 31) + 5  # beyond INT32_MAX: left out
        sizes[n // 3] = cases.INT32_MAX if status[n // 3] != 0 or n > 1000 else sizes[n // 3]
        left = (status != 0) | (sizes > cases.INT32_MAX)
        for align in (1, 16, 4096):
            d_off = torch.full((n,), -7, dtype=torch.int64, device=g.dev)
            d_cap = torch.full((n,), -7, dtype=torch.int32, device=g.dev)
            d_total = torch.full((2,), -7, dtype=torch.int64, device=g.dev)
            g.codec.plan_outputs(torch.from_numpy(sizes).to(g.dev), torch.from_numpy(status).to(g.dev), n, align, d_off, d_cap, d_total)
            g.codec.synchronize()
            cap = np.where(left, 0, sizes)
            room = (cap + align - 1) // align * align
            assert (d_cap.cpu().numpy() == cap).all(), (n, align)
            assert (d_off.cpu().numpy() == np.cumsum(room) - room).all(), (n, align)
            assert d_total.cpu().numpy().tolist() == [int(room.sum()), int(left.sum())], (n, align)
    for align in (0, 3, 8192):
        with pytest.raises(g.A.IllegalArgumentException):
            g.codec.plan_outputs(d_off, d_cap, 1, align, d_off, d_cap, d_total)


@pytest.mark.parametrize("name", OP_NAMES)
def test_decompress_unsized_gives_the_plaintext(o, g, name):
    torch = g.torch
    items = cases.clean_items(o, name, big=False)[:40]
    damaged = cases.damaged_items(o, name, 7, 8)
    data = [c for _, c, _ in items] + [d for _, d, _ in damaged]
    n = len(data)
    d_src, d_off, d_len = upload(g, data)
    r = g.codec.decompress_unsized(cases.OPS[name], d_src, d_off, d_len, n, lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=g.dev), align=16)
    g.codec.synchronize()
    as_np = lambda t, dtype: t.cpu().numpy().view(dtype)[:n]  # noqa: E731
    size_status, out_size = as_np(r["size_status"], np.int32), as_np(r["out_size"], np.int64)
    status, out_len, dst_off = as_np(r["status"], np.int32), as_np(r["out_len"], np.int32), as_np(r["dst_off"], np.int64)
    assert r["left_out"] == int((size_status != 0).sum())
    room = (np.where(size_status != 0, 0, out_size) + 15) // 16 * 16
    assert r["total_bytes"] == room.sum() and (dst_off == np.cumsum(room) - room).all()
    for i, (label, comp, length) in enumerate(items):  # the same bytes as the explicit flow gives (the test above): the plaintext
        assert size_status[i] == 0 and status[i] == 0 and out_len[i] == length, (label, size_status[i], status[i])
        assert r["dst"][int(dst_off[i]):int(dst_off[i]) + length].cpu().numpy().tobytes() == cases.decode(o, name, comp, length), label
    for i in range(len(items), n):  # damaged items: left out, or decoded to exactly the size sizing gave, or refused by the decoder (R2)
        assert size_status[i] != 0 or status[i] != 0 or out_len[i] == out_size[i]
