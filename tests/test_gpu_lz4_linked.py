"""LZ4 frames with linked blocks on the GPU (achip_ctx_set_lz4frame_linked_blocks): the catalog of tests/lz4_linked_cases.py -- constructed frames at every edge of
the rule and of the reader's output ring, damaged ones, frames of independent blocks among them -- through achip_lz4frame_decompress_batch, achip_lz4frame_decompress
and ACHIP_OP_LZ4FRAME_DECOMPRESS inside achip_mixed_batch, with the setting on and off, against the model of tests/lz4_linked_ref.py: plaintext, outLen, status,
detail and errOffset of every item, and not a byte written outside an item's capacity (canaries in front of every dstOff and behind every capacity).  Then
size -> plan -> decode (R1 / R2 of DESIGN 10b), the independent twin of the 256 KiB frame beside linked frames and alone, and the setter on a live context."""
import ctypes

import numpy as np
import pytest

from tests import lz4_linked_cases as cat, lz4_linked_ref as ref, oracle_lib

pytestmark = pytest.mark.gpu

OP_LZ4_DECOMPRESS, OP_SNAPPY_DECOMPRESS, OP_LZ4FRAME_DECOMPRESS = 0, 2, 6
CANARY, GAP = 0xA5, 48
LINKED_BLOCKS = ref.malformed(ref.D_LINKED_BLOCKS)


@pytest.fixture(scope="module")
def g():
    from tests.gpu_harness import GpuBatch
    gb = GpuBatch(0)
    yield gb
    gb.codec.native.set_lz4frame_linked_blocks(False)


@pytest.fixture(scope="module")
def want():
    """the model's answers, once: {accept: [Result per case]}"""
    return {accept: [ref.decompress(c.data, c.cap, accept) for c in cat.cases()] for accept in (True, False)}


def run_batch(g, ops, items, caps, shift, variant=None):
    """the items at sources and destinations `shift` bytes off a 16-byte boundary, GAP canary bytes around every destination -> [(status, errOffset, outLen,
    bytes)]; asserts that nothing outside the capacities was written.  ops: one op, or one per item (achip_mixed_batch)"""
    torch = g.torch
    n = len(items)
    src_off, dst_off, sp, dp = [], [], 16 + shift, 64 + shift
    for data, cap in zip(items, caps):
        src_off.append(sp)
        sp += (len(data) + 15) // 16 * 16 + 16
        dst_off.append(dp)
        dp += (cap + GAP + 15) // 16 * 16
    src = np.zeros(sp + 64, dtype=np.uint8)
    for data, so in zip(items, src_off):
        src[so:so + len(data)] = np.frombuffer(data, dtype=np.uint8)
    to = lambda a: torch.from_numpy(a).to(g.dev)  # noqa: E731
    d_src, d_so, d_sl = to(src), to(np.array(src_off, dtype=np.int64)), to(np.array([len(d) for d in items], dtype=np.int32))
    d_dst = torch.full((dp + 64,), CANARY, dtype=torch.uint8, device=g.dev)
    d_do, d_dc = to(np.array(dst_off, dtype=np.int64)), to(np.array(caps, dtype=np.int32))
    d_len, d_st = torch.full((n,), -7, dtype=torch.int32, device=g.dev), torch.full((n,), -7, dtype=torch.int32, device=g.dev)
    d_err = torch.full((n,), -7, dtype=torch.int64, device=g.dev)
    torch.cuda.synchronize()
    if variant is not None:
        g.set_option("lz4frame.decompress.variant", variant)
    try:
        if isinstance(ops, (list, tuple)):
            g.codec.launch_mixed(ops, d_src, d_so, d_sl, d_dst, d_do, d_dc, d_len, d_st, d_err, n)
        else:
            g.codec.launch(ops, d_src, d_so, d_sl, d_dst, d_do, d_dc, d_len, d_st, d_err, n)
        g.codec.synchronize()
    finally:
        if variant is not None:
            g.set_option("lz4frame.decompress.variant", 2)
    dst, out_len, status, err = d_dst.cpu().numpy(), d_len.cpu().numpy(), d_st.cpu().numpy(), d_err.cpu().numpy()
    covered = np.zeros(len(dst), dtype=bool)
    for at, cap in zip(dst_off, caps):
        covered[at:at + cap] = True
    assert (dst[~covered] == CANARY).all(), "bytes outside the items' capacities were written at %s" % np.nonzero((dst != CANARY) & ~covered)[0][:8].tolist()
    return [(int(status[k]), int(err[k]), int(out_len[k]), dst[dst_off[k]:dst_off[k] + max(int(out_len[k]), 0)].tobytes()) for k in range(n)]


def differences(cases, got, want):
    return [(c.name, r[:3], (w.status, w.offset, len(w.out)), "bytes differ" if r[0] == 0 and r[3] != w.out else "")
            for c, r, w in zip(cases, got, want) if r != (w.status, w.offset, len(w.out), w.out)]


def test_the_catalog_is_what_the_model_says_it_is(want):
    """(the CPU tests prove it case by case; here only that the GPU tests below compare with the answers they think they compare with)"""
    cases = cat.cases()
    assert sum(1 for c in cases if c.linked) >= 40 and sum(1 for c in cases if not c.linked) >= 2
    for c, on, off in zip(cases, want[True], want[False]):
        assert (on.status, on.offset) == (c.status, c.offset) and (c.plain is None or on.out == c.plain), c.name
        if c.linked:
            assert (off.status, off.offset) == (LINKED_BLOCKS, cat.linked_descriptor(c)), c.name
        else:
            assert off == on, c.name


@pytest.mark.parametrize("accept,variant,shift", [(True, 2, 0), (True, 2, 3), (True, 0, 1), (True, 0, 2), (False, 2, 3), (False, 0, 0)])
def test_batch(g, want, accept, variant, shift):
    """achip_lz4frame_decompress_batch, the whole catalog as one batch: through the list path with its serial kernel for the leftovers (variant 2, the default:
    every linked frame is a leftover) and through the wavefront-per-item kernel alone (variant 0)"""
    cases = cat.cases()
    g.codec.native.set_lz4frame_linked_blocks(accept)
    got = run_batch(g, OP_LZ4FRAME_DECOMPRESS, [c.data for c in cases], [c.cap for c in cases], shift, variant)
    assert differences(cases, got, want[accept]) == []


@pytest.mark.parametrize("accept", [True, False])
def test_single_host_buffer(g, want, accept):
    """achip_lz4frame_decompress: one item, host pointers, the destination at an odd address with canaries around it"""
    lib, ctx = g.codec.lib, g.codec.native.ctx
    g.codec.native.set_lz4frame_linked_blocks(accept)
    wrong = []
    for k, (c, w) in enumerate(zip(cat.cases(), want[accept])):
        src = np.frombuffer(c.data, dtype=np.uint8)
        shift = 1 + k % 3
        dst = np.full(shift + c.cap + GAP, CANARY, dtype=np.uint8)
        eo = ctypes.c_int64(-7)
        r = lib.achip_lz4frame_decompress(ctx, src.ctypes.data, dst.ctypes.data + shift if c.cap else None, len(src), c.cap, ctypes.byref(eo))
        assert (dst[:shift] == CANARY).all() and (dst[shift + c.cap:] == CANARY).all(), c.name
        got = (0, 0, r, dst[shift:shift + r].tobytes()) if r >= 0 else (r, eo.value, 0, b"")
        if got != (w.status, w.offset, len(w.out), w.out):
            wrong.append((c.name, got[:3], (w.status, w.offset, len(w.out))))
    assert wrong == []


@pytest.mark.parametrize("accept", [True, False])
def test_mixed_batch_beside_an_lz4_block_and_a_snappy_block(g, want, accept):
    """ACHIP_OP_LZ4FRAME_DECOMPRESS inside achip_mixed_batch: the helper contexts take a copy of the setting; the other codecs' items are not touched by it"""
    o = oracle_lib.load()
    cases = cat.cases()
    plain = cat.text(5000, seed=5)
    items = [o.compress("lz4", plain)] + [c.data for c in cases] + [o.compress("snappy", plain)]
    caps = [len(plain)] + [c.cap for c in cases] + [len(plain)]
    ops = [OP_LZ4_DECOMPRESS] + [OP_LZ4FRAME_DECOMPRESS] * len(cases) + [OP_SNAPPY_DECOMPRESS]
    g.codec.native.set_lz4frame_linked_blocks(accept)
    got = run_batch(g, ops, items, caps, 3)
    assert got[0] == (0, 0, len(plain), plain) and got[-1] == (0, 0, len(plain), plain)
    assert differences(cases, got[1:-1], want[accept]) == []


@pytest.mark.parametrize("accept", [True, False])
def test_size_plan_decode(g, want, accept):
    """achip_decoded_size_batch, achip_plan_outputs and the decode with the planned capacities.  R1: an item the reader decodes is sized exactly and comes out
    whole at its planned place; R2: a size reported for any other item is not one the reader decodes it to; a reported fault is the reader's own.  With the
    setting off the linked frames are reported at their descriptor, as the reader reports them"""
    torch = g.torch
    cases = cat.cases()
    n = len(cases)
    roomy = [ref.decompress(c.data, sum(f.content for f in ref.walk(c.data)) + 64, accept) for c in cases]  # the reader when room is no question
    g.codec.native.set_lz4frame_linked_blocks(accept)
    offs, pos = [], 3
    for c in cases:
        offs.append(pos)
        pos += len(c.data) + len(c.data) % 5 + 1
    src = np.zeros(pos + 64, dtype=np.uint8)
    for c, so in zip(cases, offs):
        src[so:so + len(c.data)] = np.frombuffer(c.data, dtype=np.uint8)
    to = lambda a: torch.from_numpy(a).to(g.dev)  # noqa: E731
    d_src, d_so, d_sl = to(src), to(np.array(offs, dtype=np.int64)), to(np.array([len(c.data) for c in cases], dtype=np.int32))
    d_size, d_sst, d_serr = (torch.full((n,), -7, dtype=t, device=g.dev) for t in (torch.int64, torch.int32, torch.int64))
    d_do, d_dc, d_total = torch.zeros(n, dtype=torch.int64, device=g.dev), torch.zeros(n, dtype=torch.int32, device=g.dev), torch.zeros(2, dtype=torch.int64, device=g.dev)
    d_len, d_st, d_err = (torch.full((n,), -7, dtype=t, device=g.dev) for t in (torch.int32, torch.int32, torch.int64))
    torch.cuda.synchronize()
    g.codec.decoded_sizes(OP_LZ4FRAME_DECOMPRESS, d_src, d_so, d_sl, d_size, d_sst, d_serr, n)
    g.codec.plan_outputs(d_size, d_sst, n, 1, d_do, d_dc, d_total)
    g.codec.synchronize()
    total = int(d_total[0].item())
    d_dst = torch.full((total + 64,), CANARY, dtype=torch.uint8, device=g.dev)
    torch.cuda.synchronize()
    g.codec.launch(OP_LZ4FRAME_DECOMPRESS, d_src, d_so, d_sl, d_dst, d_do, d_dc, d_len, d_st, d_err, n)
    g.codec.synchronize()
    size, sst, serr, do, out_len, st, dst = (t.cpu().numpy() for t in (d_size, d_sst, d_serr, d_do, d_len, d_st, d_dst))
    assert (dst[total:] == CANARY).all()
    wrong = []
    for k, (c, w) in enumerate(zip(cases, roomy)):
        s, z, e = int(sst[k]), int(size[k]), int(serr[k])
        if not accept and c.linked:
            ok = (s, e, z) == (LINKED_BLOCKS, cat.linked_descriptor(c), 0)
        elif w.status == 0:  # R1
            ok = (s, z) == (0, len(w.out)) and int(st[k]) == 0 and int(out_len[k]) == z and dst[do[k]:do[k] + z].tobytes() == w.out
        elif s == 0:  # R2
            ok = not (int(st[k]) == 0 and int(out_len[k]) != z) and int(st[k]) == ref.decompress(c.data, z, accept).status
        else:
            ok = (s, e, z) == (w.status, w.offset, 0)
        if not ok:
            wrong.append((c.name, s, e, z, int(st[k]), int(out_len[k]), w.status, w.offset, len(w.out)))
    assert wrong == []


def test_the_independent_twin_decodes_alike_beside_linked_frames_and_alone(g, want):
    cases = cat.cases()
    k = next(i for i, c in enumerate(cases) if c.name == "256 KiB of text, independent")
    twin = cases[k]
    g.codec.native.set_lz4frame_linked_blocks(True)
    beside = run_batch(g, OP_LZ4FRAME_DECOMPRESS, [c.data for c in cases], [c.cap for c in cases], 0)[k]
    alone = run_batch(g, OP_LZ4FRAME_DECOMPRESS, [twin.data], [twin.cap], 0)[0]
    g.codec.native.set_lz4frame_linked_blocks(False)
    before = run_batch(g, OP_LZ4FRAME_DECOMPRESS, [twin.data], [twin.cap], 0)[0]
    assert beside == alone == before == (0, 0, len(twin.plain), twin.plain)


def test_the_setting_on_a_live_context(g):
    import aircompressor_amd as A
    n = g.codec.native
    fresh = A.HipNative(0)
    assert fresh.get_lz4frame_linked_blocks() is False  # the default is the Java reader's
    fresh.close()
    n.set_lz4frame_linked_blocks(True)
    assert n.get_lz4frame_linked_blocks() is True
    for bad in (2, -1, 256):
        with pytest.raises(A.IllegalArgumentException):
            n.set_lz4frame_linked_blocks(bad)
        assert n.get_lz4frame_linked_blocks() is True  # a refused value leaves the stored one
    n.set_lz4frame_linked_blocks(False)
    assert n.get_lz4frame_linked_blocks() is False
    # the reader object hands its own value to a shared context before every call
    case = next(c for c in cat.cases() if c.name == "straddling periodic match")
    src, out = np.frombuffer(case.data, dtype=np.uint8), np.zeros(case.cap, dtype=np.uint8)
    accepting, strict = A.Lz4FrameHipDecompressor(native_ctx=n, accept_linked_blocks=True), A.Lz4FrameHipDecompressor(native_ctx=n)
    assert accepting.decompress_segment(src, out) == len(case.plain) and out.tobytes() == case.plain
    with pytest.raises(A.MalformedInputException) as e:
        strict.decompress_segment(src, out)
    assert "linked blocks are not supported" in str(e.value)
    assert accepting.decompress_segment(src, out) == len(case.plain)
    n.set_lz4frame_linked_blocks(False)
