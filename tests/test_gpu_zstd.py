"""GPU parity tests (through the C ABI) for the Zstd frame decoder against the CPU oracle and the reference's
golden decoder fixtures (T/zstd/AbstractTestZstd.java:41-78,175-184).  Frames with diverse features come from
libzstd via pyarrow (a third-party encoder, like zstd-jni in T/zstd/TestZstd.java:21-47)."""
import numpy as np
import pytest

from tests import common, oracle_lib
from tests import zstd_frame_cases as zc
from tests.oracle_lib import OracleError

pytestmark = pytest.mark.gpu
OP_ZSTD_DECOMPRESS = 4


@pytest.fixture(scope="module")
def gb():
    from tests.gpu_harness import GpuBatch
    return GpuBatch(0)


@pytest.fixture(scope="module", params=[(1, None), (0, None), (1, 0)], ids=["pipeline", "one-kernel", "pipeline-rings"])
def gbd(request):
    """decoder under test: the five-stage pipeline (default: batches of this module's sizes run its record executor), the one-kernel decoder it falls back to,
    and the pipeline with every item on its ring executor (zstd.decompress.exec 0: what the default picks for long-sequence items of large batches)"""
    from tests.gpu_harness import GpuBatch
    variant, exec_mode = request.param
    options = {"zstd.decompress.variant": variant}
    if exec_mode is not None:
        options["zstd.decompress.exec"] = exec_mode
    g = GpuBatch(0, options=options)
    g.variant = variant
    return g


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


DEFAULT_SEQ_WAVES = 1  # (the library's default of zstd.decompress.seq_waves, restored by the test that changes it)
DEFAULT_LIT_ITEMS = 13  # (... of zstd.decompress.lit_items)


def zstd_frames(blocks, level):
    import pyarrow as pa
    codec = pa.Codec("zstd", compression_level=level)
    return [codec.compress(b, asbytes=True) if len(b) else codec.compress(b"", asbytes=True) for b in blocks]


def plain_blocks():
    sample = [d for _, d, _ in common.corpus_sample()]
    blocks = list(sample)
    blocks += [sample[i] + sample[i + 1] for i in range(0, len(sample) - 1, 2)]  # 128 KiB: one full zstd block
    blocks += common.synthetic_blocks(21, 18)
    blocks += [d for _, d in common.HAND_CASES]
    return blocks


def test_golden_fixtures(gbd, o):
    z1, p1 = common.golden_zstd("with-checksum.zst"), common.golden_zstd("with-checksum")
    z2, p2 = common.golden_zstd("multiple-frames.zst"), common.golden_zstd("multiple-frames")
    outs, status, err = gbd.run(OP_ZSTD_DECOMPRESS, [z1, z2, z1, z2], [len(p1), len(p2), len(p1) + 500, len(p2) + 1], unaligned=True)
    assert status == [0, 0, 0, 0], (status, err)
    assert outs[0] == p1 and outs[2] == p1 and outs[1] == p2 and outs[3] == p2


def _expect(o, data, cap):
    try:
        return 0, 0, o.decompress("zstd", data, cap)
    except OracleError as e:
        return e.status, e.offset, None


def test_error_fixtures_and_corruptions(gbd, o):
    rng = np.random.default_rng(5)
    z1, p1 = common.golden_zstd("with-checksum.zst"), common.golden_zstd("with-checksum")
    cases = [
        (common.golden_zstd("offset-before-start.zst"), 1 << 20),  # "Input is corrupted"
        (common.golden_zstd("bad-second-frame.zst"), 1 << 20),      # "Invalid magic prefix"
        (z1, len(p1) - 1),                                          # "Output buffer too small"
        (z1[:-1], len(p1)), (z1[:-4], len(p1)), (z1[:100], len(p1)), (z1[:3], 10), (b"", 10), (z1, 0),
        (b"\x27\xb5\x2f\xfd" + z1[4:], len(p1)),                    # v0.7 magic
        (z1[:4] + bytes([z1[4] | 1]) + z1[5:], len(p1)),            # dictionary id flag
    ]
    bad_sum = bytearray(z1)
    bad_sum[-2] ^= 0x40
    cases.append((bytes(bad_sum), len(p1)))
    frames = zstd_frames([d for _, d, _ in common.corpus_sample()[:5]], 3)
    plains = [d for _, d, _ in common.corpus_sample()[:5]]
    for z, p in zip(frames, plains):
        cases.append((z, len(p) - 7))
        for cut in (len(z) // 3, len(z) - 2):
            cases.append((z[:cut], len(p)))
        for _ in range(10):
            m = bytearray(z)
            for _ in range(int(rng.integers(1, 3))):
                m[int(rng.integers(0, len(m)))] ^= 1 << int(rng.integers(0, 8))
            cases.append((bytes(m), len(p)))
    outs, status, err = gbd.run(OP_ZSTD_DECOMPRESS, [c for c, _ in cases], [cap for _, cap in cases])
    for i, (c, cap) in enumerate(cases):
        est, eoff, eout = _expect(o, c, cap)
        assert status[i] == est, "case %d: gpu status %d oracle %d (gpu offset %d, oracle %d)" % (i, status[i], est, err[i], eoff)
        if est == 0:
            assert outs[i] == eout, "case %d" % i
        else:
            assert err[i] == eoff, "case %d: gpu offset %d oracle %d" % (i, err[i], eoff)


def test_offsets_beyond_28_bits_are_rejected(gbd, o):
    """Offset code 28 expresses offsets up to 0x1FFFFFFC.  A hand-made 20-byte frame (one raw literal, one sequence, RLE tables: literal
    length code 0, offset code 28, match length code 3) whose offset is 0x10000000 + the extra bits: "Input is corrupted" at offset 16
    in the Java decoder (the match starts before the output).  Round 1's one-kernel decoder kept 28 bits of the offset -- such an
    offset wrapped to 0 and the pointer-jumping loop never ended.  The extra bits are varied over the wrap point."""
    base = bytes.fromhex("28b52ffd20045d000008410154001c0003000010")
    cases = [base]
    for b0 in (0, 1, 2, 3, 4, 8, 0x80, 0xFF):
        for b1 in (0, 0x40):
            for b2 in (0x10, 0x11, 0x14, 0x18, 0x1F):
                cases.append(base[:-3] + bytes([b0, b1, b2]))
    for cap in (4, 1 << 16):
        outs, status, err = gbd.run(OP_ZSTD_DECOMPRESS, cases, [cap] * len(cases))
        for i, c in enumerate(cases):
            est, eoff, eout = _expect(o, c, cap)
            assert (status[i], err[i] if est else 0) == (est, eoff), "case %d: gpu %d@%d oracle %d@%d" % (i, status[i], err[i], est, eoff)
            if est == 0:
                assert outs[i] == eout


@pytest.mark.parametrize("level", [1, 3, 9])
def test_libzstd_frames_decode_to_plaintext(gbd, o, level):
    blocks = plain_blocks()
    frames = zstd_frames(blocks, level)
    for pad in (0, 64):
        outs, status, err = gbd.run(OP_ZSTD_DECOMPRESS, frames, [len(b) + pad for b in blocks], unaligned=(pad == 0))
        for i, (b, p, s) in enumerate(zip(blocks, outs, status)):
            assert s == 0, (i, len(b), s, err[i])
            assert p == b, "block %d (len %d)" % (i, len(b))
    for b, z in list(zip(blocks, frames))[:8]:
        assert o.decompress("zstd", z, len(b)) == b


def test_multi_block_frames_and_concatenated_frames(gbd, o):
    whole = b"".join(d for _, d, _ in common.corpus_sample())  # ~1.2 MB: ten 128 KiB blocks with cross-block history
    frames = zstd_frames([whole, whole[:300000], whole[100000:100000 + 131073]], 3)
    cat = frames[1] + frames[2] + zstd_frames([b""], 3)[0] + frames[1]
    plain_cat = whole[:300000] + whole[100000:100000 + 131073] + whole[:300000]
    outs, status, err = gbd.run(OP_ZSTD_DECOMPRESS, frames + [cat], [len(whole), 300000, 131073, len(plain_cat)])
    assert status == [0, 0, 0, 0], (status, err)
    assert outs[0] == whole and outs[1] == whole[:300000] and outs[2] == whole[100000:100000 + 131073] and outs[3] == plain_cat
    assert o.decompress("zstd", cat, len(plain_cat)) == plain_cat


def frame_blocks(f):
    """number of blocks of the (single) frame f"""
    fhd = f[4]
    pos = 5 + (0 if fhd & 0x20 else 1) + ((1 if fhd & 0x20 else 0) if fhd >> 6 == 0 else 1 << (fhd >> 6))
    n = 0
    while True:
        h = int.from_bytes(f[pos:pos + 3], "little")
        pos += 3 + (1 if (h >> 1) & 3 == 1 else h >> 3)
        n += 1
        if h & 1:
            return n


@pytest.mark.timeout(900, method="thread")  # (the default pass size was last changed after the round's GPU minutes: CPU-emulator-verified)
@pytest.mark.parametrize("stream_blocks", [65536, 16])
def test_multi_block_frames_take_the_multi_block_stages(o, stream_blocks):
    """frames of several blocks (ZstdOutputStream / ZstdFrameCompressor / libzstd beyond 128 KiB) go through the
    pipeline's multi-block stages -- window, repeat offsets, Huffman and FSE tables carried from block to block -- and not to the
    one-kernel decoder; with the smallest passes (room for 16 blocks of 128 KiB, 128 block slots) the batch takes several passes and a
    frame of more blocks than a pass has slots falls back."""
    from tests.gpu_harness import GpuBatch
    g = GpuBatch(0, options={"zstd.decompress.stream_blocks": stream_blocks})
    plains = common.multi_block_plains()
    encoders = [("oracle", lambda b: o.compress("zstd", b))] + [("libzstd-%d" % l, (lambda l: lambda b: zstd_frames([b], l)[0])(l)) for l in (1, 3, 9, 19)]
    unfit = 0
    for name, enc in encoders:
        frames = [enc(b) for b in plains]
        for pad in (0, 41):
            outs, status, err = g.run(OP_ZSTD_DECOMPRESS, frames, [len(b) + pad for b in plains], unaligned=(pad == 0))
            assert all(s == 0 for s in status), (name, status, err)
            for i, (b, got) in enumerate(zip(plains, outs)):
                assert got == b, "%s frame %d (len %d)" % (name, i, len(b))
        fits = sum(1 for f in frames if frame_blocks(f) <= 8 * stream_blocks)
        assert g.codec.native.get_stat("zstd.decompress.multiblock_items") == len(frames), name
        assert g.codec.native.get_stat("zstd.decompress.multiblock_fast_items") == fits, name
        assert g.codec.native.get_stat("zstd.decompress.fallback_items") == len(frames) - fits, name
        assert g.codec.native.get_stat("zstd.decompress.multiblock_blocks") == sum(frame_blocks(f) for f in frames if frame_blocks(f) <= 8 * stream_blocks), name
        unfit += len(frames) - fits
    assert (unfit > 0) == (stream_blocks == 16)  # (libzstd level 3 on the mixed data: ~260 blocks)


def test_damaged_multi_block_frames_report_what_the_oracle_reports(gbd, o):
    """whatever the multi-block stages make of a damaged frame -- decode it (the damage may be harmless, or only change bytes) or hand
    it to the one-kernel decoder -- the caller sees the oracle's output, status and offset"""
    rng = np.random.default_rng(23)
    plains = common.multi_block_plains()[1:6]
    cases = []
    for name, enc in (("oracle", lambda b: o.compress("zstd", b)), ("libzstd-3", lambda b: zstd_frames([b], 3)[0])):
        for b in plains:
            f = enc(b)
            for k in range(18):
                m = bytearray(f)
                kind = k % 6
                if kind == 0:
                    m[int(rng.integers(0, len(m)))] ^= 1 << int(rng.integers(0, 8))
                elif kind == 1:
                    m[int(rng.integers(4, min(40, len(m))))] = int(rng.integers(0, 256))
                elif kind == 2:
                    m = m[:int(rng.integers(8, max(9, len(m))))]
                elif kind == 3:
                    m += bytes(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8).tolist())
                elif kind == 4:
                    at = int(rng.integers(0, max(1, len(m) - 16)))
                    m[at:at + 16] = bytes(min(16, len(m) - at))
                else:
                    m[len(m) - 1 - int(rng.integers(0, 6))] ^= 0x10
                cases.append((bytes(m), len(b) if k % 3 else len(b) - int(rng.integers(1, 5000))))
    outs, status, err = gbd.run(OP_ZSTD_DECOMPRESS, [c for c, _ in cases], [cap for _, cap in cases])
    for i, (c, cap) in enumerate(cases):
        est, eoff, eout = _expect(o, c, cap)
        assert status[i] == est, "case %d: gpu status %d oracle %d (gpu offset %d, oracle %d)" % (i, status[i], est, err[i], eoff)
        if est == 0:
            assert outs[i] == eout, "case %d" % i
        else:
            assert err[i] == eoff, "case %d: gpu offset %d oracle %d" % (i, err[i], eoff)


def test_pipeline_small_tiles(o):
    """a batch larger than the pipeline's tile goes through it in several passes (here: tiles of 64 items)"""
    from tests.gpu_harness import GpuBatch
    g = GpuBatch(0, options={"zstd.decompress.tile": 64})
    blocks = [b for b in plain_blocks() if 0 < len(b) <= 131072]
    blocks = (blocks * 6)[:300]
    frames = zstd_frames(blocks, 3)
    outs, status, err = g.run(OP_ZSTD_DECOMPRESS, frames, [len(b) for b in blocks])
    assert all(s == 0 for s in status), status
    assert outs == blocks
    assert g.codec.native.get_stat("zstd.decompress.fallback_items") <= 6 * 12  # only the raw-block / tiny frames


def test_single_block_host_api(o):
    import aircompressor_amd as A
    z1, p1 = common.golden_zstd("with-checksum.zst"), common.golden_zstd("with-checksum")
    d = A.ZstdHipDecompressor()
    out = bytearray(len(p1) + 9)
    n = d.decompress(z1, 0, len(z1), out, 9, len(p1))
    assert n == len(p1) and bytes(out[9:]) == p1
    assert d.get_decompressed_size(z1, 0, len(z1)) == -1
    with pytest.raises(A.MalformedInputException) as e:
        d.decompress(common.golden_zstd("offset-before-start.zst"), 0, 1559, bytearray(1 << 16), 0, 1 << 16)
    assert str(e.value).startswith("Input is corrupted")
    with pytest.raises(A.MalformedInputException) as e:
        z = common.golden_zstd("bad-second-frame.zst")
        d.decompress(z, 0, len(z), bytearray(1 << 16), 0, 1 << 16)
    assert str(e.value).startswith("Invalid magic prefix")


def test_many_frames_full_size_property(gbd, o):
    """1024 x 128 KiB frames (libzstd level 3) -> GPU decode must restore every block (checked by hash)."""
    import hashlib
    rng = np.random.default_rng(77)
    sample = b"".join(d for _, d, _ in common.corpus_sample())
    blocks = []
    for i in range(256):
        off = int(rng.integers(0, len(sample) - 131072))
        blocks.append(sample[off:off + 131072])
    frames = zstd_frames(blocks, 3)
    outs, status, err = gbd.run(OP_ZSTD_DECOMPRESS, frames * 4, [131072] * 1024)
    assert all(s == 0 for s in status)
    want = [hashlib.sha256(b).digest() for b in blocks] * 4
    assert [hashlib.sha256(p).digest() for p in outs] == want
    if gbd.variant == 1:
        # single-block frames must stay on the pipeline: none handed to the one-kernel decoder
        stages = [gbd.codec.native.get_stat("zstd.decompress.fallback_stage%d" % k) for k in range(1, 6)]
        assert gbd.codec.native.get_stat("zstd.decompress.fallback_items") == 0, stages


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_sequence_stage_wavefronts_per_workgroup(o, waves):
    """zstd.decompress.seq_waves: the pipeline's sequence stage with its 64 items a workgroup on 1, 2 or 4 wavefronts (lanes without an item beside lanes
    with one; single-block frames and the multi-block stages) -- every frame restored, nothing handed to the one-kernel decoder."""
    import hashlib
    from tests.gpu_harness import GpuBatch
    rng = np.random.default_rng(78)
    sample = b"".join(d for _, d, _ in common.corpus_sample())
    blocks = []
    for i in range(250):
        off = int(rng.integers(0, len(sample) - 131072))
        blocks.append(sample[off:off + int(rng.integers(2000, 131073))])
    blocks += [sample[:300000], sample[100000:100000 + 500000]]  # (frames of several blocks: the multi-block stages' instantiation)
    frames = zstd_frames(blocks, 3)
    g = GpuBatch(0, options={"zstd.decompress.variant": 1})
    try:
        g.set_option("zstd.decompress.seq_waves", waves)
        outs, status, err = g.run(OP_ZSTD_DECOMPRESS, frames * 16, [len(b) for b in blocks] * 16)
        assert all(s == 0 for s in status)
        want = [hashlib.sha256(b).digest() for b in blocks] * 16
        assert [hashlib.sha256(p).digest() for p in outs] == want
        assert g.codec.native.get_stat("zstd.decompress.fallback_items") == 0
    finally:
        g.set_option("zstd.decompress.seq_waves", DEFAULT_SEQ_WAVES)


@pytest.mark.parametrize("items", [8, 10, 13, 16, 20])
def test_literal_stage_items_per_wavefront(o, items):
    """zstd.decompress.lit_items: the pipeline's literal stage with 8, 10 or 16 items a wavefront (4 KiB of LDS an item: 5 / 4 / 2 wavefronts a CU), with 13
    (the default: symbol bytes and length nibbles apart, 3 KiB an item) and with 20 (16 items of symbol bytes + lengths by symbol) -- every
    frame restored (libzstd's frames and the Java encoder's, single-block and multi-block), nothing handed to the one-kernel decoder."""
    import hashlib
    from tests.gpu_harness import GpuBatch
    rng = np.random.default_rng(79)
    sample = b"".join(d for _, d, _ in common.corpus_sample())
    blocks = []
    for i in range(203):  # (not a multiple of any of the three item counts)
        off = int(rng.integers(0, len(sample) - 131072))
        blocks.append(sample[off:off + int(rng.integers(2000, 131073))])
    blocks += [sample[:300000], sample[100000:100000 + 500000]]
    frames = zstd_frames(blocks, 3)
    frames[:60] = [o.compress("zstd", b) for b in blocks[:60]]
    g = GpuBatch(0, options={"zstd.decompress.variant": 1})
    try:
        g.set_option("zstd.decompress.lit_items", items)
        outs, status, err = g.run(OP_ZSTD_DECOMPRESS, frames * 8, [len(b) for b in blocks] * 8)
        assert all(s == 0 for s in status)
        want = [hashlib.sha256(b).digest() for b in blocks] * 8
        assert [hashlib.sha256(p).digest() for p in outs] == want
        assert g.codec.native.get_stat("zstd.decompress.fallback_items") == 0
    finally:
        g.set_option("zstd.decompress.lit_items", DEFAULT_LIT_ITEMS)


def test_pipeline_takes_java_encoded_frames(gbd, o):
    """Frames as ZstdFrameCompressor writes them (single segment, one block, checksum) stay on the fast path;
    corrupting one sends exactly that item to the one-kernel decoder, which reports the Java-exact error."""
    blocks = plain_blocks()
    blocks = [b for b in blocks if 0 < len(b) <= 131072]
    frames = [o.compress("zstd", b) for b in blocks]
    outs, status, err = gbd.run(OP_ZSTD_DECOMPRESS, frames, [len(b) for b in blocks])
    assert all(s == 0 for s in status), status
    assert outs == blocks
    if gbd.variant == 1:
        raw = sum(1 for f in frames if ((f[4 + 2 + (0 if f[4] >> 6 == 0 else (1 << (f[4] >> 6)) - 1)] >> 1) & 3) != 2)
        assert gbd.codec.native.get_stat("zstd.decompress.fallback_items") <= raw + sum(1 for b in blocks if len(b) < 16)
    big = max(range(len(blocks)), key=lambda i: len(blocks[i]))
    bad = bytearray(frames[big])
    bad[len(bad) // 2] ^= 0x10
    outs, status, err = gbd.run(OP_ZSTD_DECOMPRESS, [frames[big], bytes(bad), frames[big]], [len(blocks[big])] * 3)
    est, eoff, eout = _expect(o, bytes(bad), len(blocks[big]))
    assert status[0] == 0 and status[2] == 0 and outs[0] == blocks[big] and outs[2] == blocks[big]
    assert status[1] == est and (est == 0 or err[1] == eoff)
    if gbd.variant == 1:
        assert gbd.codec.native.get_stat("zstd.decompress.fallback_items") <= 1


# ---- the execute stage's two kernels: the case catalog of tests/zstd_frame_cases.py, and tiles large enough for the per-item choice ----
DEFAULT_RING_PAD = 80  # (the library's default of decompress.ring_pad, restored by the test that changes it)


@pytest.fixture(scope="module")
def frame_cases(o):
    """(cases, expected): the hand frames of the catalog and encoders' frames next to them (the oracle's and libzstd's, text and fragments data, 300 bytes to
    128 KiB: Huffman literals from the arena, FSE tables); expected[pad][i] is the oracle's (status, offset, bytes) for case i at its capacity + pad"""
    text = b"".join(d for _, d, _ in common.corpus_sample()[:3])
    plains = zc.encoder_plains(text, common.synthetic_blocks(21, 1, 131072)[0])
    cases = zc.catalog() + zc.encoder_cases(plains, [("oracle", lambda b: o.compress("zstd", b)), ("libzstd-3", lambda b: zstd_frames([b], 3)[0])])
    expected = {pad: [_expect(o, c.frame, c.capacity(pad)) for c in cases] for pad in (0, 64)}
    for pad in (0, 64):
        for c, (est, _, eout) in zip(cases, expected[pad]):
            assert (est != 0) == c.malformed and (c.malformed or eout == c.plain), c.name  # (the catalog's own verdict is the oracle's: also tests/test_zstd_frame_cases.py)
    return cases, expected


def _run_catalog(g, cases, expected, pad):
    """the catalog through g at capacity + pad: status, offset and bytes as the oracle has them; exactly the malformed cases handed to the one-kernel decoder,
    all of them by the execute stage (a valid frame that leaves the fast path tests nothing here)"""
    outs, status, err = g.run(OP_ZSTD_DECOMPRESS, [c.frame for c in cases], [c.capacity(pad) for c in cases], unaligned=(pad == 0))
    for i, (c, (est, eoff, eout)) in enumerate(zip(cases, expected[pad])):
        assert status[i] == est, "%s: gpu status %d oracle %d (gpu offset %d, oracle %d)" % (c.name, status[i], est, err[i], eoff)
        if est == 0:
            assert len(outs[i]) == len(eout) and outs[i] == eout, c.name
        else:
            assert err[i] == eoff, "%s: gpu offset %d oracle %d" % (c.name, err[i], eoff)
    stat = g.codec.native.get_stat
    stages = [stat("zstd.decompress.fallback_stage%d" % k) for k in range(1, 7)]
    n_bad = sum(1 for c in cases if c.malformed)
    assert stat("zstd.decompress.fallback_items") == n_bad, stages
    assert stat("zstd.decompress.fallback_stage4") == sum(1 for c in cases if c.stage == 4) == n_bad, stages


@pytest.mark.parametrize("exec_mode", [0, 1], ids=["ring-executor", "record-executor"])
def test_catalog_under_each_executor(o, frame_cases, exec_mode):
    """zstd.decompress.exec 0 / 1: every item of the catalog on the ring executor (zstd_pipe_execute_kernel) / on the record executor, at exact capacities with
    unaligned outputs and with 64 bytes of slack"""
    from tests.gpu_harness import GpuBatch
    cases, expected = frame_cases
    g = GpuBatch(0, options={"zstd.decompress.variant": 1, "zstd.decompress.exec": exec_mode})
    _run_catalog(g, cases, expected, 0)
    _run_catalog(g, cases, expected, 64)


def test_catalog_on_the_ring_executor_without_a_staging_area(o, frame_cases):
    """decompress.ring_pad 0: the ring executor gets no LDS staging area for far matches (it has one from 64 bytes of pad on; the default is 80) and reads them
    from its flushed output piece by piece -- the other branch of achip_rings.h copy_match"""
    from tests.gpu_harness import GpuBatch
    cases, expected = frame_cases
    g = GpuBatch(0, options={"zstd.decompress.variant": 1, "zstd.decompress.exec": 0})
    try:
        g.set_option("decompress.ring_pad", 0)
        _run_catalog(g, cases, expected, 0)
        _run_catalog(g, cases, expected, 64)
    finally:
        g.set_option("decompress.ring_pad", DEFAULT_RING_PAD)


def header_form_items(o):
    """(frames, plaintexts): the catalog's valid frames and the encoder's frames of zc.form_plains() -- between them every literals header and every form of the
    sequence count the format has (tests/test_zstd_frame_cases.py counts them)"""
    cases = [c for c in zc.catalog() if not c.malformed]
    forms = zc.form_plains()
    return [c.frame for c in cases] + [o.compress("zstd", p) for _, p in forms], [c.plain for c in cases] + [p for _, p in forms]


def header_forms_through_the_one_kernel_decoder(g, o):
    """(also run on the CPU emulator: tools/hostemu/check_serial.py)"""
    frames, plains = header_form_items(o)
    g.set_option("zstd.decompress.variant", 0)
    try:
        outs, status, err = g.run(OP_ZSTD_DECOMPRESS, frames, [len(p) for p in plains], unaligned=True)
    finally:
        g.set_option("zstd.decompress.variant", 1)
    wrong = [(i, status[i], err[i]) for i in range(len(frames)) if status[i] != 0 or outs[i] != plains[i]]
    assert not wrong, wrong[:8]


def test_every_header_form_through_the_one_kernel_decoder_and_the_size_query(gb, o):
    """the two readers that state the Java-exact walk (zstd_decompress.hip, decoded_size.hip), on every header form: the one-kernel decoder gives the plaintext at exact capacity, the size
    query its length"""
    from tests.test_gpu_decoded_size import size_on_gpu
    header_forms_through_the_one_kernel_decoder(gb, o)
    frames, plains = header_form_items(o)
    size, status, err, _ = size_on_gpu(gb, OP_ZSTD_DECOMPRESS, frames)
    wrong = [(i, int(status[i]), int(size[i]), len(plains[i])) for i in range(len(frames)) if status[i] != 0 or size[i] != len(plains[i])]
    assert not wrong, wrong[:8]
    assert (err == 0).all()


LARGE_TILE = 32768


@pytest.fixture(scope="module")
def tile_pools(frame_cases):
    """the catalog's small cases (at most 4 KiB of output, malformed ones and both checksum settings among them) as (frame, capacity, expected, counted as long),
    apart by what the sequence stage counts them as: an item is counted as a long-sequence item when it HAS sequences and its capacity is at least 80 bytes a sequence"""
    cases, expected = frame_cases
    K = zc.kernel_constants()
    assert LARGE_TILE > K["ALL_RECORDS_MAX_ITEMS"]  # (a tile of at most that many items runs the record executor whatever it holds)
    pools = {True: [], False: []}
    far = 0
    for c, e in zip(cases, expected[0]):
        if c.cap <= 4096:
            pools[zc.counted_long(c.cap, c.nseq, K)].append((c.frame, c.cap, e, c.malformed))
            far += "far=prefetch-lane>0" in c.tags and zc.counted_long(c.cap, c.nseq, K)
    assert len(pools[True]) + len(pools[False]) <= 400 and min(len(pools[True]), len(pools[False])) >= 20
    assert sum(1 for p in pools[True] if p[3]) >= 3 and sum(1 for p in pools[False] if p[3]) >= 3
    assert far >= 2  # (long-sequence frames whose far matches the ring executor requests ahead, from lanes other than a group's first)
    return pools, K


def _large_tile(pools, n_long, extra=()):
    """LARGE_TILE items, n_long of them from the long pool, spread evenly among the others item by item (every workgroup of either execute kernel holds both
    kinds); extra: items that take the place of every 32nd one"""
    items = []
    taken = {True: 0, False: 0}
    for i in range(LARGE_TILE):
        long = (i + 1) * n_long // LARGE_TILE != i * n_long // LARGE_TILE
        items.append(pools[long][taken[long] % len(pools[long])])
        taken[long] += 1
    for k, e in enumerate(extra):
        items[32 * k + 5] = e
    return items


def _run_large_tile(g, items, K):
    """runs the items; every one as the oracle has it, exactly the malformed ones handed to the one-kernel decoder; returns the tile's long-item count as the
    library reports it, after comparing it with the count made here from the frames' sequence counts and capacities"""
    outs, status, err = g.run(OP_ZSTD_DECOMPRESS, [it[0] for it in items], [it[1] for it in items], unaligned=True)
    for i, (frame, cap, (est, eoff, eout), malformed) in enumerate(items):
        assert status[i] == est, "item %d: gpu status %d oracle %d (gpu offset %d, oracle %d)" % (i, status[i], est, err[i], eoff)
        if est == 0:
            assert len(outs[i]) == len(eout) and outs[i] == eout, "item %d" % i
        else:
            assert err[i] == eoff, "item %d: gpu offset %d oracle %d" % (i, err[i], eoff)
    stat = g.codec.native.get_stat
    assert stat("zstd.decompress.fallback_items") == sum(1 for it in items if it[3]), [stat("zstd.decompress.fallback_stage%d" % k) for k in range(1, 7)]
    want_long = sum(1 for frame, cap, _, _ in items if zc.counted_long(cap, zc.sequence_count(frame), K))
    assert stat("zstd.decompress.long_items") == want_long
    return want_long


def test_large_tile_splits_its_items_between_the_executors(o, tile_pools):
    """No option set: a tile of 32 768 items (the sequence stage in full 64-item workgroups) with 26 000 long-sequence items among 6 768 others runs the former on
    the ring executor and the latter on the record executor; with 20 000 -- fewer than the rule asks for -- all on the record executor.  zstd.decompress.long_items
    says which of the two happened."""
    from tests.gpu_harness import GpuBatch
    pools, K = tile_pools
    g = GpuBatch(0)
    n = _run_large_tile(g, _large_tile(pools, 26000), K)
    assert n == 26000 >= K["RINGS_MIN_LONG_ITEMS"] and LARGE_TILE - n >= 4096
    n = _run_large_tile(g, _large_tile(pools, 20000), K)
    assert n == 20000 < K["RINGS_MIN_LONG_ITEMS"]


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_large_tile_sequence_stage_wavefronts_per_workgroup(o, tile_pools, waves):
    """zstd.decompress.seq_waves on a tile whose sequence-stage workgroups are full (64 items each: tiles of 16 384 items and more), both executors behind it"""
    from tests.gpu_harness import GpuBatch
    pools, K = tile_pools
    g = GpuBatch(0)
    try:
        g.set_option("zstd.decompress.seq_waves", waves)
        assert _run_large_tile(g, _large_tile(pools, 26000), K) >= K["RINGS_MIN_LONG_ITEMS"]
    finally:
        g.set_option("zstd.decompress.seq_waves", DEFAULT_SEQ_WAVES)


def test_capacity_stands_in_for_size_in_a_large_tile(o, frame_cases, tile_pools):
    """The per-item rule sees the capacity, not the output size: text frames (a sequence every 10 .. 15 bytes) handed over with 100 times the capacity they need
    count as long-sequence items and, in a tile with enough of those, run on the ring executor -- plaintext and the exact length all the same"""
    from tests.gpu_harness import GpuBatch
    cases, expected = frame_cases
    pools, K = tile_pools
    text = [(c.frame, 100 * len(c.plain), (0, 0, c.plain), False) for c in cases if "-text-" in c.name and len(c.plain) <= 2500]
    assert len(text) == 6
    for frame, cap, _, _ in text:
        n = zc.sequence_count(frame)
        assert not zc.counted_long(cap // 100, n, K) and zc.counted_long(cap, n, K)
    g = GpuBatch(0)
    items = _large_tile(pools, 26000, extra=[text[k % len(text)] for k in range(LARGE_TILE // 32)])
    assert _run_large_tile(g, items, K) >= K["RINGS_MIN_LONG_ITEMS"]


# ---- encoder (level 3), rows a11-a14 -------------------------------------------------------------------------
OP_ZSTD_COMPRESS = 5


def encoder_inputs():
    sample = [d for _, d, _ in common.corpus_sample()]
    blocks = [d for _, d in common.HAND_CASES]
    blocks += sample
    blocks += [sample[i] + sample[i + 1] for i in range(0, len(sample) - 1, 2)]   # 128 KiB: one full block
    blocks += common.synthetic_blocks(31, 24)
    blocks.append(b"".join(sample[:5]) + b"tail")                                  # 3 blocks sharing tables / repcodes / Huffman reuse
    blocks.append(b"".join(sample[3:9]))                                           # > 256 KiB: default parameter row, 2^17 long table
    blocks.append(common.golden_zstd("large-rle"))
    blocks.append(common.golden_zstd("incompressible"))
    base = sample[0]
    blocks += [base[:n] for n in (1, 2, 6, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 16383, 16384, 16385)]
    return blocks


@pytest.mark.parametrize("variant", [3, 0, 1, 2], ids=["two-kernel-window-match-finder", "two-kernel-batch-probe", "two-kernel-serial-probe", "one-kernel"])
def test_zstd_compress_is_bit_exact_with_oracle(gb, o, variant):
    blocks = encoder_inputs()
    blocks += [b for b in common.synthetic_blocks(77, 12)]   # RandomGenerator-style data: long literal runs, many same-hash positions per batch
    caps = [o.max_compressed_length("zstd", len(b)) for b in blocks]
    gb.set_option("zstd.compress.variant", variant)
    try:
        outs, status, _ = gb.run(OP_ZSTD_COMPRESS, blocks, caps)
    finally:
        gb.set_option("zstd.compress.variant", 3)
    assert all(s == 0 for s in status), status
    for i, (b, z) in enumerate(zip(blocks, outs)):
        assert z == o.compress("zstd", b, caps[i]), "block %d (len %d): gpu %d bytes" % (i, len(b), len(z))
    # and the GPU decoder restores the plaintext from the GPU encoder's frames
    plain, status, err = gb.run(OP_ZSTD_DECOMPRESS, outs, [max(len(b), 1) for b in blocks])
    for i, (b, p, s) in enumerate(zip(blocks, plain, status)):
        if len(b) == 0:
            continue
        assert s == 0 and p == b, (i, s, err[i])


def test_zstd_compress_pinned_hashes_and_third_party_decoder(gb, o):
    import hashlib
    import pyarrow as pa
    sample = common.corpus_sample()
    blocks = [d for _, d, _ in sample]
    outs, status, _ = gb.run(OP_ZSTD_COMPRESS, blocks, [o.max_compressed_length("zstd", len(b)) for b in blocks])
    assert all(s == 0 for s in status)
    codec = pa.Codec("zstd")
    for (name, d, e), z in zip(sample, outs):
        assert hashlib.sha256(z).hexdigest() == e["zstd"]["sha256"], name       # committed hash of the oracle's stream
        assert codec.decompress(z, decompressed_size=len(d)).to_pybytes() == d  # libzstd accepts the frame


def test_zstd_compress_output_too_small(gb, o):
    b = common.corpus_sample()[0][1]
    cap = o.max_compressed_length("zstd", len(b))
    outs, status, _ = gb.run(OP_ZSTD_COMPRESS, [b, b, b], [10, cap, 20000])
    assert status[1] == 0 and outs[1] == o.compress("zstd", b, cap)
    for i, c in ((0, 10), (2, 20000)):
        try:
            expect = o.compress("zstd", b, c)
            assert status[i] == 0 and outs[i] == expect
        except OracleError as e:
            assert status[i] == e.status


def test_zstd_host_api_round_trip(o):
    import aircompressor_amd as A
    data = common.corpus_sample()[2][1]
    comp, decomp = A.ZstdHipCompressor(), A.ZstdHipDecompressor()
    cap = comp.max_compressed_length(len(data))
    assert cap == o.max_compressed_length("zstd", len(data))
    out = bytearray(cap)
    n = comp.compress(data, 0, len(data), out, 0, cap)
    assert bytes(out[:n]) == o.compress("zstd", data, cap)
    assert decomp.get_decompressed_size(out, 0, n) == len(data)
    back = bytearray(len(data))
    assert decomp.decompress(out, 0, n, back, 0, len(data)) == len(data) and bytes(back) == data
    with pytest.raises(A.IllegalArgumentException):
        comp.compress(data, 0, len(data), bytearray(5), 0, 5)
