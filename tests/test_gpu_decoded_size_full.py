"""achip_decoded_size_batch at size: the headline shape -- 262 144 x 64 KiB oracle-written LZ4 blocks as tests/test_gpu_baseline_size.py builds them, and the Snappy
twin -- through the lane-per-block walk, and one mixed-length batch of 16 384 LZ4 blocks through the wavefront-per-block walk.  Every size is exact."""
import numpy as np
import pytest

from tests import common, oracle_lib
from tests.test_gpu_baseline_size import _pool

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


def _size_tiled(op, comp, reps):
    """sizes len(comp) x reps items (the pool tiled `reps` times at distinct addresses); returns outSize as a (reps, len(comp)) device tensor"""
    import torch
    from tests.gpu_harness import GpuBatch
    g = GpuBatch(0)
    k = len(comp)
    n = k * reps
    lens = np.array([len(c) for c in comp], dtype=np.int32)
    pad = (lens.astype(np.int64) + 15) // 16 * 16
    off = np.cumsum(pad) - pad
    tile_bytes = int(pad.sum())
    tile = np.zeros(tile_bytes, dtype=np.uint8)
    for at, c in zip(off, comp):
        tile[at:at + len(c)] = np.frombuffer(c, dtype=np.uint8)
    d_src = torch.from_numpy(tile).to(g.dev).repeat(reps)
    src_off = (np.arange(reps, dtype=np.int64)[:, None] * tile_bytes + off[None, :]).reshape(-1)
    a_so, a_sl = torch.from_numpy(src_off).to(g.dev), torch.from_numpy(np.tile(lens, reps)).to(g.dev)
    size = torch.full((n,), -7, dtype=torch.int64, device=g.dev)
    st = torch.full((n,), -7, dtype=torch.int32, device=g.dev)
    eo = torch.full((n,), -7, dtype=torch.int64, device=g.dev)
    torch.cuda.synchronize()
    g.codec.decoded_sizes(op, d_src, a_so, a_sl, size, st, eo, n)
    g.codec.synchronize()
    assert int((st != 0).sum().item()) == 0, "statuses: %s" % st[st != 0][:8].tolist()
    return size.view(reps, k)


@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_headline_shape_262144_blocks_of_64_kib(o, codec):
    import aircompressor_amd as A
    plain = _pool(65536, 512, 11)
    comp = [o.compress(codec, b) for b in plain]
    size = _size_tiled(A.OP_LZ4_DECOMPRESS if codec == "lz4" else A.OP_SNAPPY_DECOMPRESS, comp, 512)
    assert size.numel() == 262144 and int((size != 65536).sum().item()) == 0


def test_16384_mixed_length_blocks_take_the_wavefront_walk(o):
    import torch
    import aircompressor_amd as A
    rng = np.random.default_rng(5)
    files = [d for _, d in sorted(common.corpus_full().items()) if len(d) > 300000]
    plain = []
    for i in range(256):
        data = files[i % len(files)]
        n = int(rng.integers(1, 262144)) if i % 4 else int(rng.integers(1, 600))
        at = int(rng.integers(0, len(data) - n))
        plain.append(bytes(data[at:at + n]))
    comp = [o.compress("lz4", p) for p in plain]
    size = _size_tiled(A.OP_LZ4_DECOMPRESS, comp, 64)
    want = torch.from_numpy(np.array([len(p) for p in plain], dtype=np.int64)).to(size.device)
    assert size.numel() == 16384 and bool((size == want.unsqueeze(0)).all().item())
