"""An emulator-backed stand-in for tests/gpu_harness.GpuBatch: the same run(op, blocks, caps) -> (outputs, status, offsets), with the
wavefront-per-item kernels of tools/hostemu/libemu_serial.so doing the work on the CPU.  With it the GPU parity tests of the container
readers and of the Zstd decoder -- the reference's LZ4 frame vectors, every branch of the Hadoop readers, corruption with the oracle's
status and offset -- run without a GPU (tools/hostemu/check_serial.py), against the variant-0 kernels (a wavefront per item)."""
import ctypes, os, sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib  # noqa: E402

ROOT = emulib.ROOT


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Layout:
    """One batch as every emulator entry point takes it: the items in one source buffer over `filler`, one destination buffer of `prefill` with a slot of
    caps[i] bytes per item, and the per-item arrays.  src_gap(i, length) / dst_gap(i, capacity) say how many bytes lie between the end of item i (of its capacity)
    and the start of the next -- which is what sets the misalignments a script covers --, src_lead / dst_lead where the first one starts; 64 more bytes end each
    buffer.  fresh: what out_len, status and err hold before the call."""

    def __init__(self, items, caps, src_gap, dst_gap, src_lead=64, dst_lead=64, filler=0x5A, prefill=0xA5, fresh=(-7, -7, 0)):
        self.n, self.prefill = len(items), prefill
        self.src_len = np.array([len(b) for b in items], dtype=np.int32)
        self.dst_cap = np.array(caps, dtype=np.int32).reshape(self.n)
        self.src_off, end = self._place(src_lead, self.src_len, src_gap)
        self.src = np.full(end + 64, filler, dtype=np.uint8)
        for off, b in zip(self.src_off, items):
            if len(b):
                self.src[off:off + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
        self.dst_off, end = self._place(dst_lead, self.dst_cap, dst_gap)
        self.dst = np.full(end + 64, prefill, dtype=np.uint8)
        self.out_len = np.full(self.n, fresh[0], dtype=np.int32)
        self.status = np.full(self.n, fresh[1], dtype=np.int32)
        self.err = np.full(self.n, fresh[2], dtype=np.int64)

    @staticmethod
    def _place(pos, lengths, gap):
        off = np.zeros(len(lengths), dtype=np.int64)
        for i, length in enumerate(lengths):
            off[i] = pos
            pos += int(length) + gap(i, int(length))
        return off, pos

    def args(self):
        """src, src_off, src_len, dst, dst_off, dst_cap, out_len, status, err, n: the ten arguments every entry point has in this order"""
        return tuple(P(a) for a in (self.src, self.src_off, self.src_len, self.dst, self.dst_off, self.dst_cap, self.out_len, self.status, self.err)) + (self.n,)

    def check_guards(self, what="item"):
        """nothing but an item's slot may have changed: the band in front of the first slot, every byte between a slot's end and the next slot, the band behind the last"""
        lo = 0
        for i in range(self.n):
            assert (self.dst[lo:self.dst_off[i]] == self.prefill).all(), ("%s %d: wrote beyond its capacity" % (what, i - 1)) if i else "wrote in front of the destination buffer's first slot"
            lo = int(self.dst_off[i]) + int(self.dst_cap[i])
        assert (self.dst[lo:] == self.prefill).all(), ("%s %d: wrote beyond its capacity" % (what, self.n - 1)) if self.n else "wrote into an empty batch's destination"

    def outputs(self):
        return [self.dst[self.dst_off[i]:self.dst_off[i] + max(int(self.out_len[i]), 0)].tobytes() for i in range(self.n)]


def run_windows(call, windows, flags, caps):
    """The window kernels' batch (achip_window_*): the layout with the window calls' per-item arrays on top; call(flags, *the ten, consumed, stop, need) -> 0.
    Returns the dicts the loops of tests/window_cases.py want."""
    lay = Layout(windows, caps, lambda i, n: 3, lambda i, c: 16, fresh=(-7, -7, -7))
    fl = np.array(flags, dtype=np.int32)
    stop = np.full(lay.n, -7, dtype=np.int32)
    consumed, need = (np.full(lay.n, -7, dtype=np.int64) for _ in range(2))
    r = call(P(fl), *lay.args(), P(consumed), P(stop), P(need))
    assert r == 0, r
    lay.check_guards("window")
    return [{"consumed": int(consumed[i]), "out": out, "stop": int(stop[i]), "need": int(need[i]), "status": int(lay.status[i]), "err": int(lay.err[i])}
            for i, out in enumerate(lay.outputs())]


class _Native:
    def __init__(self, owner):
        self.owner = owner

    def set_option(self, k, v):
        self.owner.options[k] = v

    def get_stat(self, name):
        return -1


class _Codec:
    def __init__(self, owner):
        self.native = _Native(owner)


class NotEmulated(Exception):
    pass


class EmuBatch:
    variant = 0  # (tests/test_gpu_zstd.py: the one-kernel decoder)

    def __init__(self, options=None):
        self.lib = emulib.load("serial")
        self.options = dict(options or {})
        self.codec = _Codec(self)

    def set_option(self, k, v):
        self.options[k] = v

    def _call(self, op, src, src_off, src_len, dst, dst_off, caps, out_len, status, err, n):
        return self.lib.emu_serial(op, int(self.options.get("hadoop.buffer_size", 262144)), src, src_off, src_len, dst, dst_off, caps, out_len, status, err, n)

    def run(self, op, blocks, caps, fill=0xA5, unaligned=False):
        gap = (lambda i, n: 0) if unaligned else (lambda i, n: -n % 16)
        lay = Layout(blocks, caps, gap, gap, prefill=fill)
        if lay.n:
            if isinstance(op, (list, tuple, np.ndarray)):
                raise NotEmulated("mixed batch")
            r = self._call(int(op), *lay.args())
            if r != 0:
                raise NotEmulated("op %d" % op)
        lay.check_guards("block")
        return lay.outputs(), lay.status.tolist(), lay.err.tolist()


class EmuAllBatch(EmuBatch):
    """The same over libemu_all.so (every decode kernel, soft order points): whole product paths -- the default variants and the experimental
    ones, chosen by the same context options the GPU tests set."""

    def __init__(self, options=None):
        self.lib = emulib.load("all")
        self.options = dict(options or {})
        self.codec = _Codec(self)
        self.variant = self.options.get("zstd.decompress.variant", 1)
        self.counters = np.zeros(64, dtype=np.int32)
        self.codec.native.get_stat = self.get_stat

    def get_stat(self, name):
        words = {"zstd.decompress.fallback_items": 0, "zstd.decompress.multiblock_items": 40, "zstd.decompress.multiblock_blocks": 41, "zstd.decompress.multiblock_fast_items": 42,
                 "zstd.decompress.long_items": 18}
        if name in words:
            return int(self.counters[words[name]])
        if name.startswith("zstd.decompress.fallback_stage"):
            return int(self.counters[32 + int(name[-1])])
        return -1

    def _call(self, op, src, src_off, src_len, dst, dst_off, caps, out_len, status, err, n):
        a = (src, src_off, src_len, dst, dst_off, caps, out_len, status, err, n)
        o = self.options
        if op == 0:
            return self.lib.emu_batch({1: 44, 7: 24}.get(o.get("lz4.decompress.variant", 1), 44), *a)
        if op == 2:
            return self.lib.emu_batch({1: 54, 7: 34}.get(o.get("snappy.decompress.variant", 1), 54), *a)
        if op == 4:
            self.variant = o.get("zstd.decompress.variant", 1)
            return self.lib.emu_zstd_full(*a, int(self.variant), int(o.get("zstd.decompress.stream_blocks", 65536)), P(self.counters))
        if op == 6:
            return self.lib.emu_lz4frame(int(o.get("lz4frame.decompress.variant", 2)), *a)
        if op == 8:
            return self.lib.emu_snappyframed(int(o.get("snappyframed.decompress.variant", 3)), *a)
        if op in (10, 12):
            return self.lib.emu_hadoop(0, 1 if op == 12 else 0, int(o.get("hadoop.buffer_size", 262144)), int(o.get("hadoop.decompress.variant", 3)), *a)
        return -1
