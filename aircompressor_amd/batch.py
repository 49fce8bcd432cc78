"""Batched, device-resident entry points (the hot path): thin wrapper over achip_*_batch.

Buffers are anything exposing `data_ptr()` (torch tensors on the HIP device) or raw integer
device addresses; no torch import here -- PyTorch is only the callers' allocator.
Work is sharded over GPUs one process per GPU by `partition_blocks` (contiguous, balanced
by bytes): blocks are independent, so there is no collective on the data path.
"""
import ctypes

import numpy as np

from . import native
from .native import HipNative

OP_LZ4_DECOMPRESS, OP_LZ4_COMPRESS, OP_SNAPPY_DECOMPRESS, OP_SNAPPY_COMPRESS, OP_ZSTD_DECOMPRESS, OP_ZSTD_COMPRESS, OP_LZ4FRAME_DECOMPRESS, OP_LZ4FRAME_COMPRESS, OP_SNAPPYFRAMED_DECOMPRESS, OP_SNAPPYFRAMED_COMPRESS, OP_LZ4HADOOP_DECOMPRESS, OP_LZ4HADOOP_COMPRESS, OP_SNAPPYHADOOP_DECOMPRESS, OP_SNAPPYHADOOP_COMPRESS, OP_ZSTDSTREAM_COMPRESS = range(15)
OP_LZO_DECOMPRESS, OP_LZO_COMPRESS = 16, 17  # (15 is no op: even ops decode, odd ops encode)
_FN = {
    OP_LZ4_DECOMPRESS: "achip_lz4_decompress_batch",
    OP_LZ4_COMPRESS: "achip_lz4_compress_batch",
    OP_SNAPPY_DECOMPRESS: "achip_snappy_decompress_batch",
    OP_SNAPPY_COMPRESS: "achip_snappy_compress_batch",
    OP_ZSTD_DECOMPRESS: "achip_zstd_decompress_batch",
    OP_ZSTD_COMPRESS: "achip_zstd_compress_batch",
    OP_LZ4FRAME_DECOMPRESS: "achip_lz4frame_decompress_batch",
    OP_LZ4FRAME_COMPRESS: "achip_lz4frame_compress_batch",
    OP_SNAPPYFRAMED_DECOMPRESS: "achip_snappyframed_decompress_batch",
    OP_SNAPPYFRAMED_COMPRESS: "achip_snappyframed_compress_batch",
    OP_LZ4HADOOP_DECOMPRESS: "achip_lz4hadoop_decompress_batch",
    OP_LZ4HADOOP_COMPRESS: "achip_lz4hadoop_compress_batch",
    OP_SNAPPYHADOOP_DECOMPRESS: "achip_snappyhadoop_decompress_batch",
    OP_SNAPPYHADOOP_COMPRESS: "achip_snappyhadoop_compress_batch",
    OP_ZSTDSTREAM_COMPRESS: "achip_zstdstream_compress_batch",
    OP_LZO_DECOMPRESS: "achip_lzo_decompress_batch",
    OP_LZO_COMPRESS: "achip_lzo_compress_batch",
}


def _ptr(x):
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return int(x)


def partition_blocks(weights, n_parts):
    """Contiguous split of block indices balanced by `weights` (achip_partition_blocks)."""
    lib = native.load_library()
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.int64))
    starts = np.zeros(n_parts + 1, dtype=np.int32)
    r = lib.achip_partition_blocks(w.ctypes.data, len(w), n_parts, starts.ctypes.data)
    if r < 0:
        native.raise_for_status(r)
    return starts


class HipMultiContextCodec:
    """ONE process, several contexts (normally one per device), one host thread per context inside the library: the Python twin of
    java/io/airlift/compress/v3/hip/HipBatchCodec.java's `run` (N contexts, N threads, byte-balanced contiguous slices) over
    achip_multi_batch_host.  Host numpy arrays in and out; units are independent, the slices exchange nothing."""

    def __init__(self, devices=None, contexts=None):
        self.lib = native.load_library()
        if contexts is None:
            if devices is None:
                devices = list(range(max(self.lib.achip_device_count(), 0)))
            contexts = [HipNative(d) for d in devices]
        if not contexts:
            raise native.HipUnavailableError("no HIP device visible: the Hip codecs cannot run (no CPU fallback)")
        self.contexts = list(contexts)
        self._handles = (ctypes.c_void_p * len(self.contexts))(*[c.ctx for c in self.contexts])
        self.slice_starts = None

    def run_host(self, op, src, src_off, src_len, dst, dst_off, dst_cap):
        """`op`: one OP_* for every item, or a sequence of one OP_* per item (a mixed batch, BASELINE configs[4])."""
        n = len(src_off)
        ops = None
        if not np.isscalar(op):
            ops = np.ascontiguousarray(op, dtype=np.int32)
            if len(ops) != n:
                raise native.IllegalArgumentException("ops must have one entry per item")
        src = np.ascontiguousarray(src, dtype=np.uint8)
        src_off = np.ascontiguousarray(src_off, dtype=np.int64)
        src_len = np.ascontiguousarray(src_len, dtype=np.int32)
        dst_off = np.ascontiguousarray(dst_off, dtype=np.int64)
        dst_cap = np.ascontiguousarray(dst_cap, dtype=np.int32)
        out_len = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        err_off = np.zeros(n, dtype=np.int64)
        starts = np.zeros(len(self.contexts) + 1, dtype=np.int32)
        r = self.lib.achip_multi_batch_host(self._handles, len(self.contexts), 0 if ops is not None else int(op), ops.ctypes.data if ops is not None else None,
                                            src.ctypes.data, src_off.ctypes.data, src_len.ctypes.data, dst.ctypes.data, dst_off.ctypes.data, dst_cap.ctypes.data,
                                            out_len.ctypes.data, status.ctypes.data, err_off.ctypes.data, n, starts.ctypes.data)
        if r < 0:
            native.raise_for_status(r)
        self.slice_starts = starts
        return out_len, status, err_off

    def close(self):
        for c in self.contexts:
            c.close()


class HipBatchCodec:
    def __init__(self, device=0, native_ctx=None):
        self.native = native_ctx if native_ctx is not None else HipNative(device)
        self.lib = self.native.lib

    def launch(self, op, src, src_off, src_len, dst, dst_off, dst_cap, out_len, status, err_off, n_blocks):
        """Asynchronous on the context stream; all arguments device-accessible."""
        fn = getattr(self.lib, _FN[op])
        r = fn(self.native.ctx, _ptr(src), _ptr(src_off), _ptr(src_len), _ptr(dst), _ptr(dst_off), _ptr(dst_cap),
               _ptr(out_len), _ptr(status), _ptr(err_off), int(n_blocks))
        if r < 0:
            native.raise_for_status(r)

    def launch_mixed(self, ops, src, src_off, src_len, dst, dst_off, dst_cap, out_len, status, err_off, n_blocks):
        """A mixed batch (BASELINE configs[4]): item i is processed by ops[i] (OP_*), any interleaving.  `ops` is a HOST int32 array;
        everything else is device-accessible as for `launch`.  The items are bucketed by codec op inside the library (each kernel
        launch is homogeneous) and the results come back in item order.  Asynchronous on the context stream."""
        ops = np.ascontiguousarray(ops, dtype=np.int32)
        if len(ops) != int(n_blocks):
            raise native.IllegalArgumentException("ops must have one entry per item")
        r = self.lib.achip_mixed_batch(self.native.ctx, ops.ctypes.data, _ptr(src), _ptr(src_off), _ptr(src_len), _ptr(dst), _ptr(dst_off), _ptr(dst_cap),
                                       _ptr(out_len), _ptr(status), _ptr(err_off), int(n_blocks))
        if r < 0:
            native.raise_for_status(r)

    def synchronize(self):
        self.native.synchronize()

    def set_lz4frame_linked_blocks(self, accept):
        """achip_ctx_set_lz4frame_linked_blocks for this codec's context: True = OP_LZ4FRAME_DECOMPRESS items (of launch, launch_mixed, run_host, run_host_mixed,
        decoded_sizes, decompress_unsized) may be frames of linked blocks; False (the default) = they fail as the Java reader's do"""
        self.native.set_lz4frame_linked_blocks(accept)

    def decoded_sizes(self, op, src, src_off, src_len, out_size, status, err_off, n_blocks):
        """achip_decoded_size_batch: out_size[i] (int64) = what item i decodes to under decode op `op`, found on the device without decoding; status[i] /
        err_off[i] report a structural fault (out_size[i] is then 0).  Asynchronous on the context stream; all arguments device-accessible."""
        r = self.lib.achip_decoded_size_batch(self.native.ctx, int(op), _ptr(src), _ptr(src_off), _ptr(src_len), _ptr(out_size), _ptr(status), _ptr(err_off), int(n_blocks))
        if r < 0:
            native.raise_for_status(r)

    def plan_outputs(self, out_size, status, n_blocks, align, dst_off, dst_cap, total):
        """achip_plan_outputs: dst_cap[i] = out_size[i], dst_off[i] = the running sum of the capacities, each rounded up to `align`; items with a status or
        beyond INT32_MAX take no room.  total (two int64): bytes of output, items left out.  Asynchronous on the context stream."""
        r = self.lib.achip_plan_outputs(self.native.ctx, _ptr(out_size), _ptr(status), int(n_blocks), int(align), _ptr(dst_off), _ptr(dst_cap), _ptr(total))
        if r < 0:
            native.raise_for_status(r)

    def decompress_unsized(self, op, src, src_off, src_len, n_blocks, alloc, align=16):
        """Decodes a device-resident batch whose decoded sizes nobody knows: size, plan, ONE 16-byte readback (the total -- the only point where this call waits
        for the device), `alloc(total)`, decode.  `alloc(nbytes)` is the caller's device allocator (it returns something with data_ptr(), or an address): it gives
        the output buffer and the per-item arrays, all of which come back in the result:
          dst, total_bytes, left_out                     the output, its planned size, the items sizing left out of it
          dst_off, dst_cap, out_len, status, err_off     the decode's arrays (int64 / int32 / int32 / int32 / int64), the decode still in flight on the stream
          out_size, size_status, size_err_off            what sizing said (int64 / int32 / int64): an item with size_status != 0 was given no room
        """
        n = int(n_blocks)
        wide, narrow = max(8 * n, 16), max(4 * n, 16)
        r = {"out_size": alloc(wide), "size_status": alloc(narrow), "size_err_off": alloc(wide), "dst_off": alloc(wide), "dst_cap": alloc(narrow),
             "out_len": alloc(narrow), "status": alloc(narrow), "err_off": alloc(wide)}
        total = alloc(16)
        self.decoded_sizes(op, src, src_off, src_len, r["out_size"], r["size_status"], r["size_err_off"], n)
        self.plan_outputs(r["out_size"], r["size_status"], n, align, r["dst_off"], r["dst_cap"], total)
        host = np.zeros(2, dtype=np.int64)
        if n > 0:
            e = self.lib.achip_memcpy_d2h(self.native.ctx, host.ctypes.data, _ptr(total), 16)
            if e < 0:
                native.raise_for_status(e)
            self.synchronize()
        r["total_bytes"], r["left_out"] = int(host[0]), int(host[1])
        r["dst"] = alloc(max(r["total_bytes"], 16))
        self.launch(op, src, src_off, src_len, r["dst"], r["dst_off"], r["dst_cap"], r["out_len"], r["status"], r["err_off"], n)
        return r

    def compress_bounds(self, op, src_len, out_size, status, n_blocks):
        """achip_compress_bound_batch: out_size[i] (int64) = what compress op `op` asks of dst_cap for src_len[i] bytes (the op's max_compressed_length, the Hadoop
        ops with the context's hadoop.buffer_size); a negative length or a bound beyond INT32_MAX gives status[i] of class INVALID_ARGUMENT and out_size[i] = 0.
        The pair feeds `plan_outputs` unchanged.  Asynchronous on the context stream; all arguments device-accessible."""
        r = self.lib.achip_compress_bound_batch(self.native.ctx, int(op), _ptr(src_len), _ptr(out_size), _ptr(status), int(n_blocks))
        if r < 0:
            native.raise_for_status(r)

    def pack_outputs(self, src, src_off, out_len, status, n_blocks, align, packed, packed_cap, packed_off, packed_len, total, raw=None, raw_off=None, raw_len=None,
                     stored=None):
        """achip_pack_outputs: a compress call's dst / dst_off / out_len / status as one dense stream.  packed_len[i] = the bytes taken (0 for an item with a
        status or a negative length), packed_off[i] = the sum of the lengths in front, each rounded up to `align`; with raw / raw_off / raw_len / stored (all
        four or none) an item whose compressed form is no smaller is taken from `raw` and stored[i] = 1.  total (three int64): bytes of the stream, items left
        out, 1 if the bytes were copied -- which happens iff `packed` is not None and total[0] <= packed_cap, decided on the device.  Asynchronous on the
        context stream."""
        r = self.lib.achip_pack_outputs(self.native.ctx, _ptr(src), _ptr(src_off), _ptr(out_len), _ptr(status), _ptr(raw), _ptr(raw_off), _ptr(raw_len), int(n_blocks),
                                        int(align), _ptr(packed), int(packed_cap), _ptr(packed_off), _ptr(packed_len), _ptr(stored), _ptr(total))
        if r < 0:
            native.raise_for_status(r)

    def _read_totals(self, total, words):
        host = np.zeros(words, dtype=np.int64)
        e = self.lib.achip_memcpy_d2h(self.native.ctx, host.ctypes.data, _ptr(total), 8 * words)
        if e < 0:
            native.raise_for_status(e)
        self.synchronize()
        return host

    def compress_packed(self, op, src, src_off, src_len, n_blocks, alloc, align=1, raw_fallback=False):
        """Compresses a device-resident batch into ONE dense buffer, the twin of `decompress_unsized`: bounds, plan, a readback of the slots' total, `alloc` the
        slot buffer, compress, pack (plan only), a readback of the dense total, `alloc` exactly that, pack.  It waits for the device at the two readbacks and
        walks nothing on the host.  `alloc(nbytes)` is the caller's device allocator (it returns something with data_ptr(), or an address).  What it returns must be
        ready for the context's stream: an allocator that fills its memory on another stream finishes the fill first.
        raw_fallback: an item whose compressed form is no smaller than its plaintext is taken from src / src_off / src_len instead (stored[i] = 1).  The result:
          packed, total_bytes, left_out                  the dense buffer (total_bytes bytes; the pack still in flight on the stream), the items without a place in it
          packed_off, packed_len, stored                 where item i lies and how many bytes (int64 / int32); int32 flags, None without raw_fallback
          slots, slot_bytes, dst_off, dst_cap            the compress call's worst-case buffer and its plan (the caller may free `slots` once the stream is idle)
          out_len, status, err_off                       the compress call's arrays (int32 / int32 / int64)
          bound, bound_status                            what the bounds said (int64 / int32): an item with bound_status != 0 was given no slot
        """
        n = int(n_blocks)
        wide, narrow = max(8 * n, 16), max(4 * n, 16)
        r = {"bound": alloc(wide), "bound_status": alloc(narrow), "dst_off": alloc(wide), "dst_cap": alloc(narrow), "out_len": alloc(narrow), "status": alloc(narrow),
             "err_off": alloc(wide), "packed_off": alloc(wide), "packed_len": alloc(narrow), "stored": alloc(narrow) if raw_fallback else None}
        total = alloc(24)
        raw = {"raw": src, "raw_off": src_off, "raw_len": src_len, "stored": r["stored"]} if raw_fallback else {}
        self.compress_bounds(op, src_len, r["bound"], r["bound_status"], n)
        self.plan_outputs(r["bound"], r["bound_status"], n, 1, r["dst_off"], r["dst_cap"], total)
        r["slot_bytes"] = int(self._read_totals(total, 2)[0]) if n > 0 else 0
        r["slots"] = alloc(max(r["slot_bytes"], 16))
        self.launch(op, src, src_off, src_len, r["slots"], r["dst_off"], r["dst_cap"], r["out_len"], r["status"], r["err_off"], n)
        self.pack_outputs(r["slots"], r["dst_off"], r["out_len"], r["status"], n, align, None, 0, r["packed_off"], r["packed_len"], total, **raw)
        host = self._read_totals(total, 3) if n > 0 else np.zeros(3, dtype=np.int64)
        r["total_bytes"], r["left_out"] = int(host[0]), int(host[1])
        r["packed"] = alloc(max(r["total_bytes"], 16))
        self.pack_outputs(r["slots"], r["dst_off"], r["out_len"], r["status"], n, align, r["packed"], r["total_bytes"], r["packed_off"], r["packed_len"], total, **raw)
        return r

    def window_decompress(self, op, flags, src, src_off, src_len, dst, dst_off, dst_cap, out_len, status, err_off, n_blocks, consumed, stop, need):
        """achip_window_decompress_batch: item i is a WINDOW of an x-snappy-framed or Hadoop stream (op: OP_SNAPPYFRAMED_ / OP_LZ4HADOOP_ / OP_SNAPPYHADOOP_DECOMPRESS)
        that begins at a unit boundary; flags[i] (int32) = native.WINDOW_FIRST | native.WINDOW_LAST.  The call takes the leading whole units that fit dst_cap[i]:
        consumed[i] (int64) bytes of input, out_len[i] bytes of plaintext; stop[i] (int32, native.STOP_*) says why it took no more and need[i] (int64) what the next
        unit wants.  The caller keeps the stream position; nothing is kept between calls.  Asynchronous on the context stream; all arguments device-accessible."""
        r = self.lib.achip_window_decompress_batch(self.native.ctx, int(op), _ptr(flags), _ptr(src), _ptr(src_off), _ptr(src_len), _ptr(dst), _ptr(dst_off), _ptr(dst_cap),
                                                   _ptr(out_len), _ptr(status), _ptr(err_off), int(n_blocks), _ptr(consumed), _ptr(stop), _ptr(need))
        if r < 0:
            native.raise_for_status(r)

    def window_compress(self, op, flags, src, src_off, src_len, dst, dst_off, dst_cap, out_len, status, err_off, n_blocks, consumed, stop, need):
        """achip_window_compress_batch: the writers' side of `window_decompress` (op: the three container compress ops).  consumed[i] = the whole blocks of window i
        whose worst case fits dst_cap[i] -- with WINDOW_LAST the partial tail too; the outputs of a stream's windows, one behind the other, are the one-shot
        writer's stream.  Asynchronous on the context stream; all arguments device-accessible."""
        r = self.lib.achip_window_compress_batch(self.native.ctx, int(op), _ptr(flags), _ptr(src), _ptr(src_off), _ptr(src_len), _ptr(dst), _ptr(dst_off), _ptr(dst_cap),
                                                 _ptr(out_len), _ptr(status), _ptr(err_off), int(n_blocks), _ptr(consumed), _ptr(stop), _ptr(need))
        if r < 0:
            native.raise_for_status(r)

    def window_host(self, op, flags, src, dst_cap, compress=False):
        """achip_window_decompress / achip_window_compress: ONE window in host memory (`src`: bytes-like), staged through the context's pinned buffer; synchronous.
        -> (consumed, output bytes, stop, need, status, err_off)"""
        src = np.frombuffer(bytes(src), dtype=np.uint8)
        dst = np.empty(max(int(dst_cap), 1), dtype=np.uint8)
        consumed, produced, need, err = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        stop = ctypes.c_int32()
        fn = self.lib.achip_window_compress if compress else self.lib.achip_window_decompress
        r = fn(self.native.ctx, int(op), int(flags), src.ctypes.data if len(src) else None, len(src), dst.ctypes.data, int(dst_cap), ctypes.byref(consumed),
               ctypes.byref(produced), ctypes.byref(stop), ctypes.byref(need), ctypes.byref(err))
        if r < 0 and stop.value != native.STOP_FAILED:
            native.raise_for_status(r)  # (the call itself failed: arguments, the device)
        return consumed.value, dst[:produced.value].tobytes(), stop.value, need.value, r, err.value

    def run_host_mixed(self, ops, src, src_off, src_len, dst, dst_off, dst_cap):
        """Host numpy arrays in/out through achip_mixed_batch_host: one op per item."""
        n = len(src_off)
        ops = np.ascontiguousarray(ops, dtype=np.int32)
        src = np.ascontiguousarray(src, dtype=np.uint8)
        src_off = np.ascontiguousarray(src_off, dtype=np.int64)
        src_len = np.ascontiguousarray(src_len, dtype=np.int32)
        dst_off = np.ascontiguousarray(dst_off, dtype=np.int64)
        dst_cap = np.ascontiguousarray(dst_cap, dtype=np.int32)
        out_len = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        err_off = np.zeros(n, dtype=np.int64)
        r = self.lib.achip_mixed_batch_host(self.native.ctx, ops.ctypes.data, src.ctypes.data, src_off.ctypes.data, src_len.ctypes.data, dst.ctypes.data,
                                            dst_off.ctypes.data, dst_cap.ctypes.data, out_len.ctypes.data, status.ctypes.data, err_off.ctypes.data, n)
        if r < 0:
            native.raise_for_status(r)
        return out_len, status, err_off

    def run_host(self, op, src, src_off, src_len, dst, dst_off, dst_cap):
        """Host numpy arrays in/out through achip_batch_host (stages through pinned memory)."""
        n = len(src_off)
        src = np.ascontiguousarray(src, dtype=np.uint8)
        src_off = np.ascontiguousarray(src_off, dtype=np.int64)
        src_len = np.ascontiguousarray(src_len, dtype=np.int32)
        dst_off = np.ascontiguousarray(dst_off, dtype=np.int64)
        dst_cap = np.ascontiguousarray(dst_cap, dtype=np.int32)
        out_len = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        err_off = np.zeros(n, dtype=np.int64)
        r = self.lib.achip_batch_host(op, self.native.ctx, src.ctypes.data, src_off.ctypes.data, src_len.ctypes.data, dst.ctypes.data,
                                      dst_off.ctypes.data, dst_cap.ctypes.data, out_len.ctypes.data, status.ctypes.data, err_off.ctypes.data, n)
        if r < 0:
            native.raise_for_status(r)
        return out_len, status, err_off

    # timing helpers on the context stream
    def event(self):
        return self.lib.achip_event_create()

    def record(self, ev):
        self.lib.achip_event_record(self.native.ctx, ev)

    def elapsed_ms(self, ev0, ev1):
        return float(self.lib.achip_event_elapsed_ms(ev0, ev1))
