"""ctypes binding of libaircompressor_hip.so -- the Python twin of the Java `HipNative` FFM record
(java/io/airlift/compress/v3/hip/HipNative.java), modelled on M/lz4/Lz4Native.java:30-129.
"""
import ctypes
import os
import math
import struct

from .errors import HipUnavailableError, IllegalArgumentException, MalformedInputException

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBRARY_PATH = os.path.join(_HERE, "libaircompressor_hip.so")

CLASS_MALFORMED, CLASS_OUTPUT_TOO_SMALL, CLASS_INVALID_ARGUMENT, CLASS_DEVICE = 1, 2, 3, 4
DETAIL_LZ4_EMPTY_OUTPUT = 7
DETAIL_LZO_MALFORMED, DETAIL_LZO_MAX_INPUT, DETAIL_LZO_MAX_OUTPUT = 111, 112, 113
# achip_window_*: a window's flags and why a call stopped (include/aircompressor_hip.h)
WINDOW_FIRST, WINDOW_LAST = 1, 2
STOP_END, STOP_NEED_INPUT, STOP_NEED_ROOM, STOP_FAILED = 0, 1, 2, 3

_i32, _i64, _vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
_BATCH = [_vp] * 10 + [_i32]

# name -> (restype, argtypes): every symbol include/aircompressor_hip.h declares
SIGNATURES = {
    "achip_status_class": (_i32, [_i32]),
    "achip_status_detail": (_i32, [_i32]),
    "achip_detail_message": (ctypes.c_char_p, [_i32]),
    "achip_version": (ctypes.c_char_p, []),
    "achip_device_count": (_i32, []),
    "achip_last_error": (ctypes.c_char_p, []),
    "achip_lz4_max_compressed_length": (_i32, [_i32]),
    "achip_lzo_max_compressed_length": (_i32, [_i32]),
    "achip_snappy_max_compressed_length": (_i32, [_i32]),
    "achip_zstd_max_compressed_length": (_i32, [_i32]),
    "achip_snappy_uncompressed_length": (_i64, [_vp, _i64, ctypes.POINTER(_i64)]),
    "achip_zstd_decompressed_size": (_i64, [_vp, _i64, ctypes.POINTER(_i64)]),
    "achip_zstd_decompress_bound": (_i64, [_vp, _i64, ctypes.POINTER(_i64)]),
    "achip_ctx_create": (_vp, [_i32]),
    "achip_ctx_destroy": (None, [_vp]),
    "achip_ctx_device": (_i32, [_vp]),
    "achip_ctx_stream": (_vp, [_vp]),
    "achip_ctx_synchronize": (_i32, [_vp]),
    "achip_ctx_set_option": (_i32, [_vp, ctypes.c_char_p, _i64]),
    "achip_ctx_get_stat": (_i64, [_vp, ctypes.c_char_p]),
    "achip_ctx_set_lz4_acceleration": (_i32, [_vp, _i32]),
    "achip_ctx_get_lz4_acceleration": (_i32, [_vp]),
    "achip_ctx_set_lz4frame_linked_blocks": (_i32, [_vp, _i32]),
    "achip_ctx_get_lz4frame_linked_blocks": (_i32, [_vp]),
    "achip_snappyframed_max_compressed_length": (_i32, [_i32]),
    "achip_snappyframed_max_compressed_length_for": (_i32, [_i32, _i32]),
    "achip_ctx_set_lz4frame_writer": (_i32, [_vp, _i32, _i32, _i32, _i32]),
    "achip_ctx_get_lz4frame_writer": (_i32, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_i32), ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    "achip_lz4frame_max_compressed_length_for": (_i32, [_i32, _i32, _i32, _i32, _i32]),
    "achip_ctx_set_snappyframed_writer": (_i32, [_vp, _i32, _i32, _i64]),
    "achip_ctx_get_snappyframed_writer": (_i32, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_i32), ctypes.POINTER(_i64)]),
    "achip_ctx_set_snappyframed_verify_checksums": (_i32, [_vp, _i32]),
    "achip_ctx_get_snappyframed_verify_checksums": (_i32, [_vp]),
    "achip_snappyframed_decompress_batch": (_i32, _BATCH),
    "achip_snappyframed_compress_batch": (_i32, _BATCH),
    "achip_snappyframed_compress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_snappyframed_decompress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_hadoop_max_compressed_length": (_i32, [_i32, _i32, _i32]),
    "achip_zstdstream_max_compressed_length": (_i32, [_i32]),
    "achip_zstdstream_compress_batch": (_i32, _BATCH),
    "achip_zstdstream_compress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_lz4hadoop_decompress_batch": (_i32, _BATCH),
    "achip_lz4hadoop_compress_batch": (_i32, _BATCH),
    "achip_snappyhadoop_decompress_batch": (_i32, _BATCH),
    "achip_snappyhadoop_compress_batch": (_i32, _BATCH),
    "achip_lz4hadoop_compress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_lz4hadoop_decompress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_snappyhadoop_compress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_snappyhadoop_decompress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_lz4frame_max_compressed_length": (_i32, [_i32]),
    "achip_lz4frame_decompress_batch": (_i32, _BATCH),
    "achip_lz4frame_compress_batch": (_i32, _BATCH),
    "achip_lz4frame_compress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_lz4frame_decompress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_xxhash64_batch": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i32]),
    "achip_xxhash32_batch": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _i32]),
    "achip_xxhash64": (_i32, [_vp, _vp, _i64, _i64, _vp]),
    "achip_xxhash32": (_i32, [_vp, _vp, _i64, _i32, _vp]),
    "achip_xxhash3_64_batch": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i32]),
    "achip_xxhash3_128_batch": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i32]),
    "achip_xxhash3_64": (_i32, [_vp, _vp, _i64, _i64, _vp]),
    "achip_xxhash3_128": (_i32, [_vp, _vp, _i64, _i64, _vp]),
    "achip_hash_state_size": (_i64, [_i32]),
    "achip_hash_states_reset": (_i32, [_vp, _i32, _vp, _i32, _i64]),
    "achip_hash_states_update": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32]),
    "achip_hash_states_digest": (_i32, [_vp, _i32, _vp, _vp, _i32]),
    "achip_hasher_create": (_vp, [_vp, _i32, _i64]),
    "achip_hasher_update": (_i32, [_vp, _vp, _i64]),
    "achip_hasher_digest": (_i32, [_vp, _vp]),
    "achip_hasher_reset": (_i32, [_vp, _i64]),
    "achip_hasher_destroy": (_i32, [_vp]),
    "achip_device_alloc": (_vp, [_vp, _i64]),
    "achip_device_free": (_i32, [_vp, _vp]),
    "achip_host_alloc_pinned": (_vp, [_i64]),
    "achip_host_free_pinned": (_i32, [_vp]),
    "achip_memcpy_h2d": (_i32, [_vp, _vp, _vp, _i64]),
    "achip_memcpy_d2h": (_i32, [_vp, _vp, _vp, _i64]),
    "achip_memset_d": (_i32, [_vp, _vp, _i32, _i64]),
    "achip_event_create": (_vp, []),
    "achip_event_destroy": (_i32, [_vp]),
    "achip_event_record": (_i32, [_vp, _vp]),
    "achip_event_elapsed_ms": (ctypes.c_float, [_vp, _vp]),
    "achip_lz4_decompress_batch": (_i32, _BATCH),
    "achip_lz4_compress_batch": (_i32, _BATCH),
    "achip_snappy_decompress_batch": (_i32, _BATCH),
    "achip_snappy_compress_batch": (_i32, _BATCH),
    "achip_zstd_decompress_batch": (_i32, _BATCH),
    "achip_zstd_compress_batch": (_i32, _BATCH),
    "achip_lzo_decompress_batch": (_i32, _BATCH),
    "achip_lzo_compress_batch": (_i32, _BATCH),
    "achip_lzo_compress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_lzo_decompress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_lz4_compress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_lz4_decompress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_snappy_compress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_snappy_decompress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_zstd_compress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_zstd_decompress": (_i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "achip_batch_host": (_i32, [_i32] + _BATCH),
    "achip_mixed_batch": (_i32, [_vp, _vp] + _BATCH[1:]),
    "achip_mixed_batch_host": (_i32, [_vp, _vp] + _BATCH[1:]),
    "achip_zstdstream_decompress_begin": (_vp, [_vp]),
    "achip_zstdstream_decompress_feed": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "achip_zstdstream_decompress_at_stopping_point": (_i32, [_vp]),
    "achip_zstdstream_decompress_end": (_i32, [_vp, _vp]),
    "achip_zstdstream_compress_begin": (_vp, [_vp]),
    "achip_zstdstream_compress_feed": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "achip_zstdstream_compress_finish": (_i32, [_vp, _vp, _vp, _i64, ctypes.POINTER(_i64)]),
    "achip_zstdstream_compress_end": (_i32, [_vp, _vp]),
    "achip_decoded_size_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32]),
    "achip_plan_outputs": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "achip_compress_bound_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32]),
    "achip_pack_outputs": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _vp]),
    "achip_window_decompress_batch": (_i32, [_vp, _i32, _vp] + _BATCH[1:] + [_vp, _vp, _vp]),
    "achip_window_compress_batch": (_i32, [_vp, _i32, _vp] + _BATCH[1:] + [_vp, _vp, _vp]),
    "achip_window_decompress": (_i32, [_vp, _i32, _i32, _vp, _i32, _vp, _i32] + [ctypes.POINTER(_i64)] * 2 + [ctypes.POINTER(_i32)] + [ctypes.POINTER(_i64)] * 2),
    "achip_window_compress": (_i32, [_vp, _i32, _i32, _vp, _i32, _vp, _i32] + [ctypes.POINTER(_i64)] * 2 + [ctypes.POINTER(_i32)] + [ctypes.POINTER(_i64)] * 2),
    "achip_multi_batch_host": (_i32, [_vp, _i32, _i32, _vp] + _BATCH[1:] + [_vp]),
    "achip_partition_blocks": (_i32, [_vp, _i32, _i32, _vp]),
}

_lib = None


def load_library():
    """dlopen the in-tree shared library and type every symbol; raises HipUnavailableError if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIBRARY_PATH):
            raise HipUnavailableError(
                "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C aircompressor_amd/csrc`); there is no CPU fallback" % LIBRARY_PATH)
        try:
            lib = ctypes.CDLL(LIBRARY_PATH)
        except OSError as e:  # e.g. libamdhip64 not loadable
            raise HipUnavailableError("cannot load %s: %s" % (LIBRARY_PATH, e))
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError here = ABI/header drift: loud on purpose
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = lib
    return _lib


SNF_DEFAULT_BLOCK_SIZE = SNF_MAX_BLOCK_SIZE = 65536
LZ4F_DEFAULT_BLOCK_MAX_SIZE = 4194304
SNF_DEFAULT_MIN_RATIO = 0.85  # ACHIP_SNF_DEFAULT_MIN_RATIO_BITS


def double_bits(value):
    """Double.doubleToRawLongBits"""
    return struct.unpack("<q", struct.pack("<d", float(value)))[0]


def java_double_text(value):
    """Double.toString(value), as the library prints a refused ratio (abi_context.cpp): the shortest digits, two at least, that read back as the value"""
    v = float(value)
    if v != v:
        return "NaN"
    if v == 0:
        return "-0.0" if math.copysign(1.0, v) < 0 else "0.0"
    if math.isinf(v):
        return "-Infinity" if v < 0 else "Infinity"
    text = next(t for t in ("%.*e" % (p - 1, v) for p in range(2, 18)) if float(t) == v)
    mantissa, exponent = text.split("e")
    sign, digits, exponent = ("-" if v < 0 else ""), mantissa.lstrip("-").replace(".", "").rstrip("0") or "0", int(exponent)
    if -3 <= exponent < 7:
        digits = digits.ljust(exponent + 1, "0") if exponent >= 0 else "0" * -exponent + digits
        whole, frac = (digits[:exponent + 1], digits[exponent + 1:]) if exponent >= 0 else ("0", digits[1:])
        return sign + whole + "." + (frac or "0")
    return sign + digits[0] + "." + (digits[1:] or "0") + "E%d" % exponent


def bits_double(bits):
    """Double.longBitsToDouble"""
    return struct.unpack("<d", struct.pack("<q", int(bits)))[0]


def status_class(status):
    return (-status) & 15 if status < 0 else 0


def status_detail(status):
    return (-status) >> 4 if status < 0 else 0


def raise_for_status(status, err_offset=0):
    """Translate a negative ACHIP status into the exception the Java codec would throw."""
    lib = load_library()
    cls, detail = status_class(status), status_detail(status)
    reason = lib.achip_detail_message(detail).decode()
    if cls == CLASS_MALFORMED:
        raise MalformedInputException(err_offset, reason, status)
    if cls == CLASS_DEVICE:
        raise HipUnavailableError("%s: %s" % (reason, lib.achip_last_error().decode()))
    raise IllegalArgumentException(reason, status)


class HipNative:
    """One HIP context (stream + scratch) on one device; owns its native handle."""

    def __init__(self, device=0):
        self.lib = load_library()
        if self.lib.achip_device_count() <= 0:
            raise HipUnavailableError("no HIP device visible: the Hip codecs cannot run (no CPU fallback)")
        self.ctx = self.lib.achip_ctx_create(device)
        if not self.ctx:
            raise HipUnavailableError("achip_ctx_create(%d) failed: %s" % (device, self.lib.achip_last_error().decode()))
        self.device = device

    @staticmethod
    def is_enabled():
        try:
            return load_library().achip_device_count() > 0
        except HipUnavailableError:
            return False

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.achip_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name, value):
        r = self.lib.achip_ctx_set_option(self.ctx, name.encode(), int(value))
        if r < 0:
            raise_for_status(r)

    def get_stat(self, name):
        return int(self.lib.achip_ctx_get_stat(self.ctx, name.encode()))

    def set_lz4_acceleration(self, acceleration):
        """Lz4Compressor.create(acceleration) for this context's LZ4 block and LZ4 frame encodes (1 .. 65537; 1: the Java encoder)"""
        r = self.lib.achip_ctx_set_lz4_acceleration(self.ctx, int(acceleration))
        if r < 0:
            raise IllegalArgumentException(self.lib.achip_last_error().decode(), r)

    def get_lz4_acceleration(self):
        r = int(self.lib.achip_ctx_get_lz4_acceleration(self.ctx))
        if r < 0:
            raise_for_status(r)
        return r

    def set_lz4frame_linked_blocks(self, accept):
        """1: this context's LZ4 frame decodes and its LZ4FRAME size queries read frames of linked blocks (liblz4's default frames; the Java reader refuses them);
        0 (the default): they fail with DETAIL_LZ4F_LINKED_BLOCKS.  The library checks the value: anything but 0 / 1 (or a bool) is refused"""
        r = self.lib.achip_ctx_set_lz4frame_linked_blocks(self.ctx, int(accept))
        if r < 0:
            raise IllegalArgumentException(self.lib.achip_last_error().decode(), r)

    def get_lz4frame_linked_blocks(self):
        r = int(self.lib.achip_ctx_get_lz4frame_linked_blocks(self.ctx))
        if r < 0:
            raise_for_status(r)
        return bool(r)

    def set_lz4frame_writer(self, block_size=LZ4F_DEFAULT_BLOCK_MAX_SIZE, block_checksum=False, content_checksum=False, content_size=False):
        """The frame descriptor of this context's LZ4 frame encodes: the block-maximum size (65536, 262144, 1048576 or 4194304) and whether a frame carries block
        checksums, a content checksum, its content size.  Anything but (4194304, False, False, False) takes the block-list writer, which asks
        achip_lz4frame_max_compressed_length_for of the capacity.  The library checks the values: a flag must be 0 / 1 (or a bool)"""
        r = self.lib.achip_ctx_set_lz4frame_writer(self.ctx, int(block_size), int(block_checksum), int(content_checksum), int(content_size))
        if r < 0:
            raise IllegalArgumentException(self.lib.achip_last_error().decode(), r)

    def get_lz4frame_writer(self):
        """-> (block_size, block_checksum, content_checksum, content_size)"""
        v = [_i32(0) for _ in range(4)]
        r = self.lib.achip_ctx_get_lz4frame_writer(self.ctx, *(ctypes.byref(x) for x in v))
        if r < 0:
            raise_for_status(r)
        return v[0].value, bool(v[1].value), bool(v[2].value), bool(v[3].value)

    def set_snappyframed_writer(self, write_checksums=True, block_size=SNF_DEFAULT_BLOCK_SIZE, min_compression_ratio=SNF_DEFAULT_MIN_RATIO):
        """SnappyFramedOutputStream(compressor, out, writeChecksums, blockSize, minCompressionRatio) for this context's x-snappy-framed encodes; the ratio
        crosses as its IEEE-754 bits"""
        r = self.lib.achip_ctx_set_snappyframed_writer(self.ctx, 1 if write_checksums else 0, int(block_size), double_bits(min_compression_ratio))
        if r < 0:
            raise IllegalArgumentException(self.lib.achip_last_error().decode(), r)

    def get_snappyframed_writer(self):
        """-> (write_checksums, block_size, min_compression_ratio)"""
        checksums, block_size, bits = _i32(0), _i32(0), _i64(0)
        r = self.lib.achip_ctx_get_snappyframed_writer(self.ctx, ctypes.byref(checksums), ctypes.byref(block_size), ctypes.byref(bits))
        if r < 0:
            raise_for_status(r)
        return bool(checksums.value), block_size.value, bits_double(bits.value)

    def set_snappyframed_verify_checksums(self, verify):
        """SnappyFramedInputStream(decompressor, in, verifyChecksums) for this context's x-snappy-framed decodes"""
        r = self.lib.achip_ctx_set_snappyframed_verify_checksums(self.ctx, 1 if verify else 0)
        if r < 0:
            raise IllegalArgumentException(self.lib.achip_last_error().decode(), r)

    def get_snappyframed_verify_checksums(self):
        r = int(self.lib.achip_ctx_get_snappyframed_verify_checksums(self.ctx))
        if r < 0:
            raise_for_status(r)
        return bool(r)

    def synchronize(self):
        r = self.lib.achip_ctx_synchronize(self.ctx)
        if r < 0:
            raise_for_status(r)

    @property
    def stream(self):
        return self.lib.achip_ctx_stream(self.ctx)
