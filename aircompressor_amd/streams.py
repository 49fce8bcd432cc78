"""Stream classes over the windowed container calls (achip_window_decompress / achip_window_compress): the Python twins of the reference's
SnappyFramedInputStream / SnappyFramedOutputStream, Lz4HadoopInputStream / Lz4HadoopOutputStream and SnappyHadoopInputStream / SnappyHadoopOutputStream
(M/snappy/SnappyFramed*Stream.java, M/lz4/Lz4Hadoop*Stream.java, M/snappy/SnappyHadoop*Stream.java) -- any stream length in bounded memory.  A stream object
holds the stream position and a pending buffer; the library keeps nothing between calls.
"""
from . import native
from .batch import HipBatchCodec, OP_SNAPPYFRAMED_DECOMPRESS, OP_SNAPPYFRAMED_COMPRESS, OP_LZ4HADOOP_DECOMPRESS, OP_LZ4HADOOP_COMPRESS, OP_SNAPPYHADOOP_DECOMPRESS, OP_SNAPPYHADOOP_COMPRESS
from .codecs import _check_snappyframed_writer
from .errors import MalformedInputException

DEFAULT_WINDOW_BYTES = 4 << 20  # what a stream holds of its source / sink at a time, unless a single unit wants more


class HipWindowInputStream:
    """read(n) / readall() over a binary source (anything with read(n)); `op` is one of the three container decode ops."""

    def __init__(self, source, op, device=0, native_ctx=None, window_bytes=DEFAULT_WINDOW_BYTES, buffer_size=None, configure=None):
        self._codec = HipBatchCodec(device, native_ctx)
        self._source, self._op, self._window = source, op, int(window_bytes)
        self._buffer_size = buffer_size
        self._configure = configure  # called with the context before every window call: the stream object's constructor arguments
        self._pending = b""       # compressed bytes not yet taken: begins at a unit boundary
        self._want = self._window  # how many of them a call wants in hand
        self._room = self._window
        self._plain = b""         # decoded bytes not yet handed out
        self._position = 0        # stream offset of _pending
        self._first, self._eof, self._error = True, False, None

    def _fill(self):
        while not self._eof and len(self._pending) < self._want:
            piece = self._source.read(self._want - len(self._pending))
            if not piece:
                self._eof = True
            self._pending += piece

    def _step(self):
        """one window call; -> False at the end of the stream"""
        if self._error is not None:
            return False
        self._fill()
        if self._eof and not self._pending and not self._first:
            return False
        if self._buffer_size is not None:
            self._codec.native.set_option("hadoop.buffer_size", self._buffer_size)
        if self._configure is not None:
            self._configure(self._codec.native)
        flags = (native.WINDOW_FIRST if self._first else 0) | (native.WINDOW_LAST if self._eof else 0)
        consumed, out, stop, need, status, err = self._codec.window_host(self._op, flags, self._pending, self._room)
        self._plain += out
        self._pending = self._pending[consumed:]
        self._first = self._first and consumed == 0
        if stop == native.STOP_FAILED:
            reason = self._codec.lib.achip_detail_message(native.status_detail(status)).decode()
            self._error = MalformedInputException(self._position + err, reason, status)
            return False  # (raised once the bytes in front of the damage have been handed out)
        self._position += consumed
        self._want, self._room = self._window, self._window
        if stop == native.STOP_NEED_INPUT and consumed == 0:
            self._want = max(len(self._pending) + self._window, need)  # grown only as far as the unit asks (or by a window, where its headers do not say)
        elif stop == native.STOP_NEED_ROOM and not out and consumed == 0:
            self._room = max(need, self._room + 1)
        return not (stop == native.STOP_END and self._eof and not self._pending)

    def read(self, n=-1):
        if n is None or n < 0:
            return self.readall()
        more = True
        while len(self._plain) < n and more:
            more = self._step()
        return self._hand_out(n)

    def readall(self):
        while self._step():
            pass
        return self._hand_out(len(self._plain))

    def _hand_out(self, n):
        if self._error is not None and not self._plain:
            raise self._error
        out, self._plain = self._plain[:n], self._plain[n:]
        return out

    def close(self):
        self._pending = self._plain = b""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class HipWindowOutputStream:
    """write(b) / finish() / close() onto a binary sink (anything with write(b)); `op` is one of the three container compress ops."""

    def __init__(self, sink, op, device=0, native_ctx=None, window_bytes=DEFAULT_WINDOW_BYTES, buffer_size=None, configure=None):
        self._codec = HipBatchCodec(device, native_ctx)
        self._sink, self._op, self._window = sink, op, int(window_bytes)
        self._buffer_size = buffer_size
        self._configure = configure
        self._pending = b""
        self._room = 2 * self._window + 65536
        self._first, self._finished = True, False

    def _flush(self, closing):
        while True:
            if self._buffer_size is not None:
                self._codec.native.set_option("hadoop.buffer_size", self._buffer_size)
            if self._configure is not None:
                self._configure(self._codec.native)
            flags = (native.WINDOW_FIRST if self._first else 0) | (native.WINDOW_LAST if closing else 0)
            consumed, out, stop, need, status, _ = self._codec.window_host(self._op, flags, self._pending, self._room, compress=True)
            if stop == native.STOP_FAILED:
                native.raise_for_status(status)
            self._sink.write(out)
            self._first = self._first and not out
            self._pending = self._pending[consumed:]
            if stop == native.STOP_NEED_ROOM and not out and consumed == 0:
                self._room = max(need, self._room + 1)
            elif stop != native.STOP_NEED_ROOM:
                return

    def write(self, b):
        if self._finished:
            raise ValueError("write to a finished stream")
        self._pending += bytes(b)
        if len(self._pending) >= self._window:
            self._flush(False)
        return len(b)

    def finish(self):
        """the rest of the stream: the partial last block, and whatever an empty stream consists of"""
        if not self._finished:
            self._flush(True)
            self._finished = True

    def close(self):
        self.finish()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _twins(name, decode_op, encode_op, hadoop, doc):
    framed = decode_op == OP_SNAPPYFRAMED_DECOMPRESS  # the x-snappy-framed twins take their reference classes' constructor arguments

    class In(HipWindowInputStream):
        def __init__(self, source, device=0, native_ctx=None, window_bytes=DEFAULT_WINDOW_BYTES, **kw):
            configure = None
            if framed:
                verify = bool(kw.pop("verify_checksums", True))
                configure = lambda ctx: ctx.set_snappyframed_verify_checksums(verify)  # noqa: E731
            super().__init__(source, decode_op, device, native_ctx, window_bytes, kw.pop("buffer_size", 262144) if hadoop else None, configure)
            assert not kw, kw

    class Out(HipWindowOutputStream):
        def __init__(self, sink, device=0, native_ctx=None, window_bytes=DEFAULT_WINDOW_BYTES, **kw):
            configure = None
            if framed:
                writer = (bool(kw.pop("write_checksums", True)), int(kw.pop("block_size", 65536)), float(kw.pop("min_compression_ratio", 0.85)))
                _check_snappyframed_writer(writer[1], writer[2])
                configure = lambda ctx: ctx.set_snappyframed_writer(*writer)  # noqa: E731
            super().__init__(sink, encode_op, device, native_ctx, window_bytes, kw.pop("buffer_size", 262144) if hadoop else None, configure)
            assert not kw, kw

    In.__name__ = In.__qualname__ = name + "HipInputStream"
    Out.__name__ = Out.__qualname__ = name + "HipOutputStream"
    In.__doc__ = "The twin of %sInputStream: %s" % (name, doc)
    Out.__doc__ = "The twin of %sOutputStream: %s" % (name, doc)
    return In, Out


SnappyFramedHipInputStream, SnappyFramedHipOutputStream = _twins("SnappyFramed", OP_SNAPPYFRAMED_DECOMPRESS, OP_SNAPPYFRAMED_COMPRESS, False,
                                                                 "x-snappy-framed streams (M/snappy/SnappyFramedInputStream.java, SnappyFramedOutputStream.java)")
Lz4HadoopHipInputStream, Lz4HadoopHipOutputStream = _twins("Lz4Hadoop", OP_LZ4HADOOP_DECOMPRESS, OP_LZ4HADOOP_COMPRESS, True,
                                                           "Hadoop LZ4 block streams (M/lz4/Lz4HadoopInputStream.java, Lz4HadoopOutputStream.java); buffer_size as Lz4HadoopStreams")
SnappyHadoopHipInputStream, SnappyHadoopHipOutputStream = _twins("SnappyHadoop", OP_SNAPPYHADOOP_DECOMPRESS, OP_SNAPPYHADOOP_COMPRESS, True,
                                                                 "Hadoop Snappy block streams (M/snappy/SnappyHadoopInputStream.java, SnappyHadoopOutputStream.java)")
