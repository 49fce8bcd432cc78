/*
 * Licensed under the Apache License, Version 2.0 (the "License");
 * you may not use this file except in compliance with the License.
 * You may obtain a copy of the License at
 *
 *     http://www.apache.org/licenses/LICENSE-2.0
 *
 * Unless required by applicable law or agreed to in writing, software
 * distributed under the License is distributed on an "AS IS" BASIS,
 * WITHOUT WARRANTIES OR CONDITIONS OF ANY KIND, either express or implied.
 * See the License for the specific language governing permissions and
 * limitations under the License.
 */
package io.airlift.compress.v3.hip;

import java.io.IOException;
import java.io.InputStream;
import java.lang.foreign.Arena;
import java.lang.foreign.MemorySegment;
import java.lang.foreign.ValueLayout;

import static java.util.Objects.checkFromIndexSize;
import static java.util.Objects.requireNonNull;

/**
 * {@code SnappyFramedInputStream}, {@code Lz4HadoopInputStream} and {@code SnappyHadoopInputStream} with the decoders on an AMD GPU (MI355X, gfx950): ONE class over
 * {@code achip_window_decompress}, the format chosen by the decode op ({@link HipNative#OP_SNAPPYFRAMED_DECOMPRESS}, {@link HipNative#OP_LZ4HADOOP_DECOMPRESS},
 * {@link HipNative#OP_SNAPPYHADOOP_DECOMPRESS}).  The stream holds a window of its source -- {@code windowBytes}, more only when a single unit of the stream asks for
 * it -- and hands it to the library, which decodes the whole units in it side by side and says how far it came; nothing is kept in the library between calls, so a
 * stream of any length is read in bounded memory.  A damaged stream delivers every byte in front of the damage and fails at the read that reaches it.
 * To read many streams at once use {@link HipNative.Context#windowBatch}: one window per stream and call.
 */
public final class HipWindowInputStream
        extends InputStream
{
    private final InputStream in;
    private final HipNative.Context context;
    private final int op;
    private final int windowBytes;
    private final Arena arena = Arena.ofShared();
    private final MemorySegment result = arena.allocate(ValueLayout.JAVA_LONG, 5);
    private byte[] pending;
    private int pendingLength;
    private int want;
    private byte[] plain;
    private int plainOffset;
    private int plainLength;
    private boolean first = true;
    private boolean inputEnded;
    private boolean finished;
    private RuntimeException failure;
    private long position;
    private byte[] singleByte;
    private boolean closed;

    public HipWindowInputStream(InputStream in, int op, int windowBytes, int device)
    {
        this.in = requireNonNull(in, "in is null");
        if (op != HipNative.OP_SNAPPYFRAMED_DECOMPRESS && op != HipNative.OP_LZ4HADOOP_DECOMPRESS && op != HipNative.OP_SNAPPYHADOOP_DECOMPRESS) {
            throw new IllegalArgumentException("op is not a container decode op");
        }
        if (windowBytes <= 0) {
            throw new IllegalArgumentException("windowBytes must be positive");
        }
        HipNative.verifyEnabled();
        this.context = new HipNative.Context(device);
        this.op = op;
        this.windowBytes = windowBytes;
        this.pending = new byte[windowBytes];
        this.plain = new byte[windowBytes];
        this.want = windowBytes;
    }

    @Override
    public int read()
            throws IOException
    {
        if (singleByte == null) {
            singleByte = new byte[1];
        }
        return read(singleByte, 0, 1) < 0 ? -1 : singleByte[0] & 0xFF;
    }

    @Override
    public int read(byte[] output, int offset, int length)
            throws IOException
    {
        checkFromIndexSize(offset, length, output.length);
        if (closed) {
            throw new IOException("stream is closed");
        }
        if (length == 0) {
            return 0;
        }
        while (plainLength == 0) {
            if (failure != null) {
                throw failure;
            }
            if (finished) {
                return -1;
            }
            step();
        }
        int size = Math.min(length, plainLength);
        System.arraycopy(plain, plainOffset, output, offset, size);
        plainOffset += size;
        plainLength -= size;
        return size;
    }

    private void step()
            throws IOException
    {
        while (!inputEnded && pendingLength < want) {
            if (pending.length < want) {
                pending = java.util.Arrays.copyOf(pending, want);
            }
            int size = in.read(pending, pendingLength, want - pendingLength);
            if (size < 0) {
                inputEnded = true;
            }
            else {
                pendingLength += size;
            }
        }
        if (inputEnded && pendingLength == 0 && !first) {
            finished = true;
            return;
        }
        int flags = (first ? HipNative.WINDOW_FIRST : 0) | (inputEnded ? HipNative.WINDOW_LAST : 0);
        int status;
        try (Arena call = Arena.ofConfined()) {
            MemorySegment source = call.allocate(Math.max(pendingLength, 1));
            MemorySegment target = call.allocate(plain.length);
            MemorySegment.copy(pending, 0, source, ValueLayout.JAVA_BYTE, 0, pendingLength);
            status = context.window(false, op, flags, source, pendingLength, target, plain.length, result);
            plainOffset = 0;
            plainLength = (int) result.get(ValueLayout.JAVA_LONG, 8);
            MemorySegment.copy(target, ValueLayout.JAVA_BYTE, 0, plain, 0, plainLength);
        }
        int consumed = (int) result.get(ValueLayout.JAVA_LONG, 0);
        int stop = result.get(ValueLayout.JAVA_INT, 16);
        long need = result.get(ValueLayout.JAVA_LONG, 24);
        System.arraycopy(pending, consumed, pending, 0, pendingLength - consumed);
        pendingLength -= consumed;
        first = first && consumed == 0;
        if (stop == HipNative.STOP_FAILED) {
            failure = HipNative.toException(status, position + result.get(ValueLayout.JAVA_LONG, 32));
            return;
        }
        position += consumed;
        want = windowBytes;
        if (stop == HipNative.STOP_NEED_INPUT && consumed == 0) {
            want = (int) Math.min(Integer.MAX_VALUE - 8, Math.max((long) pendingLength + windowBytes, need));  // grown only as far as the unit asks
        }
        else if (stop == HipNative.STOP_NEED_ROOM && plainLength == 0 && consumed == 0) {
            plain = new byte[(int) Math.max(need, (long) plain.length + 1)];
        }
        else if (stop == HipNative.STOP_END && inputEnded && pendingLength == 0) {
            finished = true;
        }
    }

    @Override
    public void close()
            throws IOException
    {
        if (!closed) {
            closed = true;
            try {
                in.close();
            }
            finally {
                arena.close();
                context.close();
            }
        }
    }
}
