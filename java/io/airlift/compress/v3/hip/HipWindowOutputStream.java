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
import java.io.OutputStream;
import java.lang.foreign.Arena;
import java.lang.foreign.MemorySegment;
import java.lang.foreign.ValueLayout;

import static java.util.Objects.checkFromIndexSize;
import static java.util.Objects.requireNonNull;

/**
 * {@code SnappyFramedOutputStream}, {@code Lz4HadoopOutputStream} and {@code SnappyHadoopOutputStream} with the encoders on an AMD GPU (MI355X, gfx950): ONE class
 * over {@code achip_window_compress}, the format chosen by the compress op ({@link HipNative#OP_SNAPPYFRAMED_COMPRESS}, {@link HipNative#OP_LZ4HADOOP_COMPRESS},
 * {@link HipNative#OP_SNAPPYHADOOP_COMPRESS}).  {@code write} collects {@code windowBytes}; a full window is handed to the library, which encodes the whole blocks in
 * it side by side and leaves the partial one for the next call; {@code close} writes the rest.  The bytes on the sink are the Java stream's for the same
 * {@code write}s followed by {@code close}, whatever the sizes of the calls.
 */
public final class HipWindowOutputStream
        extends OutputStream
{
    private final OutputStream out;
    private final HipNative.Context context;
    private final int op;
    private final Arena arena = Arena.ofShared();
    private final MemorySegment result = arena.allocate(ValueLayout.JAVA_LONG, 5);
    private final byte[] pending;
    private int pendingLength;
    private byte[] encoded;
    private boolean first = true;
    private boolean closed;

    public HipWindowOutputStream(OutputStream out, int op, int windowBytes, int device)
    {
        this.out = requireNonNull(out, "out is null");
        if (op != HipNative.OP_SNAPPYFRAMED_COMPRESS && op != HipNative.OP_LZ4HADOOP_COMPRESS && op != HipNative.OP_SNAPPYHADOOP_COMPRESS) {
            throw new IllegalArgumentException("op is not a container compress op");
        }
        if (windowBytes <= 0) {
            throw new IllegalArgumentException("windowBytes must be positive");
        }
        HipNative.verifyEnabled();
        this.context = new HipNative.Context(device);
        this.op = op;
        this.pending = new byte[windowBytes];
        this.encoded = new byte[(int) Math.min(Integer.MAX_VALUE - 8, 2L * windowBytes + 65536)];
    }

    @Override
    public void write(int b)
            throws IOException
    {
        write(new byte[] {(byte) b}, 0, 1);
    }

    @Override
    public void write(byte[] input, int offset, int length)
            throws IOException
    {
        checkFromIndexSize(offset, length, input.length);
        if (closed) {
            throw new IOException("stream is closed");
        }
        while (length > 0) {
            int size = Math.min(length, pending.length - pendingLength);
            System.arraycopy(input, offset, pending, pendingLength, size);
            pendingLength += size;
            offset += size;
            length -= size;
            if (pendingLength == pending.length) {
                flushWindow(false);
                if (pendingLength == pending.length) {
                    throw new IOException("the window is smaller than one block of the stream");
                }
            }
        }
    }

    private void flushWindow(boolean closing)
            throws IOException
    {
        while (true) {
            int flags = (first ? HipNative.WINDOW_FIRST : 0) | (closing ? HipNative.WINDOW_LAST : 0);
            int produced;
            try (Arena call = Arena.ofConfined()) {
                MemorySegment source = call.allocate(Math.max(pendingLength, 1));
                MemorySegment target = call.allocate(encoded.length);
                MemorySegment.copy(pending, 0, source, ValueLayout.JAVA_BYTE, 0, pendingLength);
                int status = context.window(true, op, flags, source, pendingLength, target, encoded.length, result);
                if (status < 0) {
                    throw HipNative.toException(status, 0);
                }
                produced = (int) result.get(ValueLayout.JAVA_LONG, 8);
                MemorySegment.copy(target, ValueLayout.JAVA_BYTE, 0, encoded, 0, produced);
            }
            out.write(encoded, 0, produced);
            int consumed = (int) result.get(ValueLayout.JAVA_LONG, 0);
            int stop = result.get(ValueLayout.JAVA_INT, 16);
            System.arraycopy(pending, consumed, pending, 0, pendingLength - consumed);
            pendingLength -= consumed;
            first = first && produced == 0;
            if (stop != HipNative.STOP_NEED_ROOM) {
                return;
            }
            if (produced == 0 && consumed == 0) {
                encoded = new byte[(int) Math.max(result.get(ValueLayout.JAVA_LONG, 24), (long) encoded.length + 1)];
            }
        }
    }

    @Override
    public void close()
            throws IOException
    {
        if (!closed) {
            closed = true;
            try {
                flushWindow(true);
                out.close();
            }
            finally {
                arena.close();
                context.close();
            }
        }
    }
}
