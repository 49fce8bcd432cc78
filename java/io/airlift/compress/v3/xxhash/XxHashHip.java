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
package io.airlift.compress.v3.xxhash;

import io.airlift.compress.v3.hip.HipNative;

import java.lang.foreign.Arena;
import java.lang.foreign.MemorySegment;
import java.lang.foreign.ValueLayout;
import java.lang.invoke.MethodHandle;

/**
 * One-shot and batched XXH64 / XXH32 on an AMD GPU (MI355X, gfx950) through {@code libaircompressor_hip.so}:
 * the GPU siblings of {@code XxHash64Hasher.hash(MemorySegment, long)} and {@code XxHash32Hasher.hash(MemorySegment, int)}.
 * <p>
 * A single host segment is staged through the context's pinned buffer (PCIe-bound; the CPU hashers are the better
 * choice for that).  The batched form hashes many device-resident buffers per call -- block / content checksums of
 * containers whose blocks already live in HBM -- at the HBM read rate.
 * <p>
 * Binding (added to {@code HipNative.MethodHandles}):
 * <pre>
 * &#64;NativeSignature(name = "achip_xxhash64", returnType = int.class, argumentTypes = {MemorySegment.class, MemorySegment.class, long.class, long.class, MemorySegment.class})
 * &#64;NativeSignature(name = "achip_xxhash32", returnType = int.class, argumentTypes = {MemorySegment.class, MemorySegment.class, long.class, int.class, MemorySegment.class})
 * &#64;NativeSignature(name = "achip_xxhash64_batch", returnType = int.class, argumentTypes = {MemorySegment.class, MemorySegment.class, MemorySegment.class, MemorySegment.class, long.class, MemorySegment.class, int.class})
 * &#64;NativeSignature(name = "achip_xxhash32_batch", returnType = int.class, argumentTypes = {MemorySegment.class, MemorySegment.class, MemorySegment.class, MemorySegment.class, int.class, MemorySegment.class, int.class})
 * </pre>
 * The streaming form ({@code create64(seed)} / {@code create32(seed)}: update, updateLE, digest, reset, close) binds {@code achip_hasher_create / _update /
 * _digest / _reset / _destroy}; batches of states in device memory are {@code achip_hash_states_reset / _update / _digest} over
 * {@code achip_hash_state_size(algo)}-byte records.
 */
public final class XxHashHip
{
    private final HipNative.Context context;

    public XxHashHip(int device)
    {
        HipNative.verifyEnabled();
        this.context = new HipNative.Context(device);
    }

    /** {@code XxHash64Hasher.hash(input, seed)} on the GPU. */
    public long hash64(MemorySegment input, long seed)
    {
        try (Arena arena = Arena.ofConfined()) {
            MemorySegment out = arena.allocate(ValueLayout.JAVA_LONG);
            int status = invoke(HipNative.xxhash64(), context.address(), input, input.byteSize(), seed, out);
            HipNative.throwIfError(status, 0);
            return out.get(ValueLayout.JAVA_LONG, 0);
        }
    }

    /** {@code XxHash32Hasher.hash(input, seed)} on the GPU. */
    public int hash32(MemorySegment input, int seed)
    {
        try (Arena arena = Arena.ofConfined()) {
            MemorySegment out = arena.allocate(ValueLayout.JAVA_INT);
            int status = invoke(HipNative.xxhash32(), context.address(), input, input.byteSize(), seed, out);
            HipNative.throwIfError(status, 0);
            return out.get(ValueLayout.JAVA_INT, 0);
        }
    }

    /**
     * Hashes {@code count} device-resident buffers: buffer i is {@code base + offsets[i]}, {@code lengths[i]} bytes;
     * all segments are device memory obtained from {@code HipNative.Context.deviceAlloc}; asynchronous on the context's stream.
     */
    public void hash64Batch(MemorySegment base, MemorySegment offsets, MemorySegment lengths, long seed, MemorySegment hashes, int count)
    {
        int status = invoke(HipNative.xxhash64Batch(), context.address(), base, offsets, lengths, seed, hashes, count);
        HipNative.throwIfError(status, 0);
    }

    /** {@code XxHash64Hasher.create(seed)} on the GPU: the streaming form (update / updateLE / digest / reset / close). */
    public Hasher64 create64(long seed)
    {
        return new Hasher64(context, seed);
    }

    /** {@code XxHash32Hasher.create(seed)} on the GPU. */
    public Hasher32 create32(int seed)
    {
        return new Hasher32(context, seed);
    }

    private static int invoke(MethodHandle handle, Object... arguments)
    {
        try {
            return (int) handle.invokeWithArguments(arguments);
        }
        catch (Throwable t) {
            throw new AssertionError("should not reach here", t);
        }
    }

    /**
     * What the four streaming hashers share: one native hasher ({@code achip_hasher_*}: a state in device memory, the bytes of every update
     * staged through the context's pinned buffer in chunks, so a segment may be longer than 2 GiB).  {@code update} and {@code digest} block;
     * {@code digest} leaves the state as it is.  The method set is the reference's ({@code XxHash64Hasher.java:91-169}): update, updateLE,
     * digest, reset, close; use after {@code close()} throws {@code IllegalStateException} as {@code checkNotClosed} does.
     */
    abstract static class StreamingHasher<T extends StreamingHasher<T>>
            implements AutoCloseable
    {
        static final int XXH32 = 0;
        static final int XXH64 = 1;
        static final int XXH3_64 = 2;
        static final int XXH3_128 = 3;

        private final MemorySegment hasher;
        private boolean closed;

        StreamingHasher(HipNative.Context context, int algorithm, long seed)
        {
            try {
                MemorySegment created = (MemorySegment) HipNative.hasherCreate().invokeWithArguments(context.address(), algorithm, seed);
                if (created.address() == 0) {
                    throw new IllegalStateException("achip_hasher_create failed");
                }
                this.hasher = created;
            }
            catch (RuntimeException | Error e) {
                throw e;
            }
            catch (Throwable t) {
                throw new AssertionError("should not reach here", t);
            }
        }

        abstract T self();

        public T update(byte[] input)
        {
            return update(input, 0, input.length);
        }

        public T update(byte[] input, int offset, int length)
        {
            java.util.Objects.checkFromIndexSize(offset, length, input.length);
            try (Arena arena = Arena.ofConfined()) {
                MemorySegment copy = arena.allocate(Math.max(length, 1));
                MemorySegment.copy(input, offset, copy, ValueLayout.JAVA_BYTE, 0, length);
                return update(copy.asSlice(0, length));
            }
        }

        public T update(MemorySegment input)
        {
            checkNotClosed();
            HipNative.throwIfError(call(HipNative.hasherUpdate(), hasher, input, input.byteSize()), 0);
            return self();
        }

        public T updateLE(long value)
        {
            try (Arena arena = Arena.ofConfined()) {
                MemorySegment bytes = arena.allocate(Long.BYTES);
                bytes.set(ValueLayout.JAVA_LONG_UNALIGNED.withOrder(java.nio.ByteOrder.LITTLE_ENDIAN), 0, value);
                return update(bytes);
            }
        }

        public T updateLE(int value)
        {
            try (Arena arena = Arena.ofConfined()) {
                MemorySegment bytes = arena.allocate(Integer.BYTES);
                bytes.set(ValueLayout.JAVA_INT_UNALIGNED.withOrder(java.nio.ByteOrder.LITTLE_ENDIAN), 0, value);
                return update(bytes);
            }
        }

        /** low word in [0] (XXH32: zero-extended), the high half of XXH3-128 in [1] */
        long[] digestWords()
        {
            checkNotClosed();
            try (Arena arena = Arena.ofConfined()) {
                MemorySegment out = arena.allocate(ValueLayout.JAVA_LONG, 2);
                HipNative.throwIfError(call(HipNative.hasherDigest(), hasher, out), 0);
                return new long[] {out.getAtIndex(ValueLayout.JAVA_LONG, 0), out.getAtIndex(ValueLayout.JAVA_LONG, 1)};
            }
        }

        public T reset()
        {
            return reset(0);
        }

        public T reset(long seed)
        {
            checkNotClosed();
            HipNative.throwIfError(call(HipNative.hasherReset(), hasher, seed), 0);
            return self();
        }

        @Override
        public void close()
        {
            if (!closed) {
                closed = true;
                call(HipNative.hasherDestroy(), hasher);
            }
        }

        private void checkNotClosed()
        {
            if (closed) {
                throw new IllegalStateException("Hasher has been closed");
            }
        }

        private static int call(MethodHandle handle, Object... arguments)
        {
            try {
                return (int) handle.invokeWithArguments(arguments);
            }
            catch (Throwable t) {
                throw new AssertionError("should not reach here", t);
            }
        }
    }

    /** The GPU sibling of a streaming {@code XxHash64Hasher} ({@code XxHash64Hasher.java:91-169}). */
    public static final class Hasher64
            extends StreamingHasher<Hasher64>
    {
        Hasher64(HipNative.Context context, long seed)
        {
            super(context, XXH64, seed);
        }

        @Override
        Hasher64 self()
        {
            return this;
        }

        public long digest()
        {
            long[] words = digestWords();
            return words[0];
        }
    }

    /** The GPU sibling of a streaming {@code XxHash32Hasher}; the seed is the low 32 bits. */
    public static final class Hasher32
            extends StreamingHasher<Hasher32>
    {
        Hasher32(HipNative.Context context, long seed)
        {
            super(context, XXH32, seed);
        }

        @Override
        Hasher32 self()
        {
            return this;
        }

        public int digest()
        {
            long[] words = digestWords();
            return (int) words[0];
        }
    }
}
