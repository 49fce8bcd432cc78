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
 * One-shot and batched XXH3 (64- and 128-bit) on an AMD GPU (MI355X, gfx950) through {@code libaircompressor_hip.so}:
 * the GPU siblings of {@code XxHash3Native.hash(MemorySegment, long)} and {@code XxHash3Native.hash128(MemorySegment, long)}.
 * <p>
 * A single host segment is staged through the context's pinned buffer (PCIe-bound; the CPU hashers are the better choice for
 * that).  The batched forms hash many device-resident buffers per call at the HBM read rate; the 128-bit batch writes the low
 * and high halves of buffer i to {@code hashes[2i]} and {@code hashes[2i + 1]}.
 * <p>
 * Binding (added to {@code HipNative.MethodHandles}):
 * <pre>
 * &#64;NativeSignature(name = "achip_xxhash3_64", returnType = int.class, argumentTypes = {MemorySegment.class, MemorySegment.class, long.class, long.class, MemorySegment.class})
 * &#64;NativeSignature(name = "achip_xxhash3_128", returnType = int.class, argumentTypes = {MemorySegment.class, MemorySegment.class, long.class, long.class, MemorySegment.class})
 * &#64;NativeSignature(name = "achip_xxhash3_64_batch", returnType = int.class, argumentTypes = {MemorySegment.class, MemorySegment.class, MemorySegment.class, MemorySegment.class, long.class, MemorySegment.class, int.class})
 * &#64;NativeSignature(name = "achip_xxhash3_128_batch", returnType = int.class, argumentTypes = {MemorySegment.class, MemorySegment.class, MemorySegment.class, MemorySegment.class, long.class, MemorySegment.class, int.class})
 * </pre>
 */
public final class XxHash3Hip
{
    private final HipNative.Context context;

    public XxHash3Hip(int device)
    {
        HipNative.verifyEnabled();
        this.context = new HipNative.Context(device);
    }

    /** {@code XxHash3Native.hash(input, seed)} on the GPU. */
    public long hash(MemorySegment input, long seed)
    {
        try (Arena arena = Arena.ofConfined()) {
            MemorySegment out = arena.allocate(ValueLayout.JAVA_LONG);
            int status = invoke(HipNative.xxhash3(), context.address(), input, input.byteSize(), seed, out);
            HipNative.throwIfError(status, 0);
            return out.get(ValueLayout.JAVA_LONG, 0);
        }
    }

    /** {@code XxHash3Native.hash128(input, seed)} on the GPU. */
    public XxHash128 hash128(MemorySegment input, long seed)
    {
        try (Arena arena = Arena.ofConfined()) {
            MemorySegment out = arena.allocate(ValueLayout.JAVA_LONG, 2);
            int status = invoke(HipNative.xxhash3Hash128(), context.address(), input, input.byteSize(), seed, out);
            HipNative.throwIfError(status, 0);
            return new XxHash128(out.getAtIndex(ValueLayout.JAVA_LONG, 0), out.getAtIndex(ValueLayout.JAVA_LONG, 1));
        }
    }

    /**
     * Hashes {@code count} device-resident buffers: buffer i is {@code base + offsets[i]}, {@code lengths[i]} bytes; {@code hashes[i]}
     * receives its 64-bit hash.  All segments are device memory obtained from {@code HipNative.Context.deviceAlloc}; asynchronous on the
     * context's stream.
     */
    public void hashBatch(MemorySegment base, MemorySegment offsets, MemorySegment lengths, long seed, MemorySegment hashes, int count)
    {
        int status = invoke(HipNative.xxhash3Batch(), context.address(), base, offsets, lengths, seed, hashes, count);
        HipNative.throwIfError(status, 0);
    }

    /** As {@link #hashBatch}, with the 128-bit hash: {@code hashes[2i]} = low, {@code hashes[2i + 1]} = high (2 * count longs). */
    public void hash128Batch(MemorySegment base, MemorySegment offsets, MemorySegment lengths, long seed, MemorySegment hashes, int count)
    {
        int status = invoke(HipNative.xxhash3Hash128Batch(), context.address(), base, offsets, lengths, seed, hashes, count);
        HipNative.throwIfError(status, 0);
    }

    /** {@code XxHash3Native.newHasher(seed)} on the GPU: the streaming form (update / updateLE / digest / reset / close). */
    public Hasher newHasher(long seed)
    {
        return new Hasher(context, seed);
    }

    /** {@code XxHash3Native.newHasher128(seed)} on the GPU. */
    public Hasher128 newHasher128(long seed)
    {
        return new Hasher128(context, seed);
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

    /** The GPU sibling of {@code XxHash3Native.Hasher64Impl} ({@code XxHash3Native.java:220-344}). */
    public static final class Hasher
            extends XxHashHip.StreamingHasher<Hasher>
    {
        Hasher(HipNative.Context context, long seed)
        {
            super(context, XXH3_64, seed);
        }

        @Override
        Hasher self()
        {
            return this;
        }

        public long digest()
        {
            long[] words = digestWords();
            return words[0];
        }
    }

    /** The GPU sibling of the 128-bit streaming hasher of {@code XxHash3Native}: same state and update as {@link Hasher}, another digest. */
    public static final class Hasher128
            extends XxHashHip.StreamingHasher<Hasher128>
    {
        Hasher128(HipNative.Context context, long seed)
        {
            super(context, XXH3_128, seed);
        }

        @Override
        Hasher128 self()
        {
            return this;
        }

        public XxHash128 digest()
        {
            long[] words = digestWords();
            return new XxHash128(words[0], words[1]);
        }
    }
}
