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

import java.lang.foreign.Arena;
import java.lang.foreign.MemorySegment;

import static java.lang.foreign.ValueLayout.JAVA_INT;
import static java.lang.foreign.ValueLayout.JAVA_LONG;

/**
 * Batched entry point: many independent blocks in one call, sharded over the GPUs of a node.
 * <p>
 * Blocks never reference each other (LZ4 offsets stay inside a block, Snappy sub-blocks and Zstd frames are
 * self-contained), so the batch is cut into contiguous slices balanced by bytes, one slice per device, with no
 * collective between devices.  Each device runs its slice on its own {@link HipNative.Context}.
 */
public final class HipBatchCodec
{
    /** Result of one batch: per-block lengths, statuses (0 = ok, negative = ACHIP status) and error offsets. */
    public record Result(int[] outputLength, int[] status, long[] errorOffset) {}

    private final HipNative.Context[] contexts;

    public HipBatchCodec()
    {
        this(HipNative.deviceCount());
    }

    public HipBatchCodec(int devices)
    {
        HipNative.verifyEnabled();
        if (devices < 1 || devices > HipNative.deviceCount()) {
            throw new IllegalArgumentException("devices must be in [1, " + HipNative.deviceCount() + "]");
        }
        contexts = new HipNative.Context[devices];
        for (int i = 0; i < devices; i++) {
            contexts[i] = new HipNative.Context(i);
        }
    }

    /**
     * Runs {@code op} (HipNative.OP_*) over blocks laid out in two host segments.
     * Block i reads {@code source[sourceOffset[i] .. +sourceLength[i])} and writes
     * {@code destination[destinationOffset[i] .. +destinationCapacity[i])}.
     */
    public Result run(int op, MemorySegment source, long[] sourceOffset, int[] sourceLength,
            MemorySegment destination, long[] destinationOffset, int[] destinationCapacity)
    {
        int blocks = sourceOffset.length;
        int[] outputLength = new int[blocks];
        int[] status = new int[blocks];
        long[] errorOffset = new long[blocks];
        int[] starts = partition(sourceLength, destinationCapacity, contexts.length);

        Thread[] workers = new Thread[contexts.length];
        Throwable[] failures = new Throwable[contexts.length];
        for (int d = 0; d < contexts.length; d++) {
            int device = d;
            int first = starts[d];
            int count = starts[d + 1] - first;
            workers[d] = Thread.ofPlatform().start(() -> {
                if (count == 0) {
                    return;
                }
                try (Arena arena = Arena.ofConfined()) {
                    MemorySegment srcOff = arena.allocateFrom(JAVA_LONG, java.util.Arrays.copyOfRange(sourceOffset, first, first + count));
                    MemorySegment srcLen = arena.allocateFrom(JAVA_INT, java.util.Arrays.copyOfRange(sourceLength, first, first + count));
                    MemorySegment dstOff = arena.allocateFrom(JAVA_LONG, java.util.Arrays.copyOfRange(destinationOffset, first, first + count));
                    MemorySegment dstCap = arena.allocateFrom(JAVA_INT, java.util.Arrays.copyOfRange(destinationCapacity, first, first + count));
                    MemorySegment outLen = arena.allocate(JAVA_INT, count);
                    MemorySegment stat = arena.allocate(JAVA_INT, count);
                    MemorySegment errOff = arena.allocate(JAVA_LONG, count);
                    contexts[device].batchHost(op, source, srcOff, srcLen, destination, dstOff, dstCap, outLen, stat, errOff, count);
                    MemorySegment.copy(outLen, JAVA_INT, 0, outputLength, first, count);
                    MemorySegment.copy(stat, JAVA_INT, 0, status, first, count);
                    MemorySegment.copy(errOff, JAVA_LONG, 0, errorOffset, first, count);
                }
                catch (Throwable e) {
                    failures[device] = e;
                }
            });
        }
        for (int d = 0; d < contexts.length; d++) {
            try {
                workers[d].join();
            }
            catch (InterruptedException e) {
                Thread.currentThread().interrupt();
                throw new RuntimeException(e);
            }
            if (failures[d] != null) {
                throw new RuntimeException("device " + d + " failed", failures[d]);
            }
        }
        return new Result(outputLength, status, errorOffset);
    }

    /**
     * The same job in ONE downcall: the library makes the split (the rule of {@link #partition}) and runs every slice on its context in a
     * native host thread ({@code achip_multi_batch_host}); {@code ops} null = every item is {@code op}, otherwise one OP_* per item (a mixed
     * batch: the items of a slice are bucketed by codec inside the library).
     */
    public Result runNative(int op, int[] ops, MemorySegment source, long[] sourceOffset, int[] sourceLength,
            MemorySegment destination, long[] destinationOffset, int[] destinationCapacity)
    {
        int blocks = sourceOffset.length;
        int[] outputLength = new int[blocks];
        int[] status = new int[blocks];
        long[] errorOffset = new long[blocks];
        try (Arena arena = Arena.ofConfined()) {
            MemorySegment opsSegment = ops == null ? MemorySegment.NULL : arena.allocateFrom(JAVA_INT, ops);
            MemorySegment srcOff = arena.allocateFrom(JAVA_LONG, sourceOffset);
            MemorySegment srcLen = arena.allocateFrom(JAVA_INT, sourceLength);
            MemorySegment dstOff = arena.allocateFrom(JAVA_LONG, destinationOffset);
            MemorySegment dstCap = arena.allocateFrom(JAVA_INT, destinationCapacity);
            MemorySegment outLen = arena.allocate(JAVA_INT, Math.max(blocks, 1));
            MemorySegment stat = arena.allocate(JAVA_INT, Math.max(blocks, 1));
            MemorySegment errOff = arena.allocate(JAVA_LONG, Math.max(blocks, 1));
            HipNative.multiBatchHost(contexts, op, opsSegment, source, srcOff, srcLen, destination, dstOff, dstCap, outLen, stat, errOff, blocks, MemorySegment.NULL);
            MemorySegment.copy(outLen, JAVA_INT, 0, outputLength, 0, blocks);
            MemorySegment.copy(stat, JAVA_INT, 0, status, 0, blocks);
            MemorySegment.copy(errOff, JAVA_LONG, 0, errorOffset, 0, blocks);
        }
        return new Result(outputLength, status, errorOffset);
    }

    /**
     * A batch decoded without anybody knowing its sizes: the output, the planned places and the decode's per-item arrays, all in device memory of
     * {@code context} (the decode may still be in flight on its stream); {@code sizeStatus[i] != 0}: sizing found item i damaged and gave it no room.
     */
    public record Unsized(HipNative.Context context, MemorySegment destination, long totalBytes, long leftOut, MemorySegment destinationOffset,
            MemorySegment destinationCapacity, MemorySegment outputLength, MemorySegment status, MemorySegment errorOffset, MemorySegment decodedSize,
            MemorySegment sizeStatus, MemorySegment sizeErrorOffset) {}

    /** achip_decoded_size_batch on the first device: thin and asynchronous like {@link HipNative.Context#launchBatch}; all segments device-accessible. */
    public void decodedSizes(int op, MemorySegment source, MemorySegment sourceOffset, MemorySegment sourceLength, MemorySegment decodedSize, MemorySegment status,
            MemorySegment errorOffset, int blocks)
    {
        contexts[0].decodedSizes(op, source, sourceOffset, sourceLength, decodedSize, status, errorOffset, blocks);
    }

    /** achip_plan_outputs on the first device: the decoders' offsets and capacities from the sizes; {@code total} receives two longs. */
    public void planOutputs(MemorySegment decodedSize, MemorySegment status, int blocks, int align, MemorySegment destinationOffset, MemorySegment destinationCapacity,
            MemorySegment total)
    {
        contexts[0].planOutputs(decodedSize, status, blocks, align, destinationOffset, destinationCapacity, total);
    }

    /**
     * Size, plan, ONE 16-byte readback of the total (the only call here that waits for the device), allocate, decode: for a caller that holds compressed
     * items in device memory and knows nothing else.  The caller frees the segments of the result with {@link HipNative.Context#freeDevice}.
     */
    public Unsized decompressUnsized(int op, MemorySegment source, MemorySegment sourceOffset, MemorySegment sourceLength, int blocks, int align)
    {
        HipNative.Context context = contexts[0];
        long wide = Math.max(8L * blocks, 16);
        long narrow = Math.max(4L * blocks, 16);
        MemorySegment decodedSize = context.allocateDevice(wide);
        MemorySegment sizeStatus = context.allocateDevice(narrow);
        MemorySegment sizeErrorOffset = context.allocateDevice(wide);
        MemorySegment destinationOffset = context.allocateDevice(wide);
        MemorySegment destinationCapacity = context.allocateDevice(narrow);
        MemorySegment outputLength = context.allocateDevice(narrow);
        MemorySegment status = context.allocateDevice(narrow);
        MemorySegment errorOffset = context.allocateDevice(wide);
        MemorySegment total = context.allocateDevice(16);
        long totalBytes = 0;
        long leftOut = 0;
        context.decodedSizes(op, source, sourceOffset, sourceLength, decodedSize, sizeStatus, sizeErrorOffset, blocks);
        context.planOutputs(decodedSize, sizeStatus, blocks, align, destinationOffset, destinationCapacity, total);
        if (blocks > 0) {
            try (Arena arena = Arena.ofConfined()) {
                MemorySegment host = arena.allocate(JAVA_LONG, 2);
                context.copyToHost(host, total, 16);
                context.synchronize();
                totalBytes = host.getAtIndex(JAVA_LONG, 0);
                leftOut = host.getAtIndex(JAVA_LONG, 1);
            }
        }
        context.freeDevice(total);
        MemorySegment destination = context.allocateDevice(Math.max(totalBytes, 16));
        context.launchBatch(op, source, sourceOffset, sourceLength, destination, destinationOffset, destinationCapacity, outputLength, status, errorOffset, blocks);
        return new Unsized(context, destination, totalBytes, leftOut, destinationOffset, destinationCapacity, outputLength, status, errorOffset, decodedSize,
                sizeStatus, sizeErrorOffset);
    }

    /**
     * A batch compressed into one dense buffer: {@code packed} holds {@code totalBytes} bytes, item i at {@code packedOffset[i]} with {@code packedLength[i]}
     * bytes (0: left out -- {@code status[i]} says why); {@code stored[i] == 1} (raw fallback only, else NULL): the item is its plaintext.  All in device
     * memory of {@code context}; the pack may still be in flight on its stream.
     */
    public record Packed(HipNative.Context context, MemorySegment packed, long totalBytes, long leftOut, MemorySegment packedOffset, MemorySegment packedLength,
            MemorySegment stored, MemorySegment outputLength, MemorySegment status, MemorySegment errorOffset) {}

    /**
     * Bounds, plan, a readback of the slots' total, allocate the slots, compress, pack (plan only), a readback of the dense total, allocate exactly that,
     * pack: for a caller whose plaintexts and their lengths live in device memory.  Two calls here wait for the device; nothing is walked on the host.
     * {@code rawFallback}: an item whose compressed form is no smaller than its plaintext is kept as the plaintext.  The caller frees the segments of the
     * result with {@link HipNative.Context#freeDevice}.
     */
    public Packed compressPacked(int op, MemorySegment source, MemorySegment sourceOffset, MemorySegment sourceLength, int blocks, int align, boolean rawFallback)
    {
        HipNative.Context context = contexts[0];
        long wide = Math.max(8L * blocks, 16);
        long narrow = Math.max(4L * blocks, 16);
        MemorySegment bound = context.allocateDevice(wide);
        MemorySegment boundStatus = context.allocateDevice(narrow);
        MemorySegment slotOffset = context.allocateDevice(wide);
        MemorySegment slotCapacity = context.allocateDevice(narrow);
        MemorySegment outputLength = context.allocateDevice(narrow);
        MemorySegment status = context.allocateDevice(narrow);
        MemorySegment errorOffset = context.allocateDevice(wide);
        MemorySegment packedOffset = context.allocateDevice(wide);
        MemorySegment packedLength = context.allocateDevice(narrow);
        MemorySegment stored = rawFallback ? context.allocateDevice(narrow) : MemorySegment.NULL;
        MemorySegment rawBase = rawFallback ? source : MemorySegment.NULL;
        MemorySegment rawOffset = rawFallback ? sourceOffset : MemorySegment.NULL;
        MemorySegment rawLength = rawFallback ? sourceLength : MemorySegment.NULL;
        MemorySegment total = context.allocateDevice(24);
        long slotBytes = 0;
        long totalBytes = 0;
        long leftOut = 0;
        try (Arena arena = Arena.ofConfined()) {
            MemorySegment host = arena.allocate(JAVA_LONG, 3);
            context.compressBounds(op, sourceLength, bound, boundStatus, blocks);
            context.planOutputs(bound, boundStatus, blocks, 1, slotOffset, slotCapacity, total);
            if (blocks > 0) {
                context.copyToHost(host, total, 16);
                context.synchronize();
                slotBytes = host.getAtIndex(JAVA_LONG, 0);
            }
            MemorySegment slots = context.allocateDevice(Math.max(slotBytes, 16));
            context.launchBatch(op, source, sourceOffset, sourceLength, slots, slotOffset, slotCapacity, outputLength, status, errorOffset, blocks);
            context.packOutputs(slots, slotOffset, outputLength, status, rawBase, rawOffset, rawLength, blocks, align, MemorySegment.NULL, 0, packedOffset, packedLength,
                    stored, total);
            if (blocks > 0) {
                context.copyToHost(host, total, 24);
                context.synchronize();
                totalBytes = host.getAtIndex(JAVA_LONG, 0);
                leftOut = host.getAtIndex(JAVA_LONG, 1);
            }
            MemorySegment packed = context.allocateDevice(Math.max(totalBytes, 16));
            context.packOutputs(slots, slotOffset, outputLength, status, rawBase, rawOffset, rawLength, blocks, align, packed, totalBytes, packedOffset, packedLength,
                    stored, total);
            context.synchronize();  // (the slots are read until the copy is done)
            context.freeDevice(slots);
            context.freeDevice(total);
            context.freeDevice(bound);
            context.freeDevice(boundStatus);
            context.freeDevice(slotOffset);
            context.freeDevice(slotCapacity);
            return new Packed(context, packed, totalBytes, leftOut, packedOffset, packedLength, stored, outputLength, status, errorOffset);
        }
    }

    /** Contiguous split balanced by bytes moved (source + destination): achip_partition_blocks itself, so that the split is the library's by construction. */
    static int[] partition(int[] sourceLength, int[] destinationCapacity, int parts)
    {
        long[] weight = new long[sourceLength.length];
        for (int i = 0; i < weight.length; i++) {
            weight[i] = (long) sourceLength[i] + destinationCapacity[i];
        }
        return HipNative.partitionBlocks(weight, parts);
    }
}
