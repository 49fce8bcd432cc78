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
package io.airlift.compress.v3.lzo;

import io.airlift.compress.v3.Decompressor;
import io.airlift.compress.v3.MalformedInputException;
import io.airlift.compress.v3.hip.HipNative;

import java.lang.foreign.MemorySegment;

import static java.lang.Math.toIntExact;
import static java.lang.String.format;
import static java.util.Objects.requireNonNull;

/**
 * LZO1X block decompressor running on an AMD GPU (MI355X, gfx950) through {@code libaircompressor_hip.so}.
 * Drop-in for {@code LzoDecompressor}: the kernel walks the format with the Java decoder's checks in
 * the Java decoder's order, so corrupt input raises the same {@link MalformedInputException} (reason and offset) --
 * a destination that is too small included: that is a MalformedInputException in this decoder.  An input may hold
 * any number of concatenated blocks.
 * <p>
 * Not thread-safe (owns one HIP stream).  For throughput use {@link io.airlift.compress.v3.hip.HipBatchCodec}.
 */
public final class LzoHipDecompressor
        implements Decompressor
{
    private final HipNative.Context context;

    public LzoHipDecompressor()
    {
        this(0);
    }

    public LzoHipDecompressor(int device)
    {
        HipNative.verifyEnabled();
        this.context = new HipNative.Context(device);
    }

    public static boolean isEnabled()
    {
        return HipNative.isEnabled();
    }

    @Override
    public int decompress(byte[] input, int inputOffset, int inputLength, byte[] output, int outputOffset, int maxOutputLength)
            throws MalformedInputException
    {
        verifyRange(input, inputOffset, inputLength);
        verifyRange(output, outputOffset, maxOutputLength);
        MemorySegment inputSegment = MemorySegment.ofArray(input).asSlice(inputOffset, inputLength);
        MemorySegment outputSegment = MemorySegment.ofArray(output).asSlice(outputOffset, maxOutputLength);
        return context.singleBlock(HipNative.OP_LZO_DECOMPRESS, inputSegment, inputLength, outputSegment, maxOutputLength);
    }

    @Override
    public int decompress(MemorySegment input, MemorySegment output)
            throws MalformedInputException
    {
        return context.singleBlock(HipNative.OP_LZO_DECOMPRESS, input, toIntExact(input.byteSize()), output, toIntExact(output.byteSize()));
    }

    private static void verifyRange(byte[] data, int offset, int length)
    {
        requireNonNull(data, "data is null");
        if (offset < 0 || length < 0 || offset + length > data.length) {
            throw new IllegalArgumentException(format("Invalid offset or length (%s, %s) in array of length %s", offset, length, data.length));
        }
    }
}
