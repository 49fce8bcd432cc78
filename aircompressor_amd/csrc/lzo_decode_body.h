// lzo_decode_body.h -- one command of the LZO1X grammar as M/lzo/LzoRawDecompressor.java:52-349 reads it, without the copies.  Every check of the Java loop
// depends on lengths, offsets and positions only -- never on a decoded byte -- so this walk alone decides status, error offset and output length of an
// item; the one copy for the two decoders of lzo_decompress.hip and the sizing kernel of decoded_size.hip.
#pragma once
#include "achip_device.h"

namespace achip {
namespace lzod {

// where the walk of an item stands (an item is any number of concatenated blocks: :49-52)
struct Walk {
    int32_t ip;        // input - inputAddress
    int64_t op;        // output - outputAddress
    int32_t lastLit;   // lastLiteralLength :54, :348
    int32_t first;     // firstCommand :53
    int32_t inBlock;   // between a block's first command and its end marker
    int32_t st, eo;    // the item's status and, for a failure, the Java exception's offset
    __device__ __forceinline__ void begin()
    {
        ip = 0;
        op = 0;
        lastLit = 0;
        first = 1;
        inBlock = 0;
        st = 0;
        eo = 0;
    }
};

constexpr int STEP_COMMAND = 0;  // a command: ml match bytes at offset off (ml == 0: none), then lit literal bytes at in[litPos ..)
constexpr int STEP_END = 1;      // a block's end marker; the item may go on
constexpr int STEP_DONE = 2;     // the item is over: w.st == 0 and every byte consumed, or the failure in w.st / w.eo

// the length-extension chain :91-95, :159-163, :200-204: zero bytes add 255 each (Java int arithmetic: it wraps), the byte that ends the chain is added
__device__ __forceinline__ int32_t extension(const uint8_t* __restrict__ in, int32_t inLimit, int32_t& ip, int32_t base)
{
    uint32_t v = (uint32_t)base;
    uint32_t next = 0;
    while (ip < inLimit && (next = in[ip++]) == 0) {
        v += 255u;
    }
    return (int32_t)(v + next);
}

#define LZOD_FAIL(off)                                                     \
    {                                                                      \
        w.st = mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_LZO_MALFORMED);    \
        w.eo = (int32_t)(off);                                             \
        return STEP_DONE;                                                  \
    }

// One trip of the Java loops.  outLimit: the item's capacity (the sizing walk passes INT32_MAX).
__device__ __forceinline__ int step(const uint8_t* __restrict__ in, int32_t inLimit, int64_t outLimit, Walk& w, int32_t& ml, int32_t& off, int32_t& lit, int32_t& litPos)
{
    int32_t ip = w.ip;
    if (w.inBlock == 0) {  // the outer loop's condition :52
        if (ip >= inLimit) {
            return STEP_DONE;
        }
        w.inBlock = 1;
        w.first = 1;
        w.lastLit = 0;
    }
    if (ip >= inLimit) LZOD_FAIL(ip);  // :56-58
    const int32_t command = (int32_t)in[ip++];
    ml = 0;
    off = 0;
    lit = 0;
    if ((command & 0xF0) == 0) {
        if (w.lastLit == 0) {  // :73-98 four or more literals
            lit = command & 0xF;
            if (lit == 0) {
                lit = extension(in, inLimit, ip, 0xF);
            }
            lit = (int32_t)((uint32_t)lit + 3u);
        }
        else {  // :99-142 two bytes within 1 KiB behind one to three literals, three bytes at 2049 .. 3072 behind four or more
            if (ip >= inLimit) LZOD_FAIL(ip);  // :111-113, :132-134
            off = ((command & 0xC) >> 2) | ((int32_t)in[ip++] << 2);
            ml = w.lastLit <= 3 ? 2 : 3;
            off |= w.lastLit <= 3 ? 0 : 0x800;
            lit = command & 3;
        }
    }
    else if (w.first != 0) {  // :144-149
        lit = command - 17;
    }
    else if ((command & 0xE0) == 0x20) {  // :190-222  0b001M_MMMM
        ml = command & 0x1F;
        if (ml == 0) {
            ml = extension(in, inLimit, ip, 0x1F);
        }
        ml = (int32_t)((uint32_t)ml + 2u);
        if ((int64_t)ip + 2 > inLimit) LZOD_FAIL(ip);  // :209-211
        const int32_t trailer = (int32_t)in[ip] | ((int32_t)in[ip + 1] << 8);
        ip += 2;
        off = trailer >> 2;
        lit = trailer & 3;
    }
    else if ((command & 0xF0) == 0x10) {  // :150-189  0b0001_HMMM
        ml = command & 7;
        if (ml == 0) {
            ml = extension(in, inLimit, ip, 7);
        }
        ml = (int32_t)((uint32_t)ml + 2u);
        if ((int64_t)ip + 2 > inLimit) LZOD_FAIL(ip);  // :168-170
        const int32_t trailer = (int32_t)in[ip] | ((int32_t)in[ip + 1] << 8);
        ip += 2;
        off = ((command & 8) << 11) + (trailer >> 2);
        if (off == 0) {  // :180-183 the last command of the block
            w.ip = ip;
            w.inBlock = 0;
            return STEP_END;
        }
        off += 0x3FFF;
        lit = trailer & 3;
    }
    else {  // :223-244  0bMMMD_DDLL (every byte that is left has one of its two high bits set: the branch of :245-248 is never taken)
        ml = ((command & 0xE0) >> 5) + 1;
        if (ip >= inLimit) LZOD_FAIL(ip);  // :235-237
        off = ((command & 0x1C) >> 2) | ((int32_t)in[ip++] << 3);
        lit = command & 3;
    }
    w.first = 0;
    if (ml < 0) LZOD_FAIL(ip);  // :251-253
    int64_t op = w.op;
    if (ml != 0) {  // :256-263
        off++;
        if (op - off < 0 || op + ml > outLimit) LZOD_FAIL(ip);
        op += ml;
    }
    if (lit < 0) LZOD_FAIL(ip);                                                // :323-325
    if (op + lit > outLimit || (int64_t)ip + lit > inLimit) LZOD_FAIL(ip);  // :327-330
    litPos = ip;
    w.ip = ip + lit;
    w.op = op + lit;
    w.lastLit = lit;
    return STEP_COMMAND;
}
#undef LZOD_FAIL

}  // namespace lzod
}  // namespace achip
