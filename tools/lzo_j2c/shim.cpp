// C entry points over the reference's LzoRawCompressor / LzoRawDecompressor as tools/j2c.py transliterates them (ref_lzo_gen.h, generated into a temporary
// directory by tools/record_lzo_vectors.py; the Java runtime pieces are oracle/ref/jrt.h).  TEST TOOLING: what the calls do is what LzoCompressor.compress /
// LzoDecompressor.decompress do around the raw codec for native MemorySegments (base == null, address == the segment's address; a fresh table per call).
// Results: >= 0 bytes written; -1 a MalformedInputException (its offset in *err_off), -2 any other exception.
#include "ref_lzo_gen.h"

extern "C" long long lzo_java_compress(const unsigned char* in, long long n, unsigned char* out, long long cap)
{
    jrt::CallScope scope;
    try {
        jarray<jint> table = jarray<jint>::make(RefL::LzoRawCompressor::MAX_TABLE_SIZE);
        return RefL::LzoRawCompressor::compress(nullptr, (jlong)(uintptr_t)in, (jint)n, nullptr, (jlong)(uintptr_t)out, (jlong)cap, table);
    }
    catch (...) {
        return -2;
    }
}

extern "C" long long lzo_java_decompress(const unsigned char* in, long long n, unsigned char* out, long long cap, long long* err_off)
{
    jrt::CallScope scope;
    try {
        return RefL::LzoRawDecompressor::decompress(nullptr, (jlong)(uintptr_t)in, (jlong)(uintptr_t)in + n, nullptr, (jlong)(uintptr_t)out, (jlong)(uintptr_t)out + cap);
    }
    catch (MalformedInputException* e) {
        *err_off = e->getOffset();
        return -1;
    }
    catch (...) {
        return -2;
    }
}
