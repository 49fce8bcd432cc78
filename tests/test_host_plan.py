"""The host side's decisions that are arithmetic -- achip_host_plan.h (chunk cutter, copy tasks, the look at a block's first tokens) and achip_zstd_frame.h
(frame header, block header, the blocks of a step) -- compiled WITHOUT HIP into one small program under AddressSanitizer and UBSan (no GPU, nothing loaded
into Python) and asked directly.  The program prints `name: values` lines; the tests compare them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aircompressor_amd", "csrc")

PROGRAM = r"""
#include "achip_host_plan.h"
#include "achip_zstd_frame.h"
#include <cstdio>
#include <string>
using namespace achip;
using plan::ChunkPlan;
using plan::HostChunk;
typedef std::vector<uint8_t> Bytes;  // (heap, exactly as long as the stream: one byte past it is the sanitizer's)

static void show(const char* name, const std::vector<long long>& v)
{
    printf("%s:", name);
    for (long long x : v) printf(" %lld", x);
    printf("\n");
}
static std::vector<long long> counts(const ChunkPlan& p)
{
    std::vector<long long> v;
    for (const HostChunk& c : p.chunks) v.push_back(c.count);
    return v;
}
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33) % n;
}
static long long staged(long long n) { return (n + 15) & ~15LL; }

// every property of a plan that does not depend on how the cutter got there; returns what is wrong, or ""
static std::string check_plan(const ChunkPlan& p, const std::vector<int32_t>& order, const std::vector<int32_t>& ops, const std::vector<int32_t>& src,
                              const std::vector<int32_t>& dst, long long chunkBytes, bool ramp)
{
    const long long n = (long long)order.size();
    long long total = 0;
    for (long long j = 0; j < n; j++) total += staged(src[order[j]]) + staged(dst[order[j]]);
    const bool ramped = ramp && total > chunkBytes;
    long long next = 0, done = 0;
    for (size_t k = 0; k < p.chunks.size(); k++) {
        const HostChunk& c = p.chunks[k];
        if (c.first != next || c.count < 1) return "items are not covered once, in order";
        long long limit = chunkBytes;
        if (ramped) {
            const long long head = k == 0 ? chunkBytes / 4 : (k == 1 ? chunkBytes / 2 : chunkBytes);
            limit = std::min(head, std::max(chunkBytes / 4, (total - done) / 2));
        }
        long long s = 0, d = 0;
        for (long long j = c.first; j < c.first + c.count; j++) {
            const int32_t i = order[j];
            if (ops[i] != c.op) return "a chunk of two ops";
            if (p.sOff[j] != s || p.dOff[j] != d || (s & 15) || (d & 15)) return "offsets overlap, leave gaps or are not 16-aligned";
            s += staged(src[i]);
            d += staged(dst[i]);
        }
        done += s + d;
        if (s != c.srcBytes || d != c.dstBytes) return "srcBytes / dstBytes";
        if (c.count > 1 && s + d > limit) return "a chunk of several items beyond its limit";
        if (k + 1 < p.chunks.size() && p.chunks[k + 1].op == c.op) {  // (closed for the limit, not for the op: the next item did not fit)
            const int32_t i = order[c.first + c.count];
            if (s + d + staged(src[i]) + staged(dst[i]) <= limit) return "a chunk closed although the next item fitted";
        }
        // the slot: inputs, what the kernels read, | what they write, outputs
        if (c.oSrcOff < c.srcBytes || c.oDstOff != c.oSrcOff + 8 * c.count || c.oSrcLen != c.oDstOff + 8 * c.count || c.oDstCap != c.oSrcLen + 4 * c.count ||
            c.inEnd != c.oDstCap + 4 * c.count) return "upload range";
        if (c.oErr < c.inEnd || (c.oErr & 63) || c.oOutLen != c.oErr + 8 * c.count || c.oStatus != c.oOutLen + 4 * c.count || c.oDst < c.oStatus + 4 * c.count || (c.oDst & 63) ||
            c.end != c.oDst + c.dstBytes) return "download range";
        if (p.maxSlot < c.end + 64) return "maxSlot";
        next += c.count;
    }
    return next == n ? "" : "items left over";
}

static void cutter()
{
    std::vector<int32_t> len(20, 100);
    ChunkPlan p = plan::cut_chunks(10, nullptr, nullptr, 0, len.data(), len.data(), 1000, false);
    show("cut.plain.counts", counts(p));
    const HostChunk& c = p.chunks[0];
    show("cut.plain.first", {c.srcBytes, c.oSrcOff, c.oDstOff, c.oSrcLen, c.oDstCap, c.inEnd, c.oErr, c.oOutLen, c.oStatus, c.oDst, c.end});
    show("cut.plain.maxslot_ok", {p.maxSlot >= c.end + 64});
    const int32_t ops[10] = {0, 0, 1, 1, 1, 1, 1, 1, 1, 1};
    p = plan::cut_chunks(10, nullptr, ops, 0, len.data(), len.data(), 1000, false);
    std::vector<long long> ranges;
    for (const HostChunk& k : p.chunks) ranges.insert(ranges.end(), {k.first, k.first + k.count - 1, k.op});
    show("cut.ops.ranges", ranges);
    show("cut.ramp.counts", counts(plan::cut_chunks(20, nullptr, nullptr, 0, len.data(), len.data(), 1024, true)));
    show("cut.ramp.small_total", counts(plan::cut_chunks(4, nullptr, nullptr, 0, len.data(), len.data(), 1024, true)));  // 896 bytes in all
    show("cut.ramp.total_equals_chunk", counts(plan::cut_chunks(4, nullptr, nullptr, 0, len.data(), len.data(), 896, true)));
    std::vector<int32_t> neg(5, 7);
    neg[3] = -1;
    show("cut.negative", {plan::cut_chunks(5, nullptr, nullptr, 0, neg.data(), len.data(), 1000, false).negativeLength,
                          plan::cut_chunks(5, nullptr, nullptr, 0, len.data(), neg.data(), 1000, true).negativeLength,
                          plan::cut_chunks(5, nullptr, nullptr, 0, len.data(), len.data(), 1000, true).negativeLength});
    // seeded random batches: mixed ops in bucketed order, lengths 0 .. 5 x chunkBytes, ramp on and off
    long long cases = 0, bad = 0;
    std::string firstBad;
    for (int t = 0; t < 400; t++) {
        const int n = 1 + (int)rnd(40);
        const long long chunkBytes = 64 + rnd(4000);
        const bool ramp = (t & 1) != 0;
        std::vector<int32_t> ops2(n), src(n), dst(n), order;
        for (int i = 0; i < n; i++) {
            ops2[i] = (int32_t)rnd(3) * 2;
            const uint32_t top = rnd(4) == 0 ? (uint32_t)(5 * chunkBytes) : (uint32_t)(chunkBytes / 3);
            src[i] = (int32_t)rnd(top + 1);
            dst[i] = (int32_t)rnd(top + 1);
        }
        for (int o = 0; o < 6; o++) {
            for (int i = 0; i < n; i++) {
                if (ops2[i] == o) order.push_back(i);
            }
        }
        const ChunkPlan q = plan::cut_chunks(n, order.data(), ops2.data(), 0, src.data(), dst.data(), chunkBytes, ramp);
        const std::string what = q.negativeLength ? "refused" : check_plan(q, order, ops2, src, dst, chunkBytes, ramp);
        cases++;
        if (!what.empty()) {
            if (bad++ == 0) firstBad = "case " + std::to_string(t) + ": " + what;
        }
    }
    show("cut.random.cases_bad", {cases, bad});
    printf("cut.random.first_bad:%s\n", firstBad.c_str());
}

static void copy_cuts()
{
    auto cuts = [](long long first, std::vector<long long> bytes) {
        std::vector<long long> v;
        for (int64_t x : plan::copy_cuts(first, (int64_t)bytes.size(), [&](int64_t j) { return (int64_t)bytes[(size_t)(j - first)]; })) v.push_back(x);
        return v;
    };
    const long long K = 1024;
    show("copy.seven_of_100k", cuts(5, std::vector<long long>(7, 100 * K)));  // 300 KiB, 300 KiB, and the last group closed
    show("copy.three_of_256k", cuts(0, std::vector<long long>(3, 256 * K)));  // a task each, no empty task behind them
    show("copy.small", cuts(2, std::vector<long long>(9, 1000)));             // below the grain: one task
    show("copy.one_item", cuts(4, {7}));
    show("copy.one_large_item", cuts(4, {1 << 20}));
}

static void lz4_short(Bytes& b, int n)
{
    for (int i = 0; i < n; i++) b.insert(b.end(), {0x10, 'a', 1, 0});  // one literal, a minimal match
}
static void probes()
{
    Bytes b;
    lz4_short(b, 16);
    show("probe.lz4.sixteen_short", {plan::probe_sequences(false, b.data(), (int64_t)b.size())});
    b.clear();
    lz4_short(b, 7);
    show("probe.lz4.seven_short", {plan::probe_sequences(false, b.data(), (int64_t)b.size())});
    b.clear();
    for (int i = 0; i < 8; i++) {
        b.insert(b.end(), {0xF0, 200});
        b.insert(b.end(), 215, 'x');
        b.insert(b.end(), {1, 0});
    }
    show("probe.lz4.eight_long", {plan::probe_sequences(false, b.data(), (int64_t)b.size())});
    // cut inside a length extension: what the counts so far say, and not a byte past the end
    std::vector<long long> cut;
    for (int shorts : {0, 8}) {
        for (int ext = 0; ext < 3; ext++) {
            for (int token : {0xF0, 0x0F}) {
                b.clear();
                lz4_short(b, shorts);
                b.push_back((uint8_t)token);
                if (token == 0x0F) b.insert(b.end(), {1, 0});  // (the match length's extension lies behind the offset)
                b.insert(b.end(), (size_t)ext, 255);
                cut.push_back(plan::probe_sequences(false, b.data(), (int64_t)b.size()));
            }
        }
    }
    show("probe.lz4.cut_in_extension", cut);
    for (int64_t n = 0; n <= 3; n++) {  // any prefix of a long literal run
        Bytes c(b.begin(), b.begin() + (size_t)n);
        (void)plan::probe_sequences(false, c.data(), n);
        (void)plan::probe_sequences(true, c.data(), n);
    }
    b.assign(1, 0x40);
    for (int i = 0; i < 16; i++) b.insert(b.end(), {0x01, 4});  // copy, 1-byte offset, length 4
    show("probe.snappy.sixteen_copies", {plan::probe_sequences(true, b.data(), (int64_t)b.size())});
    b.assign(1, 0x40);
    for (int i = 0; i < 8; i++) {
        b.push_back(59 << 2);  // literal of 60
        b.insert(b.end(), 60, 'y');
    }
    show("probe.snappy.eight_literals", {plan::probe_sequences(true, b.data(), (int64_t)b.size())});
    b.assign({0x40, 63 << 2, 1, 2});  // a literal whose four length bytes are cut short
    show("probe.snappy.cut_in_length", {plan::probe_sequences(true, b.data(), (int64_t)b.size())});
}

static void header_line(const char* name, const Bytes& b, int64_t have = -1)
{
    const zframe::FrameHeader h = zframe::read_frame_header(b.data(), have < 0 ? (int64_t)b.size() : have);
    show(name, {h.state, h.detail, h.offset, h.headerSize, h.singleSegment, h.hasChecksum, h.windowSize, h.contentSize, h.contentBeyondInt64});
}
static void frame_headers()
{
    const uint8_t field[8] = {0x34, 0x12, 0x78, 0x56, 0x01, 0, 0, 0};
    for (int single = 0; single < 2; single++) {
        for (int cs = 0; cs < 4; cs++) {
            Bytes b(1, (uint8_t)((cs << 6) | (single ? 0x20 : 0) | (cs == 2 ? 4 : 0)));  // (cs 2: with checksum)
            if (!single) b.push_back(0x58);  // window: 2 MiB
            const int n = cs == 0 ? single : 1 << cs;
            b.insert(b.end(), field, field + n);
            const std::string name = std::string("header.") + (single ? "single" : "window") + ".cs" + std::to_string(cs);
            header_line(name.c_str(), b);
            if (cs == 3) {
                header_line((name + ".short").c_str(), b, (int64_t)b.size() - 1);
                b.back() = 0x80;
                header_line((name + ".beyond_int64").c_str(), b);
            }
        }
    }
    header_line("header.empty", Bytes(1, 0), 0);
    header_line("header.dictionary_1", Bytes{0x01, 0x58, 9});           // a one-byte dictionary id behind the window descriptor
    header_line("header.dictionary_4", Bytes{0x23, 9, 9, 9, 9, 77});    // single segment, four bytes of id
    header_line("header.dictionary_short", Bytes{0x23, 9, 9, 9, 9, 77}, 5);
    show("header.magic", {zframe::magic_detail(Bytes{0x28, 0xB5, 0x2F, 0xFD}.data()), zframe::magic_detail(Bytes{0x27, 0xB5, 0x2F, 0xFD}.data()),
                          zframe::magic_detail(Bytes{0x28, 0xB5, 0x2F, 0xFC}.data())});
    // the look-back rule: window, content size, both, beyond what the reader keeps
    std::vector<long long> w;
    auto window = [&](int64_t windowSize, int64_t contentSize) {
        zframe::FrameHeader h;
        h.singleSegment = windowSize < 0;
        h.windowSize = windowSize;
        h.contentSize = contentSize;
        const zframe::FrameWindow f = zframe::frame_window(h, 128LL << 20);
        w.push_back(f.lookBack);
        w.push_back(f.windowBeyondJava);
    };
    window(1 << 20, -1);
    window(1 << 20, 5000);
    window(-1, 5000);
    window(-1, 1LL << 40);          // single segment of any size: what the reader keeps
    window(16LL << 20, -1);         // beyond Java's 8 MiB, within the reader's 128
    window(256LL << 20, -1);        // beyond both
    window(256LL << 20, 1000);      // ... but the content is small
    window(-1, -1);                 // (a single-segment frame whose size reads "not set")
    show("header.window", w);
}

static void block(Bytes& b, int type, int size, bool last, int64_t payload)
{
    const int32_t h = (size << 3) | (type << 1) | (last ? 1 : 0);
    b.insert(b.end(), {(uint8_t)h, (uint8_t)(h >> 8), (uint8_t)(h >> 16)});
    b.insert(b.end(), (size_t)payload, 0x11);
}
static void step_line(const char* name, const Bytes& b, bool hasChecksum, bool beyondJava, int32_t maxBlocks, int64_t have = -1)
{
    const zframe::Step s = zframe::list_step(b.data(), have < 0 ? (int64_t)b.size() : have, hasChecksum, beyondJava, maxBlocks);
    std::vector<long long> v = {(long long)s.blocks.size(), s.bytes, s.closing, s.expected, s.broken};
    if (s.blocks.size() <= 3) {
        for (const zframe::StepBlock& k : s.blocks) v.insert(v.end(), {k.header, (long long)k.dataPos, k.dataLen, k.streamBytes});
    }
    show(name, v);
}
static void steps()
{
    Bytes b;
    block(b, 0, 300000, true, 300000);
    step_line("step.raw_300000", b, false, false, 32);
    step_line("step.raw_300000.beyond_java", b, false, true, 32);
    step_line("step.raw_300000.a_byte_short", b, false, false, 32, (int64_t)b.size() - 1);
    b.clear();
    block(b, 1, 300000, true, 1);
    step_line("step.rle_300000", b, false, false, 32);
    b.clear();
    block(b, 3, 10, false, 10);
    step_line("step.type_3", b, false, false, 32);
    b.clear();
    block(b, 2, 131073, false, 131073);
    step_line("step.compressed_131073", b, false, false, 32);
    b.clear();
    block(b, 2, 131072, false, 131072);
    step_line("step.compressed_131072", b, false, false, 32);
    step_line("step.compressed.beyond_java", b, false, true, 32);
    b.clear();
    block(b, 0, 5, false, 5);
    block(b, 2, 40, true, 40);
    b.insert(b.end(), {0xDD, 0xCC, 0xBB, 0xAA});
    step_line("step.checksum.whole", b, true, false, 32);
    step_line("step.checksum.a_byte_short", b, true, false, 32, (int64_t)b.size() - 1);
    step_line("step.no_checksum.last_block", b, false, false, 32, (int64_t)b.size() - 4);
    b.clear();
    for (int i = 0; i < 33; i++) block(b, 0, 1, false, 1);
    step_line("step.33_blocks", b, false, false, 32);
    step_line("step.header_cut", b, false, false, 32, 4 * 5 + 2);
    // the largest RAW block the three header bytes can say is 2^21 - 1 bytes: 16 parts.  Behind 16 listed blocks the step has room for it, behind 17 it has not.
    for (int ahead : {16, 17}) {
        b.clear();
        for (int i = 0; i < ahead; i++) block(b, 0, 1, false, 1);
        block(b, 0, (1 << 21) - 1, false, (1 << 21) - 1);
        step_line(ahead == 16 ? "step.16_parts_behind_16" : "step.16_parts_behind_17", b, false, false, 32);
    }
    const zframe::BlockHeader h = zframe::read_block_header(Bytes{0x1B, 0x00, 0x10}.data());
    show("step.block_header", {h.type, h.size, h.last, h.stored});
}

int main()
{
    cutter();
    copy_cuts();
    probes();
    frame_headers();
    steps();
    return 0;
}
"""


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    clang = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("no clang++ for the sanitized host build")
    tmp = tmp_path_factory.mktemp("host_plan")
    src, exe = str(tmp / "plan.cpp"), str(tmp / "plan")
    with open(src, "w") as f:
        f.write(PROGRAM)
    # the two headers ALONE: no HIP include path, no -x hip
    subprocess.run([clang, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(":")
        out[name] = rest.strip()
    return out


def ints(printed, name):
    return [int(x) for x in printed[name].split()]


def test_the_two_headers_need_no_hip():
    for name in ("achip_host_plan.h", "achip_zstd_frame.h"):
        text = open(os.path.join(CSRC, name)).read()
        includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
        assert all("hip_runtime" not in i and i not in ('"achip_host.h"', '"achip_launch.h"', '"achip_device.h"') for i in includes), (name, includes)


def test_chunk_cutter_without_ramp(printed):
    """ten items of srcLen = dstCap = 100 (112 + 112 staged bytes each), host.chunk_bytes = 1000"""
    assert ints(printed, "cut.plain.counts") == [4, 4, 2]
    #                                           srcBytes oSrcOff oDstOff oSrcLen oDstCap inEnd oErr oOutLen oStatus oDst end
    assert ints(printed, "cut.plain.first") == [448, 448, 480, 512, 528, 544, 576, 608, 624, 640, 1088]
    assert ints(printed, "cut.plain.maxslot_ok") == [1]
    assert ints(printed, "cut.ops.ranges") == [0, 1, 0, 2, 5, 1, 6, 9, 1]  # (first, last, op) per chunk: an op ends a chunk


def test_chunk_cutter_ramp(printed):
    """twenty such items (4 480 staged bytes), host.chunk_bytes = 1024: limit = min(quarter, half, then full) and max(quarter, half of what is left at the
    chunk's first item); a chunk always takes its first item; a total at or below host.chunk_bytes is not ramped"""
    assert ints(printed, "cut.ramp.counts") == [1, 2, 4, 4, 4, 2, 1, 1, 1]
    assert ints(printed, "cut.ramp.small_total") == [4]
    assert ints(printed, "cut.ramp.total_equals_chunk") == [4]


def test_chunk_cutter_invariants_on_random_batches(printed):
    """400 seeded batches (mixed ops in bucketed order, lengths 0 .. 5 x chunkBytes, ramp on and off): every item in exactly one chunk, in order; one op
    per chunk; a chunk of several items within its limit, and closed only when the next item did not fit; offsets 16-aligned and disjoint; the upload range
    [0, inEnd) in front of the download range [oErr, end)"""
    assert ints(printed, "cut.random.cases_bad") == [400, 0], printed["cut.random.first_bad"]


def test_chunk_cutter_refuses_negative_lengths(printed):
    assert ints(printed, "cut.negative") == [1, 1, 0]  # srcLen, dstCap, neither


def test_copy_tasks(printed):
    """one task per >= 256 KiB of consecutive items; the last group is closed; a chunk of one item is one task"""
    assert ints(printed, "copy.seven_of_100k") == [5, 8, 11, 12]
    assert ints(printed, "copy.three_of_256k") == [0, 1, 2, 3]
    assert ints(printed, "copy.small") == [2, 11]
    assert ints(printed, "copy.one_item") == [4, 5]
    assert ints(printed, "copy.one_large_item") == [4, 5]


def test_probe_sequences(printed):
    """1 short, 2 long, 0 cannot tell (fewer than eight sequences); never a byte past the end (the sanitizer is the check)"""
    assert ints(printed, "probe.lz4.sixteen_short") == [1]
    assert ints(printed, "probe.lz4.seven_short") == [0]
    assert ints(printed, "probe.lz4.eight_long") == [2]
    # nothing in front: cannot tell; eight short sequences in front: short -- wherever the extension is cut (literal length, match length; 0, 1, 2 bytes of it)
    assert ints(printed, "probe.lz4.cut_in_extension") == [0] * 6 + [1] * 6
    assert ints(printed, "probe.snappy.sixteen_copies") == [1]
    assert ints(printed, "probe.snappy.eight_literals") == [2]
    assert ints(printed, "probe.snappy.cut_in_length") == [0]


OK, NEED_MORE, FAILED = 0, 1, 2
D_ZSTD_DICTIONARY = 38  # include/aircompressor_hip.h


def test_read_frame_header(printed):
    """fields: state detail offset headerSize singleSegment hasChecksum windowSize contentSize contentBeyondInt64 (offsets count from the descriptor byte:
    achip_zstd_decompressed_size reports them + 4)"""
    w = 2 << 20
    assert ints(printed, "header.window.cs0") == [OK, 0, 2, 2, 0, 0, w, -1, 0]
    assert ints(printed, "header.window.cs1") == [OK, 0, 2, 4, 0, 0, w, 0x1234 + 256, 0]
    assert ints(printed, "header.window.cs2") == [OK, 0, 2, 6, 0, 1, w, 0x56781234, 0]
    assert ints(printed, "header.window.cs3") == [OK, 0, 2, 10, 0, 0, w, 0x156781234, 0]
    assert ints(printed, "header.single.cs0") == [OK, 0, 1, 2, 1, 0, -1, 0x34, 0]
    assert ints(printed, "header.single.cs1") == [OK, 0, 1, 3, 1, 0, -1, 0x1234 + 256, 0]
    assert ints(printed, "header.single.cs2") == [OK, 0, 1, 5, 1, 1, -1, 0x56781234, 0]
    assert ints(printed, "header.single.cs3") == [OK, 0, 1, 9, 1, 0, -1, 0x156781234, 0]
    # a short header: need more (reported as "not enough input" behind the descriptor byte)
    assert ints(printed, "header.window.cs3.short")[:4] == [NEED_MORE, 0, 1, 10]
    assert ints(printed, "header.single.cs3.short")[:4] == [NEED_MORE, 0, 1, 9]
    assert ints(printed, "header.empty")[:3] == [NEED_MORE, 0, 0]
    # an 8-byte size >= 2^63 is kept apart: "not set" for the window rule, refused by achip_zstd_decompressed_size at the field
    assert ints(printed, "header.window.cs3.beyond_int64") == [OK, 0, 2, 10, 0, 0, w, -1, 1]
    assert ints(printed, "header.single.cs3.beyond_int64") == [OK, 0, 1, 9, 1, 0, -1, -1, 1]
    # a dictionary id: refused behind the id -- achip_zstd_decompressed_size: offsets 7 and 9 of the frame
    assert ints(printed, "header.dictionary_1")[:3] == [FAILED, D_ZSTD_DICTIONARY, 7 - 4]
    assert ints(printed, "header.dictionary_4")[:3] == [FAILED, D_ZSTD_DICTIONARY, 9 - 4]
    assert ints(printed, "header.dictionary_short")[:3] == [NEED_MORE, 0, 1]
    assert ints(printed, "header.magic") == [0, 36, 35]  # good, v0.7, bad


def test_frame_window(printed):
    """(lookBack, windowBeyondJava) pairs; lookBack -1: refused"""
    M = 1 << 20
    assert ints(printed, "header.window") == [M, 0, 5000, 0, 5000, 0, 128 * M, 0, 16 * M, 1, -1, 1, 1000, 1, -1, 0]


def test_list_step(printed):
    """fields: blocks bytes closing expected broken, then per block (up to three) header dataPos dataLen streamBytes; broken: 1 block type, 2 window"""
    K = 131072
    raw = [3, 300003, 1, 0, 0, K << 3, 3, K, K + 3, K << 3, 3 + K, K, K, 37856 << 3, 3 + 2 * K, 37856, 37856]
    assert ints(printed, "step.raw_300000") == raw
    assert ints(printed, "step.raw_300000.beyond_java") == raw  # RAW / RLE blocks pass under a window beyond Java's
    assert ints(printed, "step.raw_300000.a_byte_short") == [0, 0, 0, 0, 0]
    assert ints(printed, "step.rle_300000") == [3, 4, 1, 0, 0, (K << 3) | 2, 3, 1, 4, (K << 3) | 2, 3, 1, 0, (37856 << 3) | 2, 3, 1, 0]
    assert ints(printed, "step.type_3") == [0, 0, 0, 0, 1]
    assert ints(printed, "step.compressed_131073") == [0, 0, 0, 0, 1]
    assert ints(printed, "step.compressed_131072") == [1, K + 3, 0, 0, 0, (K << 3) | 4, 3, K, K + 3]
    assert ints(printed, "step.compressed.beyond_java") == [0, 0, 0, 0, 2]
    # the frame's last block goes with its checksum word: with a byte of it missing the block is not listed (the block in front of it is)
    assert ints(printed, "step.checksum.whole") == [2, 8 + 43, 1, 0xAABBCCDD, 0, 5 << 3, 3, 5, 8, (40 << 3) | 4, 11, 40, 43]
    assert ints(printed, "step.checksum.a_byte_short") == [1, 8, 0, 0, 0, 5 << 3, 3, 5, 8]
    assert ints(printed, "step.no_checksum.last_block")[:5] == [2, 8 + 43, 1, 0, 0]
    assert ints(printed, "step.33_blocks") == [32, 32 * 4, 0, 0, 0]
    assert ints(printed, "step.header_cut") == [5, 20, 0, 0, 0]
    # a block of several parts that the step has no room left for: the step ends in front of it.  (Seventeen parts cannot be written: the size field has 21 bits.)
    assert ints(printed, "step.16_parts_behind_16") == [32, 16 * 4 + 3 + (1 << 21) - 1, 0, 0, 0]
    assert ints(printed, "step.16_parts_behind_17") == [17, 17 * 4, 0, 0, 0]
    assert ints(printed, "step.block_header") == [1, (0x10001B >> 3), 1, 1]
