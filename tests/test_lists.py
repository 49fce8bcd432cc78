"""The container units' list layer (aircompressor_amd/csrc/achip_lists.h).

The carver, compiled with g++: measuring (null base) and assigning lay the same calls out alike, every pointer is aligned for its type and no two
arrays overlap.

The five container scratch sizes: each `*_scratch_bytes` function now returns what its unit's carve uses, where it used to be a hand-summed
formula with slack.  The tables below are what those formulas returned (pure arithmetic, recorded from the last commit that had them) over
N_STREAMS x BUFFER_SIZES / variants; the carved sizes must not exceed them, so no context allocates more than it did.  That they cover what the
kernels touch is true by construction (the launcher carves with the same function) and checked under tools/hostemu, which allocates exactly
these sizes."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_STREAMS = [-1, 0, 1, 2, 3, 5, 7, 15, 16, 17, 63, 64, 65, 1000, 1023, 1024, 1025, 4097, 65536, 1000003, 1048576, 3000001, 2147483647]
BUFFER_SIZES = [1024, 65536, 262143, 262144, 262145, 1048576, 4194305]
LZ4FRAME_VARIANTS = [0, 1, 2, 3]
# rows: N_STREAMS; columns: BUFFER_SIZES
HADOOP_DECOMPRESS = [
    [46407824, 46407824, 46407824, 46407824, 46407824, 47194256, 50339984],
    [46407824, 46407824, 46407824, 46407824, 46407824, 47194256, 50339984],
    [46407824, 46407824, 46407824, 46407824, 46407824, 47194256, 50339984],
    [46670048, 46670048, 46670048, 46670048, 46670048, 48242912, 54534368],
    [46932272, 46932272, 46932272, 46932272, 46932272, 49291568, 58728752],
    [47456720, 47456720, 47456720, 47456720, 47456720, 51388880, 67117520],
    [47981168, 47981168, 47981168, 47981168, 47981168, 53486192, 75506288],
    [50078960, 50078960, 50078960, 50078960, 50078960, 61875440, 109061360],
    [50341184, 50341184, 50341184, 50341184, 50341184, 62924096, 113255744],
    [50603408, 50603408, 50603408, 50603408, 50603408, 63972752, 117450128],
    [62665712, 62665712, 62665712, 62665712, 62665712, 112210928, 310391792],
    [62927936, 62927936, 62927936, 62927936, 62927936, 113259584, 314586176],
    [63190160, 63190160, 63190160, 63190160, 63190160, 114308240, 318780560],
    [308369600, 308369600, 308369600, 308369600, 308369600, 1094801600, 4240529600],
    [314400752, 314400752, 314400752, 314400752, 314400752, 1118920688, 4337000432],
    [314662976, 314662976, 314662976, 314662976, 314662976, 1119969344, 4341194816],
    [314662992, 314662992, 314662992, 314662992, 314662992, 1119969360, 4341194832],
    [314712144, 314712144, 314712144, 314712144, 314712144, 1120018512, 4341243984],
    [315695168, 315695168, 315695168, 315695168, 315695168, 1121001536, 4342227008],
    [330646640, 330646640, 330646640, 330646640, 330646640, 1135953008, 4357178480],
    [331423808, 331423808, 331423808, 331423808, 331423808, 1136730176, 4357955648],
    [362646608, 362646608, 362646608, 362646608, 362646608, 1167952976, 4389178448],
    [34674384944, 34674384944, 34674384944, 34674384944, 34674384944, 35479691312, 38700916784],
]
HADOOP_COMPRESS = [138420364, 138420364, 138420364, 138420376, 138420388, 138420412, 138420436, 138420532, 138420544, 138420556, 138421108, 138421120, 138421132, 138432352, 138432628, 138432640, 138432652, 138469516, 139206784, 150420388, 151003264, 174420364, 25908224116]
SNAPPYFRAMED_DECOMPRESS = [54534172, 54534172, 54534172, 54534200, 54534228, 54534284, 54534340, 54534564, 54534592, 54534620, 54535908, 54535936, 54535964, 54562144, 54562788, 54562816, 54562844, 54648860, 56369152, 82534228, 83894272, 138534172, 60184076260]
SNAPPYFRAMED_COMPRESS = [382017552, 382017552, 382017552, 382017568, 382017584, 382017616, 382017648, 382017776, 382017792, 382017808, 382018544, 382018560, 382018576, 382033536, 382033904, 382033920, 382033936, 382083088, 383066112, 398017584, 398794752, 430017552, 34741755888]
# rows: N_STREAMS; columns: LZ4FRAME_VARIANTS
LZ4FRAME_DECOMPRESS = [
    [4096, 41951304, 41951304, 4096],
    [4096, 41951304, 41951304, 4096],
    [4096, 41951304, 41951304, 4096],
    [4096, 41951312, 41951312, 4096],
    [4096, 41951320, 41951320, 4096],
    [4096, 41951336, 41951336, 4096],
    [4096, 41951352, 41951352, 4096],
    [4096, 41951416, 41951416, 4096],
    [4096, 41951424, 41951424, 4096],
    [4096, 41951432, 41951432, 4096],
    [4096, 41951800, 41951800, 4096],
    [4096, 41951808, 41951808, 4096],
    [4096, 41951816, 41951816, 4096],
    [4096, 41959296, 41959296, 4096],
    [4096, 41959480, 41959480, 4096],
    [4096, 41959488, 41959488, 4096],
    [4096, 41959496, 41959496, 4096],
    [4096, 41984072, 41984072, 4096],
    [4096, 42475584, 42475584, 4096],
    [4096, 49951320, 49951320, 4096],
    [4096, 50339904, 50339904, 4096],
    [4096, 65951304, 65951304, 4096],
    [4096, 17221820472, 17221820472, 4096],
]

DRIVER = r"""
#define ACHIP_LISTS_LAYOUT_ONLY 1
#include "achip_lists.h"
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>
using namespace achip::lists;

struct Probe {  // what a unit's carve looks like: counters, per-stream arrays of odd lengths, both lists, a byte slab behind them
    int32_t* counters; int64_t* wide; int32_t* narrow; uint8_t* bytes; uint16_t* halves; ChunkBatch batch; WriterList writer, writerNoSerial; uint8_t* slab;
    void carve(Carver& k, int64_t n)
    {
        counters = k.take<int32_t>(COUNTER_WORDS);
        wide = k.take<int64_t>(n);
        narrow = k.take<int32_t>(n);
        bytes = k.take<uint8_t>(n);
        halves = k.take<uint16_t>(n);
        batch.carve(k, counters);
        writer.carve(k, counters, n, true);
        writerNoSerial.carve(k, counters, n, false);
        slab = k.take<uint8_t>(3 * n + 1);
    }
};

static std::vector<std::pair<int64_t, int64_t>> spans;  // [offset, end) of every array
static bool fail = false;
template <class T>
static void note(const uint8_t* base, const T* p, int64_t count)
{
    const int64_t off = (const uint8_t*)p - base;
    if (off % (int64_t)alignof(T) != 0 || off % 16 != 0) { printf("misaligned %lld\n", (long long)off); fail = true; }
    spans.push_back({off, off + count * (int64_t)sizeof(T)});
}

int main()
{
    for (int64_t n : {1, 2, 3, 5, 7, 13, 64, 1000, 4097}) {
        Carver measure(nullptr);
        Probe m;
        m.carve(measure, n);
        if (m.counters != nullptr || m.batch.cSrcOff != nullptr || m.writer.bSize != nullptr || m.slab != nullptr) { printf("measuring handed out a pointer\n"); fail = true; }
        std::vector<uint8_t> raw((size_t)measure.used() + 64);
        uint8_t* base = raw.data() + (64 - (uintptr_t)raw.data() % 64) % 64;
        Carver assign(base);
        Probe p;
        p.carve(assign, n);
        if (assign.used() != measure.used()) { printf("measure %lld != assign %lld\n", (long long)measure.used(), (long long)assign.used()); fail = true; }
        if (p.writerNoSerial.sSerial != nullptr || p.batch.counters != p.counters || p.writer.counters != p.counters) { printf("counters / sSerial\n"); fail = true; }
        spans.clear();
        note(base, p.counters, COUNTER_WORDS);
        note(base, p.wide, n); note(base, p.narrow, n); note(base, p.bytes, n); note(base, p.halves, n);
        const ChunkBatch& b = p.batch;
        note(base, b.cSrcOff, CAPACITY); note(base, b.cDstOff, CAPACITY); note(base, b.cErrOff, CAPACITY); note(base, b.cSrcLen, CAPACITY);
        note(base, b.cDstCap, CAPACITY); note(base, b.cOutLen, CAPACITY); note(base, b.cStatus, CAPACITY);
        for (const WriterList* w : {&p.writer, &p.writerNoSerial}) {
            note(base, w->sFirst, n); note(base, w->sCount, n); note(base, w->sStatus, n);
            if (w->sSerial != nullptr) note(base, w->sSerial, n);
            note(base, w->bStream, CAPACITY); note(base, w->bIndex, CAPACITY); note(base, w->bSize, CAPACITY);
        }
        note(base, p.slab, 3 * n + 1);
        std::sort(spans.begin(), spans.end());
        for (size_t i = 0; i < spans.size(); i++) {
            if (spans[i].first < 0 || spans[i].second > assign.used() || (i > 0 && spans[i].first < spans[i - 1].second)) { printf("overlap / out of range at %zu\n", i); fail = true; }
        }
        if (spans.back().second != assign.used()) { printf("used() is not the end of the last array\n"); fail = true; }
    }
    printf(fail ? "FAILED\n" : "ok\n");
    return fail ? 1 : 0;
}
"""


def test_carver_measures_what_it_assigns_aligned_and_disjoint(tmp_path):
    src = tmp_path / "lists.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "lists")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aircompressor_amd", "csrc"), "-o", exe, str(src)], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


@pytest.fixture(scope="module")
def sizes():
    import __graft_entry__ as g
    lib = ctypes.CDLL(g.build_library())

    def fn(symbol, nargs):
        f = getattr(lib, symbol)  # (C++ functions of namespace achip: not part of the C ABI, so by their mangled names)
        f.restype = ctypes.c_int64
        f.argtypes = [ctypes.c_int32] * nargs
        return f
    return {
        "hadoop_decompress": fn("_ZN5achip31hadoop_decompress_scratch_bytesEii", 2),
        "hadoop_compress": fn("_ZN5achip29hadoop_compress_scratch_bytesEi", 1),
        "snappyframed_decompress": fn("_ZN5achip37snappyframed_decompress_scratch_bytesEi", 1),
        "snappyframed_compress": fn("_ZN5achip35snappyframed_compress_scratch_bytesEi", 1),
        "lz4frame_decompress": fn("_ZN5achip33lz4frame_decompress_scratch_bytesEii", 2),
    }


def test_carved_scratch_sizes_do_not_exceed_the_old_formulas(sizes):
    for i, n in enumerate(N_STREAMS):
        for j, b in enumerate(BUFFER_SIZES):
            assert 0 < sizes["hadoop_decompress"](n, b) <= HADOOP_DECOMPRESS[i][j], (n, b)
        assert 0 < sizes["hadoop_compress"](n) <= HADOOP_COMPRESS[i], n
        assert 0 < sizes["snappyframed_decompress"](n) <= SNAPPYFRAMED_DECOMPRESS[i], n
        assert 0 < sizes["snappyframed_compress"](n) <= SNAPPYFRAMED_COMPRESS[i], n
        for j, v in enumerate(LZ4FRAME_VARIANTS):
            assert 0 < sizes["lz4frame_decompress"](n, v) <= LZ4FRAME_DECOMPRESS[i][j], (n, v)
