"""achip_ctx_get_stat's rule -- achip_stats.h: which launch leaves which statistic, and at which word of the scratch -- compiled WITHOUT HIP into one small
program under AddressSanitizer and UBSan (no GPU, nothing loaded into Python) and asked for every documented statistic under every kind of last launch.  The
program prints `kind|name: answer` lines; the tests compare them with the tables below, whose word and byte numbers are typed in here (the numbers the
kernels and the reader used before they had names), not taken from the header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aircompressor_amd", "csrc")

PROGRAM = r"""
#include "achip_stats.h"
#include "achip_host_plan.h"
#include <cstdio>
#include <string>
#include <vector>
using namespace achip;
using stats::LastLaunch;
using stats::Located;

static void ask(const char* kind, const LastLaunch& last, const std::string& name)
{
    const std::string heap(name);  // (heap, exactly as long as the name: a byte past it is the sanitizer's)
    const Located at = stats::locate(last, heap.c_str());
    printf("%s|%s: ", kind, name.c_str());
    if (at.words == 0) printf("const %lld\n", (long long)at.value);
    else if (at.pick) printf("pick %lld %d %d %d\n", (long long)at.byteOffset, at.words, at.pickBlocks, at.pickShortLimit);
    else printf("read %lld %d %d\n", (long long)at.byteOffset, at.words, at.word);
}

int main(int argc, char** argv)
{
    std::vector<std::pair<const char*, LastLaunch>> kinds;
    kinds.push_back({"nothing", LastLaunch()});
    kinds.push_back({"block.auto.lz4", LastLaunch::block_decode(16, 12, true, true, -1)});
    kinds.push_back({"block.auto.snappy", LastLaunch::block_decode(4096, 6, true, true, -1)});
    kinds.push_back({"block.auto.remembered_rings", LastLaunch::block_decode(16, 12, true, false, LZ4_PICK_RINGS)});
    kinds.push_back({"block.auto.remembered_twopass", LastLaunch::block_decode(16, 12, true, true, LZ4_PICK_TWOPASS)});
    kinds.push_back({"block.twopass", LastLaunch::block_decode(16, 6, false, true, -1)});
    kinds.push_back({"lzo.twopass", LastLaunch::lzo_decode(true)});
    kinds.push_back({"lzo.wave", LastLaunch::lzo_decode(false)});
    kinds.push_back({"zstd.pipeline", LastLaunch::zstd_decode(16, 1)});
    kinds.push_back({"zstd.one_kernel", LastLaunch::zstd_decode(16, 0)});
    for (const auto& k : kinds) {
        for (int i = 1; i < argc; i++) ask(k.first, k.second, argv[i]);
    }
    // decompress.choice is plan::auto_pick over the probe words with the recorded blocks and short limit: 100 sampled sequences of 32 bytes each (800 units
    // of 4) are short ones for LZ4 (below 12 units) and long ones for Snappy (not below 6); a mixed batch goes to the two passes either way
    const int32_t thirtyTwo[6] = {0, 100, 800, 1, 0, 0}, mixed[6] = {1, 100, 100000, 1, 0, 0};
    for (int k = 1; k <= 2; k++) {  // block.auto.lz4, block.auto.snappy
        const Located at = stats::locate(kinds[k].second, "decompress.choice");
        printf("%s|picked: %d %d\n", kinds[k].first, plan::auto_pick(thirtyTwo, at.pickBlocks, at.pickShortLimit), plan::auto_pick(mixed, 16, at.pickShortLimit));
    }
    printf("names: %d %d\n", LZ4_PICK_RINGS, LZ4_PICK_TWOPASS);
    return 0;
}
"""

KINDS = ("nothing", "block.auto.lz4", "block.auto.snappy", "block.auto.remembered_rings", "block.auto.remembered_twopass", "block.twopass", "lzo.twopass", "lzo.wave",
         "zstd.pipeline", "zstd.one_kernel")
ZSTD_WORDS = {"zstd.decompress.fallback_items": 0, "zstd.decompress.fallback_stage1": 33, "zstd.decompress.fallback_stage2": 34, "zstd.decompress.fallback_stage3": 35,
              "zstd.decompress.fallback_stage4": 36, "zstd.decompress.fallback_stage5": 37, "zstd.decompress.fallback_stage6": 38, "zstd.decompress.long_items": 18,
              "zstd.decompress.multiblock_items": 40, "zstd.decompress.multiblock_blocks": 41, "zstd.decompress.multiblock_fast_items": 42}
SCRATCH_KEPT = ("lz4.decompress.mixed_groups", "decompress.choice", "decompress.twopass_fallback_blocks", "lzo.decompress.fallback_blocks") + tuple(ZSTD_WORDS)
NO_SUCH = ("no.such.statistic", "zstd.decompress.fallback_stage0", "zstd.decompress.fallback_stage7", "zstd.decompress.fallback_stage12", "zstd.decompress.fallback_",
           "zstd.decompress.fallback_stage", "zstd.decompress.", "zstd.decompress.long_items_", "decompress.choice.")

NONE = "const -1"
# everything that is not NONE.  read: byte offset, words read, the word of them that answers; pick: byte offset, words read, blocks, short limit
EXPECTED = {
    ("block.auto.lz4", "lz4.decompress.mixed_groups"): "read 0 1 0",
    ("block.auto.lz4", "decompress.choice"): "pick 0 6 16 12",
    ("block.auto.lz4", "decompress.twopass_fallback_blocks"): "read 4096 3 2",
    ("block.auto.snappy", "lz4.decompress.mixed_groups"): "read 0 1 0",
    ("block.auto.snappy", "decompress.choice"): "pick 0 6 4096 6",
    ("block.auto.snappy", "decompress.twopass_fallback_blocks"): "read 4096 3 2",
    ("block.auto.remembered_rings", "lz4.decompress.mixed_groups"): "read 0 1 0",  # (the probes run in every call: they are for the calls to come)
    ("block.auto.remembered_rings", "decompress.choice"): "const 0",
    ("block.auto.remembered_twopass", "lz4.decompress.mixed_groups"): "read 0 1 0",
    ("block.auto.remembered_twopass", "decompress.choice"): "const 3",
    ("block.auto.remembered_twopass", "decompress.twopass_fallback_blocks"): "read 4096 3 2",
    ("block.twopass", "decompress.twopass_fallback_blocks"): "read 0 3 2",
    ("lzo.twopass", "lzo.decompress.fallback_blocks"): "read 0 3 2",
    ("lzo.wave", "lzo.decompress.fallback_blocks"): "const 0",
    ("zstd.one_kernel", "zstd.decompress.fallback_items"): "const 16",
}
EXPECTED.update({("zstd.pipeline", name): "read %d 1 0" % (4 * word) for name, word in ZSTD_WORDS.items()})
EXPECTED.update({("zstd.one_kernel", "zstd.decompress.fallback_stage%d" % s): "const 0" for s in range(1, 7)})


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    compiler = shutil.which("g++")
    if compiler is None:
        pytest.skip("no g++ for the sanitized host build")
    tmp = tmp_path_factory.mktemp("stats_layout")
    src, exe = str(tmp / "stats.cpp"), str(tmp / "stats")
    with open(src, "w") as f:
        f.write(PROGRAM)
    # the two headers ALONE: no HIP include path, no -x hip
    subprocess.run([compiler, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, src], check=True)
    r = subprocess.run([exe] + list(SCRATCH_KEPT + NO_SUCH), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(": ")
        out[name] = rest.strip()
    return out


def test_the_header_needs_no_hip():
    text = open(os.path.join(CSRC, "achip_stats.h")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<c") for i in includes), includes  # (the C library's headers alone)


def test_every_statistic_under_every_last_launch(printed):
    """a statistic kept in the scratch has an answer under the launch that produces it and is -1 under "nothing" and under every other kind; where the
    answer is a read, it is the word the writer writes: 0, 33 .. 38, 18, 40, 41, 42 of the Zstd pipeline's counters, word 2 of the arena header behind a lead of
    0 (the two passes alone) or 4096 (behind the probes' page), words 0 .. 5 of the probes"""
    got = {(kind, name): printed["%s|%s" % (kind, name)] for kind in KINDS for name in SCRATCH_KEPT}
    want = {key: EXPECTED.get(key, NONE) for key in got}
    assert got == want, sorted((k, got[k], want[k]) for k in got if got[k] != want[k])
    assert all(got[("nothing", name)] == NONE for name in SCRATCH_KEPT)
    for name in SCRATCH_KEPT:  # each has a producer, and only kinds of one launcher produce it
        producers = {kind.split(".")[0] for kind in KINDS if got[(kind, name)] != NONE}
        assert len(producers) == 1, (name, producers)


def test_names_that_are_no_statistic(printed):
    for kind in KINDS:
        for name in NO_SUCH:
            assert printed["%s|%s" % (kind, name)] == NONE, (kind, name)


def test_choice_is_the_hosts_pick_at_the_recorded_familys_limit(printed):
    """(32-byte sequences, a mixed batch) -> 3 two passes / 0 rings"""
    assert printed["block.auto.lz4|picked"] == "3 3"
    assert printed["block.auto.snappy|picked"] == "0 3"
    assert printed["names"] == "0 3"
