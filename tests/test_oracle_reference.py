"""Oracle checks on the reference's test corpus (tests/golden/corpus_full.bin.xz) and its decoders' literal tables
(tests/golden/java_tables.json, cut from the Java sources by tools/make_golden.py): corpus round trips, cross-decoding with
third-party codecs (tests/native_libs.py: the ones the reference bundles, else the system's), the decoder's tables, and the
stability of tests/golden/manifest.json."""
import hashlib
import json
import os

import pytest

from tests import common, native_libs, oracle_lib


def corpus_files():
    """[(path under the reference's testdata/, bytes)] -- all 42 files"""
    return sorted(common.corpus_full().items())


def java_tables():
    return json.load(open(os.path.join(common.GOLDEN, "java_tables.json")))


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


def test_manifest_is_current(o):
    manifest = json.load(open(os.path.join(common.GOLDEN, "manifest.json")))
    files = corpus_files()
    assert sorted(manifest) == [rel for rel, _ in files]
    for rel, d in files:
        assert manifest[rel]["sha256"] == hashlib.sha256(d).hexdigest()
        for codec in ("lz4", "snappy", "zstd"):
            c = o.compress(codec, d)
            assert manifest[rel][codec]["sha256"] == hashlib.sha256(c).hexdigest(), (rel, codec)
            assert o.decompress(codec, c, len(d)) == d


@pytest.mark.skipif(not native_libs.available(), reason="needs liblz4, libsnappy and libzstd (the reference's bundled copies or the system's)")
def test_cross_decode_with_bundled_native_codecs(o):
    nl = native_libs
    for f, d in corpus_files():
        assert nl.lz4_decompress(o.compress("lz4", d), len(d)) == d, f       # our stream, their decoder
        assert o.decompress("lz4", nl.lz4_compress(d), len(d)) == d, f        # their stream, our decoder
        assert nl.snappy_decompress(o.compress("snappy", d), len(d)) == d, f
        assert o.decompress("snappy", nl.snappy_compress(d), len(d)) == d, f
        assert nl.zstd_decompress(o.compress("zstd", d), len(d)) == d, f           # oracle's level-3 frames, libzstd 1.5.6 decoder
        for i in range(0, min(len(d), 3 * 131072), 131072):
            b = d[i:i + 131072]
            assert nl.zstd_decompress(o.compress("zstd", b), len(b)) == b


@pytest.mark.skipif(not native_libs.available("zstd"), reason="needs libzstd (the reference's bundled copy or the system's)")
def test_zstd_decoder_on_libzstd_frames(o):
    # T/zstd/TestZstd.java:21-47 exercises the Java decoder on zstd-jni level-3 frames; libzstd stands in
    nl = native_libs
    for f, d in corpus_files():
        for level in (1, 3, 7):
            assert o.decompress("zstd", nl.zstd_compress(d, level), len(d)) == d, (f, level)
        for i in range(0, min(len(d), 4 * 131072), 131072):
            b = d[i:i + 131072]
            assert o.decompress("zstd", nl.zstd_compress(b, 3), len(b)) == b


def test_snappy_op_table_matches_java_source(o):
    table = java_tables()["snappy_op_lookup_table"]
    assert len(table) == 256

    def entry(op):  # the layout restated in oracle/snappy.c and the HIP kernel
        kind, hi = op & 3, op >> 2
        if kind == 0:
            return hi + 1 if hi < 60 else (((hi - 59) << 11) | 1)
        if kind == 1:
            return (1 << 11) | ((hi >> 3) << 8) | ((hi & 7) + 4)
        return ((2 if kind == 2 else 4) << 11) | (hi + 1)

    assert [entry(i) for i in range(256)] == table


def test_zstd_default_tables_match_java_source(o):
    """oracle/zstd_dec.c builds the predefined LL/OF/ML decoding tables from the RFC 8878 distributions with
    the reference's own table builder; the result must equal the literal tables in ZstdFrameDecompressor.java:85-113.
    Decoding a frame whose sequences use predefined (BASIC) tables exercises them: offset-before-start.zst uses
    all-BASIC tables and must fail exactly at the corrupted offset, and libzstd frames of tiny inputs use BASIC mode."""
    if not native_libs.available("zstd"):
        pytest.skip("needs libzstd (the reference's bundled copy or the system's)")
    for n in (20, 60, 200, 1000):
        d = (b"abcdefgh" * 200)[:n] + bytes(range(n % 50))
        assert o.decompress("zstd", native_libs.zstd_compress(d, 3), len(d)) == d
    # and literally: the three Java tables against tables dumped through a BASIC-mode decode
    blocks = java_tables()["zstd_default_fse_tables"]
    assert len(blocks) == 3
    import ctypes
    import subprocess
    import tempfile
    src = r'''
    #include <stdio.h>
    #include "%s/oracle/zstd_dec.c"
    int main(void) { zctx* c = calloc(1, sizeof(zctx)); build_defaults(c);
      const fse_table* t[3] = {&c->default_ll, &c->default_of, &c->default_ml};
      for (int k = 0; k < 3; k++) { int n = 1 << t[k]->log2_size; printf("%%d\n", t[k]->log2_size);
        for (int i = 0; i < n; i++) printf("%%d ", t[k]->new_state[i]); printf("\n");
        for (int i = 0; i < n; i++) printf("%%d ", t[k]->symbol[i]); printf("\n");
        for (int i = 0; i < n; i++) printf("%%d ", t[k]->number_of_bits[i]); printf("\n"); }
      return 0; }''' % common.HERE.rsplit("/tests", 1)[0]
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "dump.c"), "w").write(src)
        subprocess.run(["gcc", "-O1", "-w", "-o", os.path.join(td, "dump"), os.path.join(td, "dump.c"),
                        os.path.join(common.HERE, "..", "oracle", "xxhash64.c")], check=True)
        lines = subprocess.run([os.path.join(td, "dump")], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    nums = lambda s: [int(x) for x in s.split()]  # noqa: E731
    for k, t in enumerate(blocks):
        assert int(lines[4 * k]) == t["log2_size"]
        assert nums(lines[4 * k + 1]) == t["new_state"]
        assert nums(lines[4 * k + 2]) == t["symbol"]
        assert nums(lines[4 * k + 3]) == t["number_of_bits"]


def test_random_generator_feeds_codecs(o):
    for ratio in (0.1, 0.25, 0.5, 0.75, 1.0):
        g = o.random_generator(ratio).tobytes()
        for k in (0, 5):
            block = g[(k * 65536) % 1048576:][:65536]
            for codec in ("lz4", "snappy"):
                assert o.decompress(codec, o.compress(codec, block), 65536) == block
