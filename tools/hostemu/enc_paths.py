"""Which way the sequences of the LZ4 and Snappy window encoders go (lz4_compress_mw.h / snappy_compress_mw.h, variant 4), and which way the Zstd encoder goes
(zstd_compress_body.h, zstd_dfast_mw.h; --option is its variant, 3 by default): a counting build of the emulator library (-DACHIP_HOST_STATS:
emulib.py's target enc_stats, rebuilt here when stale), the counters per input or summed, the bytes against the oracle's.

    enc_paths.py [lz4|snappy] [corpus|catalog]      corpus: the 64 KiB slices of tests/golden, a line each;  catalog: tests/encoder_edge_cases.py (the entries an
                                                    emulator run takes), a line per counter with the case that raised it first

    enc_paths.py zstd catalog [--option N]          tests/zstd_encoder_cases.py (emulator_cases()), the same table

    enc_paths.py lz4|snappy|zstd catalog --json [--option N]      the same as one JSON line [[case, identical, {counter: count}], ...]
                                                    (tests/test_encoder_edge_cases.py builds the library once and starts one of these per variant, side by side)"""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emulib
from emu_harness import EmuBatch

OPS = {"lz4": 1, "snappy": 3, "zstd": 5}
DEFAULT_OPTION = {"lz4": 4, "snappy": 4, "zstd": 3}
COUNTERS = {
    "lz4": {20: "sequences of the replay", 21: "vector path", 22: "more than 4 bytes match backwards", 23: "candidate inside the window", 24: "no usable facts",
            25: "mode-2 matches", 26: "windows", 27: "zero-literal hits", 28: "scalar count from registers (okA && okB)", 29: "scalar count from memory",
            30: "memory catch-up, second trip (window)", 31: "block ends at a probe beyond matchFindLimit", 32: "block ends behind a match",
            33: "match ends beyond its window", 34: "memory catch-up, second trip (mode 2)", 35: "mode 2 runs off the end"},
    "snappy": {40: "copies of the replay", 41: "candidate inside the window", 42: "re-probe hits", 43: "copies split into pieces of 64 / 60", 44: "last piece a copy-1",
               45: "last piece a copy-2", 46: "mode-2 copies", 47: "windows", 48: "search runs off the end in a window", 49: "search runs off the end in mode 2",
               50: "vector path", 51: "copy ends beyond its window", 52: "scalar count from registers (okA && okB)", 53: "scalar count from memory"},
    # 0 .. 16: the window match finder (variant 3); 17 .. 19: the position-by-position finder (variants 0, 1, 2); 60, 61, 64 .. 127: the entropy stage and the blocks
    "zstd": {0: "windows", 1: "searches", 2: "matches", 3: "repeat at +1", 4: "long", 5: "short", 6: "candidate inside the window", 7: "backward bytes",
             8: "backward from memory", 9: "match ends beyond the window", 10: "repeat loop hits", 11: "count_table to memory", 12: "count_window to memory",
             13: "count_repeat to memory", 14: "serial steps", 15: "searches without a hit", 16: "windows with equal hashes",
             17: "batch probe", 18: "probe of one position", 19: "batch probe finds nothing",
             60: "previous Huffman table not valid: its alphabet ends below the block's largest symbol", 61: "Huffman table log at the floor of 5",
             64: "literals: raw below 64", 65: "RLE literals, one-byte header", 66: "RLE literals, two-byte header", 67: "RLE literals, three-byte header",
             68: "literals: raw by the (n >> 7) + 4 shortcut", 69: "previous Huffman table valid", 70: "previous Huffman table not valid: a symbol has no code", 71: "table reused by preference",
             72: "table reused by estimate", 73: "new table beats a valid one", 74: "one stream", 75: "four streams", 76: "literals: raw after the streams were sized",
             77: "compressed literals, three-byte header", 78: "four-byte header", 79: "five-byte header", 80: "treeless literals written", 81: "setMaxHeight limits the tree",
             82: "repayment step from rank 1", 83: "repayment step where the scan stops", 84: "overpaid: no leaf of rank 1, back to the last cut leaf", 85: "overpaid: the next leaf of rank 1",
             86: "weights all equal", 87: "no weight twice", 88: "weights FSE-compressed", 89: "weights direct", 90: "Huffman table log 11", 91: "table log from the input size",
             92: "table log from the symbol count", 93: "LL predefined", 94: "LL RLE", 95: "LL FSE", 96: "OF predefined", 97: "OF RLE", 98: "OF FSE",
             99: "ML predefined", 100: "ML RLE", 101: "ML FSE", 102: "predefined: one code, at most two sequences", 103: "predefined: fewer than minNumberOfSequences",
             104: "predefined: largest count < count >> (log - 1)", 105: "predefined offsets disallowed (code >= 28)", 106: "last code's count decremented",
             107: "last code's count kept", 108: "FSE table log at its maximum", 109: "FSE table log from the sequence count", 110: "FSE table log from the symbol count",
             111: "FSE table log 5", 112: "normalizeCounts2", 113: "zero run of 0 .. 2 behind a zero", 114: "zero run of 3 .. 23", 115: "zero run of 24 and more",
             116: "sequence count in one byte", 117: "in two bytes", 118: "in three bytes", 119: "no sequences", 120: "last group of the lane-parallel encoder (< 64)",
             121: "full group of 64", 122: "literal length >= 65536 (code 35)", 123: "match length >= 65539 (code 52)", 124: "block dropped by the gain test",
             125: "block committed", 126: "window base moves", 127: "new table: the previous one is not valid"},
}


def build(clang=None):
    """the emulator's encoder unit with the counters compiled in, rebuilt whatever lies there (emulib.py's target enc_stats; the compiler is emulib's)"""
    emulib.build("enc_stats")
    return emulib.path("enc_stats")


class StatsBatch(EmuBatch):
    def __init__(self, lib, option):
        self.lib, self.options, self.option = lib, {}, option

    def _call(self, op, *batch):
        return self.lib.emu_encode(op, *batch, self.option, 262144)


def count(codec, inputs, oracle, option=None, lib=None):
    """every input on its own through the counting build: [(output == the oracle's, {counter: count})]"""
    lib = lib or emulib.load("enc_stats")
    stats = (ctypes.c_longlong * 128).in_dll(lib, "g_zc_stats")
    option = DEFAULT_OPTION[codec] if option is None else option
    out = []
    for data in inputs:
        for i in range(128):
            stats[i] = 0
        outs, status, _ = StatsBatch(lib, option).run(OPS[codec], [data], [oracle.max_compressed_length(codec, len(data))])
        out.append((status[0] == 0 and outs[0] == oracle.compress(codec, data), {k: int(stats[k]) for k in COUNTERS[codec]}))
    return out


def main():
    from tests import common, oracle_lib
    o = oracle_lib.load()
    codecs = [c for c in ("lz4", "snappy", "zstd") if c in sys.argv[1:]] or ["lz4", "snappy"]
    option = int(sys.argv[sys.argv.index("--option") + 1]) if "--option" in sys.argv else None

    def catalog(codec):  # (each codec's catalog is imported where it is asked for: a run for one codec needs only that codec's module)
        if codec == "zstd":
            from tests import zstd_encoder_cases
            return zstd_encoder_cases.emulator_cases(option)
        from tests import encoder_edge_cases
        return encoder_edge_cases.emulator_cases(codec)
    if "--json" in sys.argv:
        entries = catalog(codecs[0])
        print(json.dumps([[e[0], ok, c] for e, (ok, c) in zip(entries, count(codecs[0], [d for _, d, _ in entries], o, option))]))
        return
    for codec in codecs:
        names = COUNTERS[codec]
        if "catalog" in sys.argv[1:]:
            entries = catalog(codec)
            results = count(codec, [d for _, d, _ in entries], o, option)
            print("%s: %d catalog entries, %d differ from the oracle" % (codec, len(entries), sum(not ok for ok, _ in results)))
            for k, what in names.items():
                first = next((e[0] for e, (_, c) in zip(entries, results) if c[k]), None)
                print("  %2d %-46s %7d   first: %s" % (k, what, sum(c[k] for _, c in results), first))
        else:
            for name, data, _ in common.corpus_sample():
                (ok, c), = count(codec, [data[:65536]], o)
                print("%-28s ok=%s  %s" % (name, ok, "  ".join("%s %d" % (names[k], c[k]) for k in names)))


if __name__ == "__main__":
    main()
