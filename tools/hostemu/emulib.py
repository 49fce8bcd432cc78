"""The emulator libraries: the one table of what is built from what, and the one place where a compile command is put together and a library is opened.

    emulib.py [target ...]      builds the named targets (all of them when none is named); tools/hostemu/build.sh is this call

load(target) is what every check script opens its library with: it builds the library first when the file is missing or older than anything that can go into
it (its unit, the units and the shim beside it, the kernel sources and headers), so a script run by hand never checks yesterday's kernel.  HOSTEMU_LIB=<file in
tools/hostemu> names another build of the same unit instead (tools/hostemu/run_asan_fuzz.sh makes such builds): it is loaded as it lies there, never rebuilt.
The sanitizer builds have no entry here."""
import ctypes
import glob
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
INCLUDE = ["-I", HERE, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "aircompressor_amd", "csrc")]
# access lockstep (hip/hip_runtime.h, HOSTEMU_ACCESS_LOCKSTEP): clang's callbacks before every load and store of the kernel source, frame pointers for "earliest first"
LOCKSTEP = ["-fno-omit-frame-pointer", "-fsanitize-coverage=inline-8bit-counters,trace-loads,trace-stores"]
JOBS = 4  # compilers side by side

# target: (translation unit, library, -O level, access-lockstep unit, -D ...)
TARGETS = {
    "zstd":            ("emu_zstd.cpp",         "libemu_zstd.so",         1, False, ()),
    "enc":             ("emu_enc.cpp",          "libemu_enc.so",          2, True,  ()),
    "all":             ("emu_all.cpp",          "libemu_all.so",          1, False, ()),
    "serial":          ("emu_serial.cpp",       "libemu_serial.so",       1, False, ()),
    "emu":             ("emu.cpp",              "libemu.so",              1, False, ()),
    "xxh3":            ("emu_xxh3.cpp",         "libemu_xxh3.so",         1, False, ()),
    "size":            ("emu_size.cpp",         "libemu_size.so",         1, False, ()),
    "pack":            ("emu_pack.cpp",         "libemu_pack.so",         1, False, ()),
    "xxh_stream":      ("emu_xxh_stream.cpp",   "libemu_xxh_stream.so",   1, False, ()),
    "window":          ("emu_window.cpp",       "libemu_window.so",       1, False, ()),
    "lz4_accel":       ("emu_lz4_accel.cpp",    "libemu_lz4_accel.so",    2, True,  ()),
    "snf_params_w":    ("emu_snf_params.cpp",   "libemu_snf_params_w.so", 2, True,  ("SNF_PARAMS_WRITERS",)),
    "snf_params_r":    ("emu_snf_params.cpp",   "libemu_snf_params_r.so", 1, False, ()),
    "lz4f_writer":     ("emu_lz4f_writer.cpp",  "libemu_lz4f_writer.so",  2, True,  ()),
    "lzo_w":           ("emu_lzo.cpp",          "libemu_lzo_w.so",        2, True,  ("LZO_ENCODER",)),  # the encoder; lzo_r: the decoders and the sizing kernel
    "lzo_r":           ("emu_lzo.cpp",          "libemu_lzo_r.so",        1, False, ()),
    "enc_stats":       ("emu_enc.cpp",          "libemu_enc_stats.so",    2, True,  ("ACHIP_HOST_STATS",)),  # the counting build: enc_paths.py, zc_stats.py
    "lockstep":        ("emu_lockstep.cpp",     "libemu_lockstep.so",     2, True,  ()),  # HOSTEMU_LIB=libemu_lockstep.so check_v3.py
    "entropy_unit":    ("emu_entropy_unit.cpp", "libemu_entropy_unit.so", 2, True,  ()),
    "unit_oracle_enc": ("unit_oracle_enc.c",    "libunit_oracle_enc.so",  2, False, ()),  # a C unit over oracle/*.c: check_entropy_unit.py's reference
}
GROUPS = {"snf_params": ("snf_params_w", "snf_params_r"), "lzo": ("lzo_w", "lzo_r")}  # (a name of build.sh that stands for two libraries)
DEFAULT = ("zstd", "enc", "all", "serial", "emu", "xxh3", "size", "pack", "xxh_stream", "window", "lz4_accel", "snf_params", "lz4f_writer", "lzo")  # what build.sh builds when nothing is named


def compiler():
    """the clang++ for the host build of the kernel source, or None"""
    clang = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    return clang if os.path.exists(clang) else None


def path(target):
    return os.path.join(HERE, TARGETS[target][1])


def command(target, out=None):
    unit, lib, level, lockstep, defines = TARGETS[target]
    tail = ["-o", out or path(target), os.path.join(HERE, unit)]
    if unit.endswith(".c"):
        oracle = sorted(f for f in glob.glob(os.path.join(ROOT, "oracle", "*.c")) if os.path.basename(f) != "zstd_enc.c")  # (the unit includes zstd_enc.c itself)
        return ["gcc", "-O%d" % level, "-fPIC", "-std=gnu11", "-fno-strict-aliasing", "-pthread", "-w", "-shared"] + tail + oracle
    return [compiler() or "clang++", "-O%d" % level, "-std=c++17", "-fPIC", "-shared"] + (LOCKSTEP if lockstep else []) + ["-D" + d for d in defines] + INCLUDE + tail


def program_command(source, exe):
    """a stand-alone host program over the shim and the kernel headers (tests/test_host_logic.py: the decoder choice rule)"""
    return [compiler() or "clang++", "-O1", "-std=c++17"] + INCLUDE + ["-o", exe, source]


def expand(names):
    return [t for name in names for t in GROUPS.get(name, (name,))]


def build(*names):
    """compiles the named targets, at most JOBS side by side; a library appears under its name only when it is whole (a script may be loading the old one)"""
    targets = expand(names)
    for k in range(0, len(targets), JOBS):
        running = []
        for t in targets[k:k + JOBS]:
            tmp = "%s.%d.tmp.so" % (path(t)[:-3], os.getpid())  # (*.so: ignored like the library itself if a build is cut short)
            running.append((t, tmp, subprocess.Popen(command(t, tmp), cwd=ROOT)))
        failed = [t for t, tmp, job in running if job.wait() != 0]
        for t, tmp, _ in running:
            if t in failed:
                if os.path.exists(tmp):
                    os.remove(tmp)
            else:
                os.replace(tmp, path(t))
        if failed:
            raise RuntimeError("the emulator libraries %s did not build" % ", ".join(failed))


def sources(target):
    """every file that can go into a target's library"""
    unit = TARGETS[target][0]
    patterns = [(HERE, "*.cpp"), (HERE, "*.h"), (HERE, "emulib.py"), (HERE, "hip", "*"), (ROOT, "aircompressor_amd", "csrc", "*"), (ROOT, "include", "*")]
    if unit.endswith(".c"):
        patterns += [(HERE, unit), (ROOT, "oracle", "*.c"), (ROOT, "oracle", "*.h")]
    return [f for p in patterns for f in glob.glob(os.path.join(*p)) if os.path.isfile(f)]


def stale(target):
    lib = path(target)
    return not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in sources(target))


def load(target, env=True):
    """-> ctypes.CDLL of a target's library, built first if stale; with HOSTEMU_LIB set (and env: a script that opens two libraries honours it for its first)
    that file instead, as it is"""
    named = os.environ.get("HOSTEMU_LIB") if env else None
    if named:
        return ctypes.CDLL(os.path.join(HERE, named))
    if stale(target):
        print("emulib: building %s" % TARGETS[target][1], file=sys.stderr, flush=True)
        build(target)
    return ctypes.CDLL(path(target))


if __name__ == "__main__":
    unknown = [t for t in sys.argv[1:] if t not in TARGETS and t not in GROUPS]
    if unknown:
        sys.exit("emulib: no target %s (targets: %s)" % (", ".join(unknown), " ".join(list(GROUPS) + list(TARGETS))))
    build(*(sys.argv[1:] or DEFAULT))
    print("built %s" % " ".join(sys.argv[1:] or DEFAULT))
