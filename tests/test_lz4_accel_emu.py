"""The `_accel` kernels of aircompressor_amd/csrc/lz4_compress.hip -- serial probes, batch probes, the window encoder at both table widths, the two-tier arrangement,
the frame writer -- on the CPU under the fiber emulator, bytes against the pure-Python model: tools/hostemu/check_lz4_accel.py --quick.  The correctness check of
the masked replay that needs no GPU."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_accelerated_lz4_kernels_on_the_emulator():
    clang = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("no clang++ for the host build of the kernel source")
    emu_dir = os.path.join(ROOT, "tools", "hostemu")
    subprocess.run([clang, "-O2", "-std=c++17", "-fPIC", "-shared", "-fno-omit-frame-pointer", "-fsanitize-coverage=inline-8bit-counters,trace-loads,trace-stores",
                    "-I", emu_dir, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "aircompressor_amd", "csrc"),
                    "-o", os.path.join(emu_dir, "libemu_lz4_accel.so"), os.path.join(emu_dir, "emu_lz4_accel.cpp")], check=True)
    r = subprocess.run([sys.executable, os.path.join(emu_dir, "check_lz4_accel.py"), "--quick"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert re_items(r.stdout) > 500 and "items, 0 wrong" in r.stdout and "MISMATCH" not in r.stdout


def re_items(out):
    import re
    m = re.search(r"lz4 acceleration emulator: (\d+) items", out)
    return int(m.group(1)) if m else 0
