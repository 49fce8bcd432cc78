"""The window kernels of the chunked containers (achip_window_*) under the fiber emulator, without a GPU: tools/hostemu/emu_window.cpp built for the host and
tools/hostemu/check_window.py --quick over the cases of tests/window_cases.py -- every cut, the standard loop driven to the end, the writers' plans -- against the
model built from the oracle's one-shot readers and writers."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_kernels_under_the_emulator():
    clang = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("no clang++ for the host build of the kernel source")
    import __graft_entry__ as g
    g.build_library()  # (check_window.py compares nothing with it; tests.oracle_lib builds the oracle on its own)
    emu_dir = os.path.join(ROOT, "tools", "hostemu")
    subprocess.run([clang, "-O1", "-std=c++17", "-fPIC", "-shared", "-I", emu_dir, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "aircompressor_amd", "csrc"),
                    "-o", os.path.join(emu_dir, "libemu_window.so"), os.path.join(emu_dir, "emu_window.cpp")], check=True)

    def start(*args):
        return subprocess.Popen([sys.executable, os.path.join(emu_dir, "check_window.py"), "--quick", *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    # side by side (separate processes; the library is read-only): the cuts by format, the two loops
    jobs = {fmt: start("--part", "cuts", "--format", fmt) for fmt in ("snappyframed", "lz4hadoop", "snappyhadoop")}
    jobs["drive"] = start("--part", "drive")
    jobs["writers"] = start("--part", "writers")
    for name, job in jobs.items():
        out = job.communicate()[0]
        assert job.returncode == 0, (name, out)
        lines = re.findall(r"window emulator, [a-z ]+: (\d+) checks, (\d+) wrong", out)
        assert len(lines) == 1 and int(lines[0][0]) > 50 and int(lines[0][1]) == 0, (name, out)
