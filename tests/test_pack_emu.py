"""The bound kernel, the pack scan and the dense copy (aircompressor_amd/csrc/pack_outputs.hip) on the CPU under the fiber emulator, against numpy and the
library's host bound functions: tools/hostemu/check_pack.py over the cases of tests/pack_cases.py.  The correctness check of these kernels that needs no GPU."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_kernels_on_the_emulator():
    import __graft_entry__ as g
    g.build_library()  # (the host bound functions the bound kernel is compared with)
    clang = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("no clang++ for the host build of the kernel source")
    emu_dir = os.path.join(ROOT, "tools", "hostemu")
    subprocess.run([clang, "-O1", "-std=c++17", "-fPIC", "-shared", "-I", emu_dir, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "aircompressor_amd", "csrc"),
                    "-o", os.path.join(emu_dir, "libemu_pack.so"), os.path.join(emu_dir, "emu_pack.cpp")], check=True)
    r = subprocess.run([sys.executable, os.path.join(emu_dir, "check_pack.py"), "--quick"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "pack calls, 0 wrong" in r.stdout and "MISMATCH" not in r.stdout
