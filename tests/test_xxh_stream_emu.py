"""The streaming hashers' kernels (aircompressor_amd/csrc/xxhash_stream.hip: reset, the quad / lane / wavefront updates, the digests) on the
CPU under the fiber emulator, against the one-shot references: tools/hostemu/check_xxh_stream.py over the plans of tests/xxh_stream_cases.py.
The correctness check of these kernels that needs no GPU."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_hash_kernels_on_the_emulator():
    from tests import oracle_lib
    oracle_lib.load()  # (the XXH64 / XXH32 reference)
    clang = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("no clang++ for the host build of the kernel source")
    emu_dir = os.path.join(ROOT, "tools", "hostemu")
    subprocess.run([clang, "-O1", "-std=c++17", "-fPIC", "-shared", "-I", emu_dir, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "aircompressor_amd", "csrc"),
                    "-o", os.path.join(emu_dir, "libemu_xxh_stream.so"), os.path.join(emu_dir, "emu_xxh_stream.cpp")], check=True)
    r = subprocess.run([sys.executable, os.path.join(emu_dir, "check_xxh_stream.py"), "--quick"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert re_states(r.stdout) and ", 0 wrong" in r.stdout and "MISMATCH" not in r.stdout


def re_states(text):
    import re
    m = re.search(r"xxh stream emulator: (\d+) states, 0 wrong", text)
    return m is not None and int(m.group(1)) > 10000
