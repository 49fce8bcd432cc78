"""The x-snappy-framed writers and readers of aircompressor_amd/csrc/snappy_frame.hip with the parameters of achip_ctx_set_snappyframed_writer and
achip_ctx_set_snappyframed_verify_checksums -- the wavefront-per-stream writer, the block list, the serial kernel behind a list that overflows, the window writer
at every cut (also with a list so small that windows stop at their share of it), reader variants 0 .. 3 and the window reader (variants 1 .. 3) with verify on and
off -- on the CPU under the fiber emulator, bytes, statuses and offsets against the pure-Python model: tools/hostemu/check_snf_params.py --quick.
What --quick leaves to the GPU test (tests/test_gpu_snf_params.py runs the whole catalog): the block encoder costs an order point per memory access here, so block
sizes 1, 2, 63 and 64 run whole at ratios 0.85 and 0.5 (1.0 and the smallest double once each), 4096 with inputs of up to a block and a byte and the several-block
run at two parameter sets, and 65535 / 65536 not at all; without --quick the script runs the whole catalog (hours)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_snappyframed_parameters_on_the_emulator():
    clang = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("no clang++ for the host build of the kernel source")
    emu_dir = os.path.join(ROOT, "tools", "hostemu")
    include = ["-I", emu_dir, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "aircompressor_amd", "csrc")]
    source = os.path.join(emu_dir, "emu_snf_params.cpp")
    builds = [subprocess.Popen([clang, "-O2", "-std=c++17", "-fPIC", "-shared", "-fno-omit-frame-pointer", "-fsanitize-coverage=inline-8bit-counters,trace-loads,trace-stores",
                                "-DSNF_PARAMS_WRITERS"] + include + ["-o", os.path.join(emu_dir, "libemu_snf_params_w.so"), source]),
              subprocess.Popen([clang, "-O1", "-std=c++17", "-fPIC", "-shared"] + include + ["-o", os.path.join(emu_dir, "libemu_snf_params_r.so"), source])]
    assert [b.wait() for b in builds] == [0, 0]
    r = subprocess.run([sys.executable, os.path.join(emu_dir, "check_snf_params.py"), "--quick"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    m = re.search(r"snf parameters emulator: (\d+) items, 0 wrong", r.stdout)
    assert m and int(m.group(1)) > 1000 and "MISMATCH" not in r.stdout
