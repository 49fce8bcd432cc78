"""LZ4 frames with linked blocks under the fiber emulator, without a GPU: lz4frame_decompress_kernel (tools/hostemu/emu_serial.cpp) and the LZ4FRAME sizing kernels
(tools/hostemu/emu_size.cpp) built for the host, and tools/hostemu/check_lz4_linked.py over the catalog of tests/lz4_linked_cases.py -- with the setting on and
off, at four destination misalignments -- against the model of tests/lz4_linked_ref.py."""
import re

from tests import common


def test_linked_frames_under_the_emulator():
    common.emulib()  # (skips here, before anything is built, where there is no compiler)
    jobs = {part: ("check_lz4_linked.py", "--part", part) for part in ("decode", "size")}  # side by side: separate processes, the libraries are read-only
    for part, r in common.emulator_checks(["serial", "size"], jobs).items():
        assert r.returncode == 0, (part, r.stdout)
        lines = re.findall(r"lz4 linked emulator, %s: (\d+) checks, (\d+) wrong" % part, r.stdout)
        assert len(lines) == 1 and int(lines[0][0]) >= 8 * 40 and int(lines[0][1]) == 0, (part, r.stdout)
