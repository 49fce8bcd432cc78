"""The window kernels of the chunked containers (achip_window_*) under the fiber emulator, without a GPU: tools/hostemu/emu_window.cpp built for the host and
tools/hostemu/check_window.py --quick over the cases of tests/window_cases.py -- every cut, the standard loop driven to the end, the writers' plans -- against the
model built from the oracle's one-shot readers and writers."""
import re

from tests import common


def test_window_kernels_under_the_emulator():
    common.emulib()  # (skips here, before anything is built, where there is no compiler)
    import __graft_entry__ as g
    g.build_library()  # (check_window.py compares nothing with it; tests.oracle_lib builds the oracle on its own)

    def job(*args):
        return ("check_window.py", "--quick") + args
    # side by side (separate processes; the library is read-only): the cuts by format, the two loops
    jobs = {fmt: job("--part", "cuts", "--format", fmt) for fmt in ("snappyframed", "lz4hadoop", "snappyhadoop")}
    jobs["drive"] = job("--part", "drive")
    jobs["writers"] = job("--part", "writers")
    for name, r in common.emulator_checks(["window"], jobs).items():
        out = r.stdout
        assert r.returncode == 0, (name, out)
        lines = re.findall(r"window emulator, [a-z ]+: (\d+) checks, (\d+) wrong", out)
        assert len(lines) == 1 and int(lines[0][0]) > 50 and int(lines[0][1]) == 0, (name, out)
