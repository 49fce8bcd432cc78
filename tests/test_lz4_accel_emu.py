"""The `_accel` kernels of aircompressor_amd/csrc/lz4_compress.hip -- serial probes, batch probes, the window encoder at both table widths, the two-tier arrangement,
the frame writer -- on the CPU under the fiber emulator, bytes against the pure-Python model: tools/hostemu/check_lz4_accel.py --quick.  The correctness check of
the masked replay that needs no GPU."""
from tests import common


def test_accelerated_lz4_kernels_on_the_emulator():
    r = common.emulator_checks(["lz4_accel"], {"lz4_accel": ("check_lz4_accel.py", "--quick")})["lz4_accel"]
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert re_items(r.stdout) > 500 and "items, 0 wrong" in r.stdout and "MISMATCH" not in r.stdout


def re_items(out):
    import re
    m = re.search(r"lz4 acceleration emulator: (\d+) items", out)
    return int(m.group(1)) if m else 0
