"""The LZO kernels of aircompressor_amd/csrc (lzo_parse2_kernel with the record executor, lzo_decompress_wave_kernel, the hand-over of an exhausted arena, the
sizing kernel, the encoder, the decode paths at four destination misalignments) on the CPU under the fiber emulator, the whole catalog against the pure-Python
model: tools/hostemu/check_lzo.py.  The correctness check that needs no GPU."""
import re

from tests import common


def test_lzo_kernels_on_the_emulator():
    r = common.emulator_checks(["lzo"], {"lzo": ("check_lzo.py",)})["lzo"]
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    m = re.search(r"lzo emulator: (\d+) items, (\d+) wrong", r.stdout)
    assert m and int(m.group(1)) > 1500 and int(m.group(2)) == 0 and "MISMATCH" not in r.stdout
    handed = re.search(r"an arena of 24 chunks \[(\d+) handed over\]", r.stdout)
    assert handed and int(handed.group(1)) > 0
