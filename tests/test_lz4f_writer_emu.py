"""The block-list LZ4 frame writer of aircompressor_amd/csrc/lz4_frame_writer.hip -- plan, seal, encode, compact -- on the CPU under the fiber emulator, bytes,
lengths and statuses against the pure-Python model: tools/hostemu/check_lz4f_writer.py --quick.
What --quick leaves to the GPU test (tests/test_gpu_lz4f_writer.py runs the whole catalog): the block encoder costs an order point per memory access here, so the
64 KiB settings run with every flag off and every flag on over the inputs of up to two blocks, one large setting runs its B + 1 (the wide table, a second block of
one byte), and the defaults, the refusals, the list of three entries and acceleration 7 run whole; without --quick the script runs the whole catalog."""
import re

from tests import common


def test_lz4_frame_writer_on_the_emulator():
    r = common.emulator_checks(["lz4f_writer"], {"lz4f_writer": ("check_lz4f_writer.py", "--quick")})["lz4f_writer"]
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    m = re.search(r"lz4 frame writer emulator: (\d+) items, 0 wrong", r.stdout)
    assert m and int(m.group(1)) >= 60 and "MISMATCH" not in r.stdout
