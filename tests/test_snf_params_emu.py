"""The x-snappy-framed writers and readers of aircompressor_amd/csrc/snappy_frame.hip with the parameters of achip_ctx_set_snappyframed_writer and
achip_ctx_set_snappyframed_verify_checksums -- the wavefront-per-stream writer, the block list, the serial kernel behind a list that overflows, the window writer
at every cut (also with a list so small that windows stop at their share of it), reader variants 0 .. 3 and the window reader (variants 1 .. 3) with verify on and
off -- on the CPU under the fiber emulator, bytes, statuses and offsets against the pure-Python model: tools/hostemu/check_snf_params.py --quick.
What --quick leaves to the GPU test (tests/test_gpu_snf_params.py runs the whole catalog): the block encoder costs an order point per memory access here, so block
sizes 1, 2, 63 and 64 run whole at ratios 0.85 and 0.5 (1.0 and the smallest double once each), 4096 with inputs of up to a block and a byte and the several-block
run at two parameter sets, and 65535 / 65536 not at all; without --quick the script runs the whole catalog (hours)."""
import re

from tests import common


def test_snappyframed_parameters_on_the_emulator():
    r = common.emulator_checks(["snf_params"], {"snf_params": ("check_snf_params.py", "--quick")})["snf_params"]  # (the writers' and the readers' library, built side by side)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    m = re.search(r"snf parameters emulator: (\d+) items, 0 wrong", r.stdout)
    assert m and int(m.group(1)) > 1000 and "MISMATCH" not in r.stdout
