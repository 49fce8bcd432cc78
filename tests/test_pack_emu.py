"""The bound kernel, the pack scan and the dense copy (aircompressor_amd/csrc/pack_outputs.hip) on the CPU under the fiber emulator, against numpy and the
library's host bound functions: tools/hostemu/check_pack.py over the cases of tests/pack_cases.py.  The correctness check of these kernels that needs no GPU."""
from tests import common


def test_pack_kernels_on_the_emulator():
    import __graft_entry__ as g
    g.build_library()  # (the host bound functions the bound kernel is compared with)
    r = common.emulator_checks(["pack"], {"pack": ("check_pack.py", "--quick")})["pack"]
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "pack calls, 0 wrong" in r.stdout and "MISMATCH" not in r.stdout
