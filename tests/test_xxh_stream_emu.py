"""The streaming hashers' kernels (aircompressor_amd/csrc/xxhash_stream.hip: reset, the quad / lane / wavefront updates, the digests) on the
CPU under the fiber emulator, against the one-shot references: tools/hostemu/check_xxh_stream.py over the plans of tests/xxh_stream_cases.py.
The correctness check of these kernels that needs no GPU."""
from tests import common


def test_stream_hash_kernels_on_the_emulator():
    from tests import oracle_lib
    oracle_lib.load()  # (the XXH64 / XXH32 reference)
    r = common.emulator_checks(["xxh_stream"], {"xxh_stream": ("check_xxh_stream.py", "--quick")})["xxh_stream"]
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert re_states(r.stdout) and ", 0 wrong" in r.stdout and "MISMATCH" not in r.stdout


def re_states(text):
    import re
    m = re.search(r"xxh stream emulator: (\d+) states, 0 wrong", text)
    return m is not None and int(m.group(1)) > 10000
