"""csrc/narrow.h, the 24-bit copy of a level-0 inverse that the fine apply
kernel streams, on the host: tests/cpp/narrow_format_check.cpp includes the
header (its encode, decode and offset functions are __host__ __device__
inline) and is built with -fsanitize=address,undefined as a stand-alone
program.  It checks the round trip (|q s - x| <= 2^-24 max|x| (1 + 2^-23) per
entry for records with +-max and 0, subnormals, one dominant entry, all-equal
and all-zero entries; the fp32 decode is q s correctly rounded), that inf and
NaN records decode to non-finite values, and that the byte offsets of all
4 656 slots are distinct, in range and 16-byte aligned per dword group."""
import os
import subprocess

from conftest import PKG, REPO


def test_narrow_format_host_program(tmp_path):
    src = os.path.join(REPO, "tests", "cpp", "narrow_format_check.cpp")
    exe = str(tmp_path / "narrowchk")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    print(out)
    assert "narrow format ok" in out

