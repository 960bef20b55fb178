"""The device solver's call-order state (IpmHold, lpopc_amd/csrc/rpm_ipm_hold.hpp) on the CPU: tests/native/ipm_hold_test.cpp walks
every sequence of six calls on it and on a restatement of the four flags it replaced, plain and under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]], ids=["plain", "asan_ubsan"])
def test_every_call_sequence_against_the_flags(tmp_path, sanitize):
    exe = str(tmp_path / "ipm_hold_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + sanitize +
                          [os.path.join(ROOT, "tests", "native", "ipm_hold_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), r.stdout + r.stderr
