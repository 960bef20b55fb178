"""The host arithmetic shared by the sweep steps (deal_columns, clamp_tile, halve_tile, split_columns, lds_budget and the overlap
rule first_overlap in lpopc_amd/csrc/rpm_engine.hpp) on the CPU: tests/native/sweep_plan_test.cpp walks every small input, plain
and under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]], ids=["plain", "asan_ubsan"])
def test_deal_columns_and_clamp_tile(tmp_path, sanitize):
    exe = str(tmp_path / "sweep_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + sanitize +
                          [os.path.join(ROOT, "tests", "native", "sweep_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), r.stdout + r.stderr
