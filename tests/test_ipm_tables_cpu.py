"""The index tables rpm_ipm_create uploads beside the plan (lpopc_amd/csrc/rpm_ipm_tables.cpp: fill list, fused-fill tables,
sub-problem list, long columns) on the CPU: tests/native/ipm_tables_test.cpp builds them for nested plans of small meshes and walks
every entry, plain and under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lpopc_amd", "csrc")
# the host-only sources the tables need: no HIP header, no device
SOURCES = [os.path.join(ROOT, "tests", "native", "ipm_tables_test.cpp")] + \
          [os.path.join(CSRC, f) for f in ("rpm_setup.cpp", "rpm_mesh.cpp", "rpm_ipm.cpp", "rpm_ipm_tables.cpp")]


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]], ids=["plain", "asan_ubsan"])
def test_fill_list_and_fused_fill_tables(tmp_path, sanitize):
    # (unoptimised, one compiler process per source: compiling is all the time this test takes)
    flags = ["-std=c++17", "-O0", "-Wall"] + sanitize
    objects = [str(tmp_path / (os.path.basename(src) + ".o")) for src in SOURCES]
    compilers = [subprocess.Popen(["g++"] + flags + ["-c", src, "-o", obj]) for src, obj in zip(SOURCES, objects)]
    assert [c.wait() for c in compilers] == [0] * len(SOURCES)
    exe = str(tmp_path / "ipm_tables_test")
    subprocess.check_call(["g++"] + sanitize + objects + ["-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), r.stdout + r.stderr
    print(r.stdout.strip())
