"""Solution sensitivities (rpm_ipm_sensitivities) without a device: the source table of their right-hand sides
(ipm_sens_table, lpopc_amd/csrc/rpm_ipm_tables.cpp) — tests/native/ipm_sens_table_test.cpp builds it for the plans of quadrotor 2 x 4
(band and nested), bryson_denham 2 x 8 and launch 2 x 5, walks every entry against a brute-force restatement and exercises every
refusal, plain and under AddressSanitizer + UBSan — and the new symbols: declared, listed, exported, with their ctypes signatures."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lpopc_amd.engine import ABI_SYMBOLS, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lpopc_amd", "csrc")
# the host-only sources the table needs: no HIP header, no device
SOURCES = [os.path.join(ROOT, "tests", "native", "ipm_sens_table_test.cpp")] + \
          [os.path.join(CSRC, f) for f in ("rpm_setup.cpp", "rpm_mesh.cpp", "rpm_ipm.cpp", "rpm_ipm_tables.cpp")]
NEW_SYMBOLS = ["rpm_ipm_initial_state_variables", "rpm_ipm_sensitivities_dev", "rpm_ipm_sensitivities", "rpm_ipm_apply_sensitivities_dev",
               "rpm_ipm_apply_sensitivities", "rpm_ipm_debug_sensitivity_rhs", "rpm_sweep_sensitivities"]


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]], ids=["plain", "asan_ubsan"])
def test_sensitivity_source_table(tmp_path, sanitize):
    # (unoptimised, one compiler process per source: compiling is all the time this test takes)
    flags = ["-std=c++17", "-O0", "-Wall"] + sanitize
    objects = [str(tmp_path / (os.path.basename(src) + ".o")) for src in SOURCES]
    compilers = [subprocess.Popen(["g++"] + flags + ["-c", src, "-o", obj]) for src, obj in zip(SOURCES, objects)]
    assert [c.wait() for c in compilers] == [0] * len(SOURCES)
    exe = str(tmp_path / "ipm_sens_table_test")
    subprocess.check_call(["g++"] + sanitize + objects + ["-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "\nok:" in "\n" + r.stdout, r.stdout + r.stderr
    print(r.stdout.strip())


def test_symbols_declared_listed_and_exported(built):
    L = lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
    flat = " ".join(open(os.path.join(ROOT, "include", "rpm_hip.h")).read().split())
    for sig in ("int rpm_ipm_initial_state_variables(rpm_ipm* s, int phase, int* var_index /* nx */);",
                "int rpm_ipm_sensitivities_dev(rpm_ipm* s, int n_par, const int* var_index, double* d_dx, double* d_dlambda, double* delta_w, "
                "int* info, void* stream);",
                "int rpm_ipm_sensitivities(rpm_ipm* s, int n_par, const int* var_index, double* dx, double* dlambda, double* delta_w, int* info);",
                "int rpm_ipm_apply_sensitivities_dev(rpm_ipm* s, int n_par, const int* var_index, const double* d_dx, const double* d_dlambda, "
                "const double* d_delta, const double* d_x, double* d_x_out, const double* d_lambda, double* d_lambda_out, void* stream);",
                "int rpm_ipm_apply_sensitivities(rpm_ipm* s, int n_par, const int* var_index, const double* dx, const double* dlambda, "
                "const double* delta, const double* x, double* x_out, const double* lambda, double* lambda_out);",
                "int rpm_ipm_debug_sensitivity_rhs(rpm_ipm* s, int n_par, const int* var_index, double* rhs);",
                "int rpm_sweep_sensitivities(rpm_sweep* s, int n_par, const int* var_index, double* dx, double* dlambda, double* delta_w, "
                "int* info);"):
        assert sig in flat, sig
    dp, ip, vp, i = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p, C.c_int
    assert L.rpm_ipm_initial_state_variables.argtypes == [vp, i, ip]
    assert L.rpm_ipm_sensitivities_dev.argtypes == [vp, i, ip, vp, vp, dp, ip, vp]
    assert L.rpm_ipm_sensitivities.argtypes == [vp, i, ip, dp, dp, dp, ip]
    assert L.rpm_ipm_apply_sensitivities_dev.argtypes == [vp, i, ip] + [vp] * 8
    assert L.rpm_ipm_apply_sensitivities.argtypes == [vp, i, ip] + [dp] * 7
    assert L.rpm_ipm_debug_sensitivity_rhs.argtypes == [vp, i, ip, dp]
    assert L.rpm_sweep_sensitivities.argtypes == [vp, i, ip, dp, dp, dp, ip]
    # a NULL handle: RPM_E_INVALID, decided before anything else
    a, k = np.zeros(8), np.zeros(2, dtype=np.int32)
    pa, pk = a.ctypes.data_as(dp), k.ctypes.data_as(ip)
    assert L.rpm_ipm_initial_state_variables(None, 0, pk) == 1
    assert L.rpm_ipm_sensitivities_dev(None, 1, pk, None, None, None, None, None) == 1
    assert L.rpm_ipm_sensitivities(None, 1, pk, pa, pa, None, None) == 1
    assert L.rpm_ipm_apply_sensitivities_dev(None, 1, pk, None, None, None, None, None, None, None, None) == 1
    assert L.rpm_ipm_apply_sensitivities(None, 1, pk, pa, None, pa, pa, pa, None, None) == 1
    assert L.rpm_ipm_debug_sensitivity_rhs(None, 1, pk, pa) == 1
    assert L.rpm_sweep_sensitivities(None, 1, pk, pa, None, None, None) == 1
