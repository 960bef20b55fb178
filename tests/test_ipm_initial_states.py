"""Measured initial states of a receding-horizon sweep (rpm_ipm_set_initial_states*, rpm_sweep_set_initial_states) and the
closed loop they were built for.

The reference of rpm_ipm_set_initial_states is rpm_ipm_set_all_bounds with the same numbers: the solver re-reads its bounds at
every solve, so the two must give the same solve bit for bit (x, lambda, z, objective, status, iterations), cold and warm, from a
host array and from a device array.  The closed loop (quadrotor 2 x 4, 3 instances, three steps of dt = 0.1 on the horizon of
2, options WARM of test_ipm_warm_start.py) runs the device-resident step — set_initial_states_dev, warm solve,
bound_multipliers_dev, shift of x, lambda, z_L, z_U — beside the same step through the host forms (set_all_bounds, host
shift_plan_batch) and asks for equal bits after every step; every instance must end with status 0 and within
1e-7 * max(1, |cold objective|) of a cold solve from the same measured states, the bound of test_ipm_warm_start.py.  The
measured state of a step is the shifted plan's own initial state plus a seeded disturbance of at most 0.01 per component.
Iteration counts are printed, not asserted: a shifted plan can cost more iterations than a cold start.
"""
import ctypes as C
import os

import numpy as np
import pytest

import test_ipm_warm_start as wsm
from lpopc_amd import problems
from lpopc_amd.engine import ABI_SYMBOLS, BatchedIPM, NLPEngine, RpmError, lib
from lpopc_amd.group import SweepGroup
from lpopc_amd.problem import Options

NEW_SYMBOLS = ["rpm_ipm_set_initial_states_dev", "rpm_ipm_set_initial_states", "rpm_sweep_set_initial_states"]
SOLVED = ("x", "lambda", "obj", "status", "iterations", "kkt_error")


def test_symbols_exist_and_are_listed(built):
    L = lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rpm_hip.h")).read()
    flat = " ".join(header.split())
    assert "int rpm_ipm_set_initial_states_dev(rpm_ipm* s, int phase, const double* d_state0, void* stream);" in flat
    assert "int rpm_ipm_set_initial_states(rpm_ipm* s, int phase, const double* state0);" in flat
    assert "int rpm_sweep_set_initial_states(rpm_sweep* s, int phase, const double* state0);" in flat
    assert L.rpm_ipm_set_initial_states(None, 0, None) == 1 and L.rpm_ipm_set_initial_states_dev(None, 0, None, None) == 1
    assert L.rpm_sweep_set_initial_states(None, 0, None) == 1


def _same(got, want, keys, what):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (what, k)


def _set(solver, form, states):
    import torch
    if form == "host":
        solver.set_initial_states(0, states)
    else:
        d = torch.from_numpy(np.ascontiguousarray(states)).cuda()
        solver.set_initial_states_dev(0, d)
        torch.cuda.synchronize()


@pytest.mark.gpu
def test_the_solve_equals_the_one_after_set_all_bounds(built):
    eng, XL, XU, idx, x0 = wsm._quadrotor_sweep()
    B = len(x0)
    XL2, XU2, _ = wsm._quadrotor_bounds(eng, B, seed=9, scale=0.02, base=XL)
    cold_s, warm_s = BatchedIPM(eng), BatchedIPM(eng, **wsm.WARM)
    cold_s.set_all_bounds(XL, XU)
    cold = cold_s.solve(x0)
    assert (cold["status"] == 0).all()
    z = cold_s.bound_multipliers()
    warm_s.set_all_bounds(XL2, XU2)
    warm = warm_s.solve(cold["x"], cold["lambda"], z)
    assert (warm["status"] == 0).all()
    for form in ("host", "dev"):
        a, w = BatchedIPM(eng), BatchedIPM(eng, **wsm.WARM)          # fresh solvers: their bounds are the engine's
        _set(a, form, XL[:, idx])
        got = a.solve(x0)
        _same(got, cold, SOLVED, (form, "cold"))
        gz = a.bound_multipliers()
        assert np.array_equal(gz[0], z[0]) and np.array_equal(gz[1], z[1]), form
        _set(w, form, XL[:, idx])                                    # written twice: the second states replace the first
        _set(w, form, XL2[:, idx])
        _same(w.solve(cold["x"], cold["lambda"], z), warm, SOLVED + ("z_L", "z_U"), (form, "warm"))
        a.close()
        w.close()
    # the shares of a sweep get their own rows
    g = SweepGroup(problems.quadrotor(2, 4), [0, 0, 0], B, wsm._exact())
    g.set_initial_states(0, XL[:, idx])
    _same(g.solve(x0), cold, ("x", "lambda", "obj", "status", "iterations"), "sweep")
    with pytest.raises(RpmError) as ei:
        g.set_initial_states(1, XL[:, idx])
    assert ei.value.code == 1 and "phase index is out of range" in str(ei.value)
    g.close()
    for s in (cold_s, warm_s):
        s.close()
    eng.close()


@pytest.mark.gpu
def test_argument_errors_are_decided_on_the_host(built):
    L = lib()
    dp = C.POINTER(C.c_double)
    eng, XL, XU, idx, x0 = wsm._quadrotor_sweep()
    s = BatchedIPM(eng)
    s0 = np.ascontiguousarray(XL[:, idx])
    for phase in (-1, 1):
        assert L.rpm_ipm_set_initial_states(s._h, phase, s0.ctypes.data_as(dp)) == 1
        assert b"phase %d is out of range" % phase in L.rpm_ipm_last_error(s._h)
        assert L.rpm_ipm_set_initial_states_dev(s._h, phase, C.c_void_p(8), None) == 1
    assert L.rpm_ipm_set_initial_states(s._h, 0, None) == 1 and b"state0 is NULL" in L.rpm_ipm_last_error(s._h)
    assert L.rpm_ipm_set_initial_states_dev(s._h, 0, None, None) == 1 and b"state0 is NULL" in L.rpm_ipm_last_error(s._h)
    with pytest.raises(RpmError) as ei:
        s.set_initial_states(0, np.zeros((len(x0), 11)))
    assert "state0 has 33 entries, expected 36" in str(ei.value)
    s.close()
    eng.close()
    # a problem whose initial states are free (the sled's are pinned by events, not by bounds)
    sled = NLPEngine(problems.param_sled(2, 4), Options(), n_instances=2, device=0)
    f = BatchedIPM(sled)
    with pytest.raises(RpmError) as ei:
        f.set_initial_states(0, np.zeros((2, 2)))
    assert ei.value.code == 1 and "variable 0 (initial state 0) is free in the solver's plan" in str(ei.value)
    assert L.rpm_ipm_set_initial_states_dev(f._h, 0, C.c_void_p(8), None) == 1
    assert b"variable 0 (initial state 0) is free" in L.rpm_ipm_last_error(f._h)
    f.close()
    sled.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "dev"])
def test_a_nan_state_stops_its_instance_alone(built, form):
    eng, XL, XU, idx, x0 = wsm._quadrotor_sweep()
    cold_s, warm_s = BatchedIPM(eng), BatchedIPM(eng, **wsm.WARM)
    states = np.array(XL[:, idx])
    _set(cold_s, form, states)
    cold = cold_s.solve(x0)
    z = cold_s.bound_multipliers()
    _set(warm_s, form, states)
    warm = warm_s.solve(cold["x"], cold["lambda"], z)
    assert (cold["status"] == 0).all() and (warm["status"] == 0).all()
    states[1, 7] = np.nan
    _set(cold_s, form, states)
    _set(warm_s, form, states)
    for tag, got, want in (("cold", cold_s.solve(x0), cold), ("warm", warm_s.solve(cold["x"], cold["lambda"], z), warm)):
        assert got["status"][1] == 5, (tag, got["status"])
        for k in SOLVED:
            assert np.array_equal(got[k][[0, 2]], want[k][[0, 2]]), (tag, k)
    for s in (cold_s, warm_s):
        s.close()
    eng.close()


@pytest.mark.gpu
def test_closed_loop_on_the_device_equals_the_host_forms(built):
    import torch
    eng, XL, XU, idx, x0 = wsm._quadrotor_sweep()
    B, n, m = len(x0), eng.n, eng.m
    dt = np.full((B, 1), 0.1)
    noise = np.random.RandomState(31).uniform(-0.01, 0.01, size=(3, B, 12))
    first, cold_s = BatchedIPM(eng), BatchedIPM(eng)
    dev_s, host_s = BatchedIPM(eng, **wsm.WARM), BatchedIPM(eng, **wsm.WARM)
    first.set_all_bounds(XL, XU)
    plan = first.solve(x0)
    assert (plan["status"] == 0).all()
    zl, zu = first.bound_multipliers()
    sh = eng.shift_plan_batch(dt, plan["x"], plan["lambda"], (zl, zu))           # the plan the first step starts from
    assert not sh["nonfinite"].any()
    host = {k: sh[k] for k in ("x", "lambda", "z_L", "z_U")}
    cur = [torch.from_numpy(sh[k]).cuda() for k in ("x", "lambda", "z_L", "z_U")]
    nxt = [torch.empty_like(t) for t in cur]
    d_dt, d_noise = torch.from_numpy(dt).cuda(), torch.from_numpy(noise).cuda()
    d_idx = torch.tensor(idx, device="cuda")
    d_flag = torch.empty(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for step in range(3):
        # ---- the device leg: nothing but B x 12 measured states is formed outside the library's launches
        d_s0 = (cur[0][:, d_idx] + d_noise[step]).contiguous()
        dev_s.set_initial_states_dev(0, d_s0)
        rd = dev_s.solve_dev(cur[0], cur[1], d_z_L=cur[2], d_z_U=cur[3], warm=True)
        dev_s.bound_multipliers_dev(cur[2], cur[3])
        eng.shift_plan_batch_dev(d_dt, cur[0], nxt[0], cur[1], nxt[1], cur[2], cur[3], nxt[2], nxt[3], d_flag)
        torch.cuda.synchronize()
        # ---- the same step through the host forms
        s0 = host["x"][:, idx] + noise[step]
        assert np.array_equal(d_s0.cpu().numpy(), s0)
        XLs, XUs = np.array(XL), np.array(XU)
        XLs[:, idx] = XUs[:, idx] = s0
        host_s.set_all_bounds(XLs, XUs)
        rh = host_s.solve(host["x"], host["lambda"], (host["z_L"], host["z_U"]))
        hz = host_s.bound_multipliers()
        assert np.array_equal(hz[0], rh["z_L"]) and np.array_equal(hz[1], rh["z_U"])
        hs = eng.shift_plan_batch(dt, rh["x"], rh["lambda"], hz)
        for k in ("obj", "status", "iterations", "kkt_error"):
            assert np.array_equal(rd[k], rh[k]), (step, k)
        for t, k in zip(cur, ("x", "lambda", "z_L", "z_U")):
            assert np.array_equal(t.cpu().numpy(), rh[k]), (step, "solved", k)
        for t, k in zip(nxt, ("x", "lambda", "z_L", "z_U")):
            assert np.array_equal(t.cpu().numpy(), hs[k]), (step, "shifted", k)
        assert not d_flag.cpu().numpy().any() and not hs["nonfinite"].any()
        # ---- against a cold solve from the same measured states
        cold_s.set_all_bounds(XLs, XUs)
        cold = cold_s.solve(x0)
        print("closed loop step %d: iterations cold %s, shifted primal + dual %s" % (
            step, list(map(int, cold["iterations"])), list(map(int, rd["iterations"]))))
        assert (cold["status"] == 0).all() and (rd["status"] == 0).all(), (step, cold["status"], rd["status"])
        assert np.all(np.abs(rd["obj"] - cold["obj"]) <= 1e-7 * np.maximum(1.0, np.abs(cold["obj"]))), (step, rd["obj"], cold["obj"])
        host = {k: hs[k] for k in ("x", "lambda", "z_L", "z_U")}
        cur, nxt = nxt, cur
    for s in (first, cold_s, dev_s, host_s):
        s.close()
    eng.close()
