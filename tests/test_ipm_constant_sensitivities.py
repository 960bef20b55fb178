"""Solution sensitivities of the device solver to the instances' constants (rpm_ipm_constant_sensitivities, rpm_ipm_sens.hip):
column k solves the solver's reduced system (13) at the state it holds against minus the central difference, over the instance's
own step h = rho (1 + |c_k|), of grad f + J' lambda (free variables) and of g (rows) — include/rpm_hip.h.

What is compared with what:
  column table       ipm_const_table (tests/native/ipm_const_table_test.cpp: brute force, every refusal of the list check, plain and
                     under AddressSanitizer + UBSan) and, from its dump, against a numpy restatement here; no device
  right-hand sides   rpm_ipm_debug_constant_sensitivity_rhs against the rule in numpy, from a one-instance engine's eval_grad_f /
                     eval_g / eval_jac_g with set_instance_constants(0, c+-): bit for bit.  (The restatement walks ALL triplets of a
                     column: those outside the state-dependent block differ by exactly 0 and add 0 * lambda.)
  solutions          against rpm_ipm_debug_solve_dense on the storage rpm_ipm_debug_pass(2) leaves: bit for bit
  instances          B = 37 with per-instance constants against a B = 1 solver per instance, bit for bit; shared constants against
                     the same values set per instance; rpm_set_all_instance_constants against the loop of single calls
  closed form        brachistochrone: t_f ~ g^(-1/2), so dt_f/dg = -t_f / (2 g)
  end to end         central differences of the device's own re-solves, bounded by 10 x the same figure of the CPU restatement
  predictor          rpm_ipm_apply_constant_sensitivities against its rule, bit for bit; its miss against the move of the solution
Shapes are those of tests/test_ipm_pass.py and tests/test_ipm_sensitivities.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _ipm_pass_reference as ref
import test_ipm_pass as tp
import test_ipm_sensitivities as ts
import test_ipm_warm_start as ws
from lpopc_amd import problems
from lpopc_amd.engine import ABI_SYMBOLS, BatchedIPM, NLPEngine, RpmError, lib
from lpopc_amd.group import SweepGroup
from lpopc_amd.problem import Options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lpopc_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "native", "ipm_const_table_test.cpp")] + \
          [os.path.join(CSRC, f) for f in ("rpm_setup.cpp", "rpm_mesh.cpp", "rpm_ipm.cpp", "rpm_ipm_tables.cpp")]
NEW_SYMBOLS = ["rpm_ipm_constant_sensitivities_dev", "rpm_ipm_constant_sensitivities", "rpm_ipm_apply_constant_sensitivities_dev",
               "rpm_ipm_apply_constant_sensitivities", "rpm_ipm_debug_constant_sensitivity_rhs", "rpm_sweep_constant_sensitivities",
               "rpm_set_all_instance_constants"]
RHO = 1e-5                                   # the default of "sens_constant_step"
MASS, ARM, PREF_X, PREF_Y, PREF_Z, WU = 0, 2, 7, 8, 9, 14   # quadrotor's constants (lpopc_amd/problems.py)
QUAD5 = np.array([MASS, ARM, PREF_X, PREF_Z, WU], dtype=np.int32)
# launch: thrust_srb enters the dynamics of phases 1 and 2 only; mu the dynamics and the final event (orbital elements); Re the
# dynamics and the path constraint (lpopc_amd/csrc/problems/problems.hpp)
LAUNCH3 = np.array([16, 9, 14], dtype=np.int32)


# ---------------------------------------------------------------------------------------------------- without a device
@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]], ids=["plain", "asan_ubsan"])
def test_column_table(tmp_path, sanitize):
    flags = ["-std=c++17", "-O0", "-Wall"] + sanitize
    objects = [str(tmp_path / (os.path.basename(src) + ".o")) for src in SOURCES]
    compilers = [subprocess.Popen(["g++"] + flags + ["-c", src, "-o", obj]) for src, obj in zip(SOURCES, objects)]
    assert [c.wait() for c in compilers] == [0] * len(SOURCES)
    exe = str(tmp_path / "ipm_const_table_test")
    subprocess.check_call(["g++"] + sanitize + objects + ["-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "\nok:" in "\n" + r.stdout, r.stdout + r.stderr
    print(r.stdout.strip())
    # the numpy restatement, from what the program dumps of the plan and of the table
    d = subprocess.run([exe, "--dump"], capture_output=True, text=True, timeout=120)
    assert d.returncode == 0 and "ok: dumped" in d.stdout, d.stdout + d.stderr
    cases, cur = {}, None
    for ln in d.stdout.splitlines():
        key, _, rest = ln.partition(" ")
        if key == "case":
            cur = cases.setdefault(rest, {})
        elif key != "ok:":
            cur[key] = np.array(rest.split(), dtype=np.int64)
    assert sorted(cases) == ["launch_band", "launch_nested", "param_sled_fixed", "param_sled_free", "quadrotor_band", "quadrotor_nested"]
    for name, t in cases.items():
        n, m, nv, nnz_nl, nnz = t["sizes"]
        fixed, pos, ji, jj = t["fixed"], t["pos"], t["jac_i"], t["jac_j"]
        assert fixed.size == n and ji.size == nnz and jj.size == nnz and pos.size >= nv + m
        free = np.nonzero(fixed == 0)[0]
        assert np.array_equal(t["var"], free) and np.array_equal(t["var_pos"], pos[free]), name
        assert np.array_equal(t["row_pos"], pos[nv:nv + m]), name
        nl = np.arange(nnz) < nnz_nl
        per = [np.nonzero(nl & (jj == i))[0] for i in free]              # ascending triplet index
        ent = np.concatenate(per) if per else np.zeros(0, dtype=np.int64)
        assert np.array_equal(t["ptr"], np.concatenate([[0], np.cumsum([p.size for p in per])])), name
        assert np.array_equal(t.get("ent", np.zeros(0)), ent) and np.array_equal(t.get("ent_row", np.zeros(0)), ji[ent]), name
        # every triplet of the state-dependent block in a free column is there once, and columns reach beyond that block
        assert ent.size == int((nl & (fixed[jj] == 0)).sum()) > 0 and int((~nl & (fixed[jj] == 0)).sum()) > 0, name


def test_symbols_declared_listed_and_exported(built):
    L = lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
    flat = " ".join(open(os.path.join(ROOT, "include", "rpm_hip.h")).read().split())
    for sig in ("int rpm_ipm_constant_sensitivities_dev(rpm_ipm* s, int n_par, const int* const_index, double* d_dx, double* d_dlambda, "
                "double* delta_w, int* info, void* stream);",
                "int rpm_ipm_constant_sensitivities(rpm_ipm* s, int n_par, const int* const_index, double* dx, double* dlambda, "
                "double* delta_w, int* info);",
                "int rpm_ipm_apply_constant_sensitivities_dev(rpm_ipm* s, int n_par, const int* const_index, const double* d_dx, "
                "const double* d_dlambda, const double* d_delta, const double* d_x, double* d_x_out, const double* d_lambda, "
                "double* d_lambda_out, void* stream);",
                "int rpm_ipm_apply_constant_sensitivities(rpm_ipm* s, int n_par, const int* const_index, const double* dx, "
                "const double* dlambda, const double* delta, const double* x, double* x_out, const double* lambda, double* lambda_out);",
                "int rpm_ipm_debug_constant_sensitivity_rhs(rpm_ipm* s, int n_par, const int* const_index, double* rhs);",
                "int rpm_sweep_constant_sensitivities(rpm_sweep* s, int n_par, const int* const_index, double* dx, double* dlambda, "
                "double* delta_w, int* info);",
                "int rpm_set_all_instance_constants(rpm_engine* e, const double* consts /* n_instances x n */, int n);"):
        assert sig in flat, sig
    dp, ip, vp, i = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p, C.c_int
    assert L.rpm_ipm_constant_sensitivities_dev.argtypes == [vp, i, ip, vp, vp, dp, ip, vp]
    assert L.rpm_ipm_constant_sensitivities.argtypes == [vp, i, ip, dp, dp, dp, ip]
    assert L.rpm_ipm_apply_constant_sensitivities_dev.argtypes == [vp, i, ip] + [vp] * 8
    assert L.rpm_ipm_apply_constant_sensitivities.argtypes == [vp, i, ip] + [dp] * 7
    assert L.rpm_ipm_debug_constant_sensitivity_rhs.argtypes == [vp, i, ip, dp]
    assert L.rpm_sweep_constant_sensitivities.argtypes == [vp, i, ip, dp, dp, dp, ip]
    assert L.rpm_set_all_instance_constants.argtypes == [vp, dp, i]
    a, k = np.zeros(8), np.zeros(2, dtype=np.int32)
    pa, pk = a.ctypes.data_as(dp), k.ctypes.data_as(ip)
    assert L.rpm_ipm_constant_sensitivities_dev(None, 1, pk, None, None, None, None, None) == 1
    assert L.rpm_ipm_constant_sensitivities(None, 1, pk, pa, pa, None, None) == 1
    assert L.rpm_ipm_apply_constant_sensitivities_dev(None, 1, pk, None, None, None, None, None, None, None, None) == 1
    assert L.rpm_ipm_apply_constant_sensitivities(None, 1, pk, pa, None, pa, pa, pa, None, None) == 1
    assert L.rpm_ipm_debug_constant_sensitivity_rhs(None, 1, pk, pa) == 1
    assert L.rpm_sweep_constant_sensitivities(None, 1, pk, pa, None, None, None) == 1
    assert L.rpm_set_all_instance_constants(None, pa, 1) == 1


# ---------------------------------------------------------------------------------------------------- cases
def _consts_of(prob):
    return np.array(prob.userfunction_.consts, dtype=np.float64)


def _instance_consts(base, B, ks):
    """instance 0 keeps the problem's constants, instance b > 0 has the listed ones moved by b per cent"""
    c = np.tile(base, (B, 1))
    for b in range(1, B):
        c[b, ks] *= 1.0 + 0.01 * b
    return c


class _Case(tp.Case):
    """tests/test_ipm_pass.py's Case for a problem its table does not name: seeded interior iterate, random lambda and z"""

    def __init__(self, name, prob, hessian, B):
        self.name, self.opts = name, {}
        options = tp._options(hessian)
        self.eng = NLPEngine(prob, options, n_instances=B, device=0)
        self.one = e = NLPEngine(prob, options, device=0)
        xl, xu, gl, gu = e.get_bounds_info()
        self.XL, self.XU = np.tile(xl, (B, 1)), np.tile(xu, (B, 1))
        x0 = e.get_starting_point()[:e.n]
        self.X0 = np.stack([problems.seeded_iterate(x0, xl, xu, 40 + b) for b in range(B)])
        rng = np.random.RandomState(21)
        self.lam = rng.standard_normal((B, e.m)) * 3.0
        self.z = (np.abs(rng.standard_normal((B, e.n))) * 0.5, np.abs(rng.standard_normal((B, e.n))) * 0.5)
        self.B, self.hessian = B, hessian
        self.ipm = BatchedIPM(self.eng)
        self.ipm.set_all_bounds(self.XL, self.XU)
        jr, jc = ref.zero_based(*e.eval_jac_g_structure(), e.m, e.n)
        hr, hc = ref.zero_based(*e.eval_h_structure(), e.n, e.n)
        self.lay = ref.Layout(e.n, e.m, gl, gu, jr, jc, hr, hc)
        self.gl = gl
        self.o = dict(ref.OPTS)
        self._slots = None


def _make_case(which):
    """-> (case, the constants of every instance (B, nconst), the list); per-instance constants where `own`"""
    if which in ("quadrotor-band", "quadrotor-nested"):
        case, prob, ks, own = tp.Case("quadrotor", nested=int(which.endswith("nested"))), problems.quadrotor(2, 4), QUAD5, True
    elif which == "brachistochrone":
        prob = problems.brachistochrone(3, 7)
        case, ks, own = _Case(which, prob, "exact", 2), np.array([0], dtype=np.int32), True
    elif which == "launch_2x5":
        case, prob, ks, own = tp.Case("launch_2x5"), problems.launch(2, 5), LAUNCH3, False
    else:
        prob = problems.param_sled()
        case, ks, own = _Case(which, prob, "exact-parameters", 2), np.array([0], dtype=np.int32), False
    base = _consts_of(prob)
    consts = _instance_consts(base, case.B, ks) if own else np.tile(base, (case.B, 1))
    if own:
        for b in range(1, case.B):
            case.eng.set_instance_constants(b, consts[b])
    return case, consts, ks


def _rhs_reference(one, lay, fixed, consts, X, LAM, ks, rho=RHO):
    """the rule of include/rpm_hip.h in numpy: (B, P, Nt), unknown order; `one` is left with consts[0]"""
    B = len(X)
    out = np.zeros((B, len(ks), lay.nt))
    cols = [np.nonzero(lay.jc == i)[0] for i in range(lay.n)]          # ascending triplet index
    for b in range(B):
        x, lam, c = np.ascontiguousarray(X[b]), LAM[b], consts[b]
        for k, j in enumerate(ks):
            h = rho * (1.0 + abs(c[j]))
            ev = []
            for moved in (c[j] + h, c[j] - h):
                cc = c.copy()
                cc[j] = moved
                one.set_instance_constants(0, cc)
                ev.append((one.eval_grad_f(x).copy(), one.eval_g(x).copy(), one.eval_jac_g(x).copy()))
            (gp, cp, jp), (gm, cm, jm) = ev
            h2 = h + h
            for i in range(lay.n):
                if fixed[i]:
                    continue
                acc = gp[i] - gm[i]
                for t in cols[i]:
                    acc = acc + (jp[t] - jm[t]) * lam[lay.jr[t]]
                out[b, k, i] = -(acc / h2)
            out[b, k, lay.nv:] = -((cp - cm) / h2)
    one.set_instance_constants(0, consts[0])
    return out


# ---------------------------------------------------------------------------------------------------- 1: right-hand sides
@pytest.mark.gpu
@pytest.mark.parametrize("state", ["interior", "converged"])
@pytest.mark.parametrize("which", ["quadrotor-band", "quadrotor-nested", "brachistochrone", "launch_2x5", "param_sled"])
def test_right_hand_sides_bit_for_bit(built, which, state):
    case, consts, ks = _make_case(which)
    lay = case.lay
    st = case.start(*ts._state_inputs(case, state))
    assert not st["status"].any()
    got = case.ipm.debug_constant_sensitivity_rhs(ks)
    fixed = case.XL[0] == case.XU[0]
    want = _rhs_reference(case.one, lay, fixed, consts, st["v"][:, :lay.n], st["lambda"], ks)
    print("%s %s: %d constants, %d non-zero right-hand-side entries of %d" % (which, state, len(ks), int((want != 0).sum()), want.size))
    for k in range(len(ks)):
        assert (want[:, k, :lay.n] != 0).any() or (want[:, k, lay.nv:] != 0).any(), (which, k)
    assert np.array_equal(got, want), (which, state, np.argwhere(got != want)[:5].tolist())
    assert not got[:, :, lay.n:lay.nv].any() and not got[:, :, np.nonzero(fixed)[0]].any()
    # the hook again: the same bits (the scratch is reused, the engine's constants were not touched)
    assert np.array_equal(case.ipm.debug_constant_sensitivity_rhs(ks), got)
    # a larger step is another right-hand side, by the same rule
    case.ipm.set_option("sens_constant_step", 1e-3)
    got3 = case.ipm.debug_constant_sensitivity_rhs(ks[:1])
    assert np.array_equal(got3, _rhs_reference(case.one, lay, fixed, consts, st["v"][:, :lay.n], st["lambda"], ks[:1], rho=1e-3))
    case.close()


# ---------------------------------------------------------------------------------------------------- 2: solutions
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["quadrotor-band", "quadrotor-nested", "launch_2x5"])
def test_solutions_bit_for_bit_against_the_factor_hook(built, which):
    case, consts, ks = _make_case(which)
    lay = case.lay
    n, nv, nt = lay.n, lay.nv, lay.nt
    inputs = ts._converged_state(case)
    fixed = case.XL[0] == case.XU[0]
    ran = 0
    for on in (1, 0):
        try:
            case.ipm.set_option("fused_fill", on)
        except RpmError:
            assert on == 1
            continue
        ran += 1
        st = case.start(*inputs)
        out = case.ipm.debug_pass(2)
        assert (out["inst"]["status"] == 0).all() and (out["inst"]["delta_w"] == 0).all()
        rhs = case.ipm.debug_constant_sensitivity_rhs(ks)
        assert np.array_equal(rhs, _rhs_reference(case.one, lay, fixed, consts, st["v"][:, :n], st["lambda"], ks))
        stats = case.ipm.stats()
        sens = case.ipm.constant_sensitivities(ks)
        assert case.ipm.stats() == stats
        assert (sens["info"] == 0).all() and (sens["delta_w"] == 0).all(), (sens["info"], sens["delta_w"])
        dense = np.zeros((case.B, nt, nt))
        for b in range(case.B):
            low, _, _ = tp._dense_from_storage(case, out["K"][b])
            dense[b] = low + np.tril(low, -1).T
        for k in range(len(ks)):
            sol, npos, _ = case.ipm.debug_solve_dense(dense, rhs[:, k, :])
            assert (npos == nv).all()
            assert np.array_equal(sens["dx"][:, k, ~fixed], sol[:, :n][:, ~fixed]), (which, on, k, "dx")
            assert np.array_equal(sens["dlambda"][:, k, :], sol[:, nv:]), (which, on, k, "dlambda")
            assert not sens["dx"][:, k, fixed].any() and not sol[:, :n][:, fixed].any()
        assert np.isfinite(sens["dx"]).all() and np.isfinite(sens["dlambda"]).all() and sens["dx"][:, :, ~fixed].any()
    assert ran >= 1
    case.close()


# ---------------------------------------------------------------------------------------------------- 3: instances
def _quad_consts(B, seed=5):
    """per-instance constants of a quadrotor sweep: mass within 5 per cent, the target within 0.2 per axis"""
    base = _consts_of(problems.quadrotor(2, 4))
    rng = np.random.RandomState(seed)
    c = np.tile(base, (B, 1))
    c[:, MASS] *= 1.0 + rng.uniform(-0.05, 0.05, B)
    c[:, PREF_X:PREF_Z + 1] += rng.uniform(-0.2, 0.2, (B, 3))
    return c


@pytest.mark.gpu
def test_every_instance_as_if_alone(built):
    B = 37
    consts = _quad_consts(B)
    eng, ipm, XL, XU, x0, _ = ts._quadrotor_batch(B)
    eng.set_all_instance_constants(consts)
    sol = ipm.solve(x0)
    assert (sol["status"] == 0).all()
    sens = ipm.constant_sensitivities(QUAD5)
    assert (sens["info"] == 0).all() and (sens["delta_w"] == 0).all()
    fixed = XL[0] == XU[0]
    assert not sens["dx"][:, :, fixed].any() and np.abs(sens["dx"]).max(axis=(0, 2)).min() > 0
    # the loop of single calls: the same bits
    eng2, ipm2, _, _, _, _ = ts._quadrotor_batch(B)
    for b in range(B):
        eng2.set_instance_constants(b, consts[b])
    sol2 = ipm2.solve(x0)
    sens2 = ipm2.constant_sensitivities(QUAD5)
    for k in ("x", "lambda", "obj", "status", "iterations"):
        assert np.array_equal(sol2[k], sol[k]), k
    for k in ("dx", "dlambda", "delta_w", "info"):
        assert np.array_equal(sens2[k], sens[k]), k
    ipm2.close()
    eng2.close()
    # a B = 1 solver on every instance
    e1 = NLPEngine(problems.quadrotor(2, 4), ws._exact(), n_instances=1, device=0)
    s1 = BatchedIPM(e1)
    for b in range(B):
        e1.set_instance_constants(0, consts[b])
        s1.set_all_bounds(XL[b:b + 1], XU[b:b + 1])
        one = s1.solve(x0[b:b + 1])
        assert np.array_equal(one["x"][0], sol["x"][b])
        alone = s1.constant_sensitivities(QUAD5)
        for k in ("dx", "dlambda", "delta_w", "info"):
            assert np.array_equal(alone[k][0], sens[k][b]), (b, k)
    s1.close()
    e1.close()
    ipm.close()
    eng.close()


@pytest.mark.gpu
def test_shared_constants_as_if_set_per_instance(built):
    B = 5
    base = _consts_of(problems.quadrotor(2, 4))
    got = []
    for per_instance in (False, True):
        eng, ipm, XL, XU, x0, _ = ts._quadrotor_batch(B)
        if per_instance:
            eng.set_all_instance_constants(np.tile(base, (B, 1)))
        sol = ipm.solve(x0)
        assert (sol["status"] == 0).all()
        got.append((sol, ipm.constant_sensitivities(QUAD5), ipm.debug_constant_sensitivity_rhs(QUAD5)))
        ipm.close()
        eng.close()
    assert np.array_equal(got[0][0]["x"], got[1][0]["x"]) and np.array_equal(got[0][2], got[1][2])
    for k in ("dx", "dlambda", "delta_w", "info"):
        assert np.array_equal(got[0][1][k], got[1][1][k]), k


# ---------------------------------------------------------------------------------------------------- 4: nothing disturbed
@pytest.mark.gpu
def test_nothing_disturbed(built):
    import torch
    B = 5
    consts = _quad_consts(B)
    eng, ipm, XL, XU, x0, _ = ts._quadrotor_batch(B)
    eng.set_all_instance_constants(consts)
    sol = ipm.solve(x0)
    assert (sol["status"] == 0).all()
    z = ipm.bound_multipliers()

    def evaluate():
        d_x = torch.from_numpy(sol["x"]).cuda()
        d_g = torch.full((B, eng.m), float("nan"), dtype=torch.float64, device="cuda")
        d_v = torch.full((B, eng.nnz_jac), float("nan"), dtype=torch.float64, device="cuda")
        eng.eval_pair_dev(d_x, d_g, d_v)
        torch.cuda.synchronize()
        return d_g.cpu().numpy(), d_v.cpu().numpy()

    g0, v0 = evaluate()
    stats, times = ipm.stats(), ipm.kernel_times()
    sens = ipm.constant_sensitivities(QUAD5)
    assert (sens["info"] == 0).all()
    assert ipm.stats() == stats and ipm.kernel_times() == times
    g1, v1 = evaluate()
    assert np.array_equal(g0, g1) and np.array_equal(v0, v1)         # the engine evaluates with ITS constants, as before
    z2 = ipm.bound_multipliers()
    assert np.array_equal(z[0], z2[0]) and np.array_equal(z[1], z2[1])
    # a refused call and the test hook leave them alone as well
    with pytest.raises(RpmError):
        ipm.constant_sensitivities([MASS, MASS])
    ipm.debug_constant_sensitivity_rhs(QUAD5)
    g2, v2 = evaluate()
    assert np.array_equal(g0, g2) and np.array_equal(v0, v2)
    warm_after = ipm.solve(sol["x"], sol["lambda"], z)
    warm_after_stats = ipm.stats()
    again = ipm.solve(x0)
    for k in ("x", "lambda", "obj", "status", "iterations", "kkt_error"):
        assert np.array_equal(again[k], sol[k]), k
    z3 = ipm.bound_multipliers()
    warm_plain = ipm.solve(again["x"], again["lambda"], z3)
    for k in ("x", "lambda", "z_L", "z_U", "obj", "status", "iterations", "kkt_error"):
        assert np.array_equal(warm_after[k], warm_plain[k]), k
    assert ipm.stats() == warm_after_stats
    # the call again, after all that: the same bits
    ipm.solve(x0)
    sens2 = ipm.constant_sensitivities(QUAD5)
    for k in ("dx", "dlambda", "delta_w", "info"):
        assert np.array_equal(sens2[k], sens[k]), k
    ipm.close()
    eng.close()


# ---------------------------------------------------------------------------------------------------- 5: containment, refusals
@pytest.mark.gpu
def test_a_nan_instance_is_left_out_alone(built):
    B, bad = 7, 5
    eng, ipm, XL, XU, x0, _ = ts._quadrotor_batch(B)
    eng.set_all_instance_constants(_quad_consts(B))
    sol = ipm.solve(x0)
    z = ipm.bound_multipliers()
    ipm.debug_start(sol["x"], sol["lambda"], z)
    clean = ipm.constant_sensitivities(QUAD5)
    lam = sol["lambda"].copy()
    lam[bad, 3] = np.nan
    st = ipm.debug_start(sol["x"], lam, z)
    assert st["status"][bad] == 5
    out = ipm.constant_sensitivities(QUAD5)
    assert out["info"][bad] == 2 and np.isnan(out["dx"][bad]).all() and np.isnan(out["dlambda"][bad]).all() and np.isnan(out["delta_w"][bad])
    keep = np.arange(B) != bad
    assert (out["info"][keep] == 0).all()
    for k in ("dx", "dlambda", "delta_w"):
        assert np.array_equal(out[k][keep], clean[k][keep]), k
    ipm.close()
    eng.close()


@pytest.mark.gpu
def test_refusals_on_a_live_solver(built):
    L = lib()
    eng, ipm, XL, XU, x0, _ = ts._quadrotor_batch(2)
    n, m, P = eng.n, eng.m, len(QUAD5)

    def refused(code, text, fn):
        with pytest.raises(RpmError) as ei:
            fn()
        assert ei.value.code == code and text in str(ei.value), (code, text, str(ei.value))

    refused(1, "valid after a finished solve", lambda: ipm.constant_sensitivities(QUAD5))              # before any solve
    refused(1, "valid after a finished solve", lambda: ipm.debug_constant_sensitivity_rhs(QUAD5))
    sol = ipm.solve(x0)
    assert ipm.constant_sensitivities(QUAD5)["info"].tolist() == [0, 0]
    for call in (ipm.constant_sensitivities, ipm.debug_constant_sensitivity_rhs):
        refused(1, "const_index is NULL", lambda: call(None))
        refused(1, "outside 1 .. 32", lambda: call(np.zeros(0, dtype=np.int32)))
        refused(1, "outside 1 .. 32", lambda: call(np.arange(33)))
        refused(1, "is outside the 15 constants", lambda: call([MASS, 15]))
        refused(1, "is outside the 15 constants", lambda: call([-1]))
        refused(1, "constant 7 is listed twice", lambda: call([PREF_X, MASS, PREF_X]))
    ci = QUAD5.ctypes.data_as(C.POINTER(C.c_int))
    assert L.rpm_ipm_constant_sensitivities(ipm._h, P, ci, None, None, None, None) == 1 and b"dx is NULL" in L.rpm_ipm_last_error(ipm._h)
    assert L.rpm_ipm_constant_sensitivities_dev(ipm._h, P, ci, None, None, None, None, None) == 1
    assert L.rpm_ipm_debug_constant_sensitivity_rhs(ipm._h, P, ci, None) == 1 and b"rhs is NULL" in L.rpm_ipm_last_error(ipm._h)
    # the option
    for bad in (0.0, -1e-5, 0.2, float("nan")):
        refused(1, "sens_constant_step", lambda: ipm.set_option("sens_constant_step", bad))
    ipm.set_option("sens_constant_step", 0.1)
    ipm.set_option("sens_constant_step", RHO)
    # the predictor
    dx, delta = np.zeros((2, P, n)), np.zeros((2, P))
    refused(1, "x_out and x overlap", lambda: ipm._chk(L.rpm_ipm_apply_constant_sensitivities(
        ipm._h, P, ci, *[a.ctypes.data_as(C.POINTER(C.c_double)) for a in (dx, dx, delta, sol["x"], sol["x"])], None, None)))
    refused(1, "dx, delta, x or x_out is NULL", lambda: ipm.apply_constant_sensitivities(QUAD5, dx, None, sol["x"]))
    refused(1, "listed twice", lambda: ipm.apply_constant_sensitivities([MASS, MASS], dx, delta, sol["x"]))
    refused(1, "is outside the 15 constants", lambda: ipm.apply_constant_sensitivities([15], dx[:, :1], delta[:, :1], sol["x"]))
    # rpm_set_all_instance_constants
    with pytest.raises(RpmError, match="takes 15 constants"):
        eng.set_all_instance_constants(np.zeros((2, 14)))
    ipm.set_option("nlp_scaling", 1)
    refused(2, "nlp_scaling", lambda: ipm.constant_sensitivities(QUAD5))
    ipm.set_option("nlp_scaling", 0)
    assert ipm.constant_sensitivities(QUAD5)["info"].tolist() == [0, 0]
    ipm.close()
    eng.close()
    # a limited-memory solver
    eng = NLPEngine(problems.quadrotor(2, 4), Options(), n_instances=2, device=0)
    ipm = BatchedIPM(eng)
    ipm.set_all_bounds(XL, XU)
    refused(2, "limited-memory", lambda: ipm.constant_sensitivities(QUAD5))
    refused(2, "limited-memory", lambda: ipm.debug_constant_sensitivity_rhs(QUAD5))
    ipm.close()
    eng.close()
    # a functor without constants
    eng = NLPEngine(problems.bryson_denham(2, 8), ws._exact(), n_instances=2, device=0)
    ipm = BatchedIPM(eng)
    x0 = np.tile(eng.get_starting_point()[:eng.n], (2, 1))
    ipm.solve(x0)
    refused(1, "takes no constants", lambda: ipm.constant_sensitivities([0]))
    refused(1, "takes no constants", lambda: ipm.debug_constant_sensitivity_rhs([0]))
    refused(1, "takes no constants", lambda: ipm.apply_constant_sensitivities([0], np.zeros((2, 1, eng.n)), np.zeros((2, 1)), x0))
    ipm.close()
    eng.close()


@pytest.mark.gpu
def test_sweep_form(built):
    B = 5
    consts = _quad_consts(B)
    eng, ipm, XL, XU, x0, _ = ts._quadrotor_batch(B)
    eng.set_all_instance_constants(consts)
    sol = ipm.solve(x0)
    want = ipm.constant_sensitivities(QUAD5)
    sweep = SweepGroup(problems.quadrotor(2, 4), [0, 0], B, ws._exact())       # one device listed twice
    assert [c for _, c in sweep.shares()] == [2, 3]
    L = lib()
    for r, (first, count) in enumerate(sweep.shares()):        # the shares' engines, each with its own rows
        rows = np.ascontiguousarray(consts[first:first + count])
        assert L.rpm_set_all_instance_constants(L.rpm_sweep_engine(sweep._h, r), rows.ctypes.data_as(C.POINTER(C.c_double)), rows.shape[1]) == 0
    for b in range(B):
        sweep.set_bounds(b, XL[b], XU[b])
    with pytest.raises(RpmError, match="valid after a finished solve"):
        sweep.constant_sensitivities(QUAD5)
    got_sol = sweep.solve(x0)
    assert np.array_equal(got_sol["x"], sol["x"])
    got = sweep.constant_sensitivities(QUAD5)
    for k in ("dx", "dlambda", "delta_w", "info"):
        assert np.array_equal(got[k], want[k]), k
    no_lam = sweep.constant_sensitivities(QUAD5, want_lambda=False)
    assert no_lam["dlambda"] is None and np.array_equal(no_lam["dx"], want["dx"])
    with pytest.raises(RpmError, match="share 0"):
        sweep.constant_sensitivities([MASS, MASS])
    sweep.close()
    ipm.close()
    eng.close()


# ---------------------------------------------------------------------------------------------------- 6: closed form
@pytest.mark.gpu
def test_brachistochrone_closed_form(built):
    """t_f ~ g^(-1/2) — exactly so for the discretised problem, the bounds on v staying inactive —, so dt_f/dg = -t_f / (2 g):
    |dt_f/dg + t_f / (2 g)| <= 1e-6 t_f / (2 g).  The CPU restatement attains 1.2e-9; a missing term or a wrong sign is an error of
    order 1; three orders are left for device rounding."""
    prob = problems.brachistochrone(3, 7)
    g = _consts_of(prob)[0]
    eng = NLPEngine(prob, ws._exact(), n_instances=1, device=0)
    ipm = BatchedIPM(eng, tol=1e-10)
    sol = ipm.solve(eng.get_starting_point()[:eng.n].reshape(1, -1))
    assert sol["status"][0] <= 1, sol["status"]
    sens = ipm.constant_sensitivities([0])
    tf = sol["x"][0, eng.n - 1]
    got, want = sens["dx"][0, 0, eng.n - 1], -tf / (2.0 * g)
    print("brachistochrone: t_f %.10f, dt_f/dg %.12g, closed form %.12g, relative error %.2e, info %d" %
          (tf, got, want, abs(got - want) / abs(want), sens["info"][0]))
    assert abs(sol["obj"][0] - tf) < 1e-9 and 0.5 < tf < 1.5
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    ipm.close()
    eng.close()


# ---------------------------------------------------------------------------------------------------- 7: end to end
def _quad_with(consts):
    prob = problems.quadrotor(2, 4)
    prob.userfunction_.consts = [float(v) for v in consts]
    return prob


def _dense_const_sensitivities(lay, o, sol, xl, xu, c, ks, rho):
    """dx/dc of the barrier problem at the restatement's solution: the matrix of tests/test_ipm_sensitivities.py's
    _dense_sensitivities, the right-hand side by the rule of include/rpm_hip.h from restatements with c+- """
    from oracle.oracle import Oracle
    n, m, nv, nt = lay.n, lay.m, lay.nv, lay.nt
    x, lam = sol["x"], sol["lambda"]
    _, _, gl, gu = o.bounds()
    v = np.concatenate([x, sol["slack"]])
    vl, vu = np.concatenate([xl, gl[lay.srow]]), np.concatenate([xu, gu[lay.srow]])
    free = vl != vu
    rel = 1e-8
    vl = np.where(free & (vl > -ref.INF), vl - rel * np.maximum(1.0, np.abs(vl)), vl)
    vu = np.where(free & (vu < ref.INF), vu + rel * np.maximum(1.0, np.abs(vu)), vu)
    mu = sol["trace"][-1]["mu"]
    zL = np.where(free & (vl > -ref.INF), mu / np.maximum(v - vl, 1e-300), 0.0)
    zU = np.where(free & (vu < ref.INF), mu / np.maximum(vu - v, 1e-300), 0.0)
    K, _, _ = ref.kkt_13(lay, v, vl, vu, zL, zU, o.eval_jac_g(x), o.eval_h(x, 1.0, lam), 0.0, 1e-9)
    K = np.asarray(K, dtype=np.float64)
    out = []
    for j in ks:
        h = rho * (1.0 + abs(c[j]))
        ends = []
        for moved in (c[j] + h, c[j] - h):
            cc = c.copy()
            cc[j] = moved
            oc = Oracle(_quad_with(cc), ts._fd_options())
            ends.append((oc.eval_grad_f(x), oc.eval_g(x), oc.eval_jac_g(x)))
        (gp, cp, jp), (gm, cm, jm) = ends
        dl = gp - gm
        np.add.at(dl, lay.jc, (jp - jm) * lam[lay.jr])
        rhs = np.zeros(nt)
        rhs[:n] = np.where(free[:n], -dl / (2 * h), 0.0)
        rhs[nv:] = -(cp - cm) / (2 * h)
        d = np.linalg.solve(K, rhs)[:n]
        d[~free[:n]] = 0.0
        out.append(d)
    return out


def _oracle_figure(XL, XU, x0, consts, ks, hfd):
    """the CPU restatement's figure (oracle/ipm_oracle.py solves): the dense sensitivities against central differences of its
    re-solves with constant k moved by -+ hfd (1 + |c_k|), worst over instances and columns"""
    from oracle import ipm_oracle
    from oracle.oracle import Oracle
    worst = 0.0
    for b in range(len(XL)):
        c = consts[b]
        o = Oracle(_quad_with(c), ts._fd_options())
        _, _, gl, gu = o.bounds()
        ji, jj = ref.zero_based(*o.jac_structure(), o.m, o.n)
        hi, hj = ref.zero_based(*o.hess_structure(), o.n, o.n)
        lay = ref.Layout(o.n, o.m, gl, gu, ji, jj, hi, hj)
        base = ipm_oracle.solve(o, x0[b], x_l=XL[b], x_u=XU[b], tol=1e-10)
        assert base["status"] == 0
        S = _dense_const_sensitivities(lay, o, base, XL[b], XU[b], c, ks, RHO)
        for k, j in enumerate(ks):
            h = hfd * (1.0 + abs(c[j]))
            fd = []
            for sgn in (1.0, -1.0):
                cc = c.copy()
                cc[j] = c[j] + sgn * h
                r = ipm_oracle.solve(Oracle(_quad_with(cc), ts._fd_options()), base["x"], x_l=XL[b], x_u=XU[b], tol=1e-10)
                assert r["status"] == 0
                fd.append(r["x"])
            d = (fd[0] - fd[1]) / (2 * h)
            worst = max(worst, np.abs(d - S[k]).max() / max(1.0, np.abs(S[k]).max()))
    return worst


@pytest.mark.gpu
def test_end_to_end_against_re_solves(built):
    """F = max |FD_k - dx_k|_inf / max(1, |dx_k|_inf), FD_k the central difference of the device's own re-solves with constant k moved
    by -+ 1e-4 (1 + |c_k|) — the 30 moved problems ride as the instances of one batch —, at most 10 x the same figure of the CPU
    restatement, computed here (5.4e-5 when the issue was written)."""
    B, hfd = 3, 1e-4
    ks = QUAD5
    P = len(ks)
    prob = problems.quadrotor(2, 4)
    consts = np.tile(_consts_of(prob), (B, 1))
    eng = NLPEngine(prob, ts._fd_options(), n_instances=B, device=0)
    XL, XU, _ = ws._quadrotor_bounds(eng, B)
    x0 = np.tile(eng.get_starting_point()[:eng.n], (B, 1))
    ipm = BatchedIPM(eng, tol=1e-10)
    ipm.set_all_bounds(XL, XU)
    sol = ipm.solve(x0)
    assert (sol["status"] == 0).all()
    z = ipm.bound_multipliers()
    sens = ipm.constant_sensitivities(ks)
    assert (sens["info"] == 0).all()
    ipm.close()
    eng.close()
    # instance (b, k, s) of the moved batch
    rep = lambda a: np.repeat(a, 2 * P, axis=0)
    moved, steps = rep(consts), np.zeros((B, P))
    for b in range(B):
        for k, j in enumerate(ks):
            steps[b, k] = hfd * (1.0 + abs(consts[b, j]))
            moved[(b * P + k) * 2 + 0, j] = consts[b, j] + steps[b, k]
            moved[(b * P + k) * 2 + 1, j] = consts[b, j] - steps[b, k]
    eng2 = NLPEngine(prob, ts._fd_options(), n_instances=2 * P * B, device=0)
    eng2.set_all_instance_constants(moved)
    ipm2 = BatchedIPM(eng2, tol=1e-10)
    ipm2.set_all_bounds(rep(XL), rep(XU))
    r = ipm2.solve(rep(sol["x"]), rep(sol["lambda"]), (rep(z[0]), rep(z[1])))
    assert (r["status"] == 0).all(), r["status"]
    ipm2.close()
    eng2.close()
    xs = r["x"].reshape(B, P, 2, -1)
    F = 0.0
    for b in range(B):
        for k in range(P):
            fd = (xs[b, k, 0] - xs[b, k, 1]) / (2 * steps[b, k])
            F = max(F, np.abs(fd - sens["dx"][b, k]).max() / max(1.0, np.abs(sens["dx"][b, k]).max()))
    F_ref = _oracle_figure(XL, XU, x0, consts, ks, hfd)
    print("end to end: device figure %.3e, CPU restatement's figure %.3e, |S|_inf %s" %
          (F, F_ref, np.abs(sens["dx"]).max(axis=(0, 2))))
    assert F <= 10.0 * F_ref, (F, F_ref)


# ---------------------------------------------------------------------------------------------------- 8: predictor
@pytest.mark.gpu
def test_predictor(built):
    """the predictor's arithmetic bit for bit (host form, device form, replayed from a graph), and its quality: after a move of the
    mass by up to 0.06 and of the target by up to 0.05 per axis it misses the re-solved x by at most a tenth of how far x moved (the
    CPU restatement: a 136th or better)"""
    import torch
    B = 3
    ks = np.array([MASS, PREF_X, PREF_Y, PREF_Z], dtype=np.int32)
    prob = problems.quadrotor(2, 4)
    consts = np.tile(_consts_of(prob), (B, 1))
    eng = NLPEngine(prob, ts._fd_options(), n_instances=B, device=0)
    XL, XU, _ = ws._quadrotor_bounds(eng, B)
    x0 = np.tile(eng.get_starting_point()[:eng.n], (B, 1))
    ipm = BatchedIPM(eng, tol=1e-10)
    ipm.set_all_bounds(XL, XU)
    sol = ipm.solve(x0)
    assert (sol["status"] == 0).all()
    z = ipm.bound_multipliers()
    sens = ipm.constant_sensitivities(ks)
    assert (sens["info"] == 0).all()
    delta = np.random.RandomState(3).uniform(-1.0, 1.0, (B, len(ks))) * np.array([0.06, 0.05, 0.05, 0.05])
    want_x, want_l = sol["x"].copy(), sol["lambda"].copy()
    for k in range(len(ks)):
        want_x = want_x + sens["dx"][:, k, :] * delta[:, k, None]
        want_l = want_l + sens["dlambda"][:, k, :] * delta[:, k, None]
    got_x, got_l = ipm.apply_constant_sensitivities(ks, sens["dx"], delta, sol["x"], sens["dlambda"], sol["lambda"])
    assert np.array_equal(got_x, want_x) and np.array_equal(got_l, want_l)
    assert np.array_equal(ipm.apply_constant_sensitivities(ks, sens["dx"], delta, sol["x"]), want_x)      # x alone
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t_dx, t_dl, t_delta, t_x, t_lam = dev(sens["dx"]), dev(sens["dlambda"]), dev(delta), dev(sol["x"]), dev(sol["lambda"])
    t_xo, t_lo = torch.full_like(t_x, float("nan")), torch.full_like(t_lam, float("nan"))
    ipm.apply_constant_sensitivities_dev(ks, t_dx, t_delta, t_x, t_xo, t_dl, t_lam, t_lo)
    torch.cuda.synchronize()
    assert np.array_equal(t_xo.cpu().numpy(), want_x) and np.array_equal(t_lo.cpu().numpy(), want_l)
    # the device-resident sensitivities: the same bits as the host form's
    t_dx2, t_dl2 = torch.full_like(t_dx, float("nan")), torch.full_like(t_dl, float("nan"))
    rd = ipm.constant_sensitivities_dev(ks, t_dx2, t_dl2)
    assert np.array_equal(t_dx2.cpu().numpy(), sens["dx"]) and np.array_equal(t_dl2.cpu().numpy(), sens["dlambda"])
    assert np.array_equal(rd["info"], sens["info"]) and np.array_equal(rd["delta_w"], sens["delta_w"])
    # captured: one launch, nothing else
    t_xo.fill_(float("nan"))
    t_lo.fill_(float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ipm.apply_constant_sensitivities_dev(ks, t_dx, t_delta, t_x, t_xo, t_dl, t_lam, t_lo)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(t_xo.cpu().numpy(), want_x) and np.array_equal(t_lo.cpu().numpy(), want_l)
    # quality
    after = consts.copy()
    after[:, ks] += delta
    eng.set_all_instance_constants(after)
    moved = ipm.solve(sol["x"], sol["lambda"], z)
    assert (moved["status"] == 0).all()
    miss = np.abs(moved["x"] - want_x).max(axis=1)
    move = np.abs(moved["x"] - sol["x"]).max(axis=1)
    print("predictor: |x(c + d) - (x + S d)|_inf = %s, |x(c + d) - x|_inf = %s" % (miss, move))
    assert (miss <= move / 10.0).all(), (miss, move)
    ipm.close()
    eng.close()
