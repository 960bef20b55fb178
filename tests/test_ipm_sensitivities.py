"""Solution sensitivities of the device solver to variables that are fixed in its plan (rpm_ipm_sensitivities, rpm_ipm_sens.hip):
column k solves the solver's reduced system (13) at the state it holds against minus column var_index[k] of the matrix.

What is compared with what:
  right-hand sides   rpm_ipm_debug_sensitivity_rhs against the numpy restatement of the rule (sums of the same doubles in the same
                     order, from the one-instance engine's eval_jac_g / eval_h at the state's x, lambda): bit for bit
  solutions          against rpm_ipm_debug_solve_dense on the storage rpm_ipm_debug_pass(2) leaves and those right-hand sides — the
                     factor and substitution kernels on the same bits —: bit for bit.  The residual of every column against the
                     long-double matrix of tests/_ipm_pass_reference.py is printed (pytest -s), not asserted
  instances          B = 37 against a B = 1 solver per instance, bit for bit; a warm solve after the call against one without it
  end to end         central differences of the device's own re-solves, bounded by 10 x the same figure of the CPU restatement
                     (oracle/ipm_oracle.py solves, a dense numpy solve of the linearised system), computed here
  predictor          rpm_ipm_apply_sensitivities against its rule in numpy, bit for bit; its miss against the move of the solution
Cases and shapes are those of tests/test_ipm_pass.py."""
import ctypes as C

import numpy as np
import pytest

import _ipm_pass_reference as ref
import test_ipm_pass as tp
import test_ipm_warm_start as ws
from lpopc_amd import problems
from lpopc_amd.engine import BatchedIPM, NLPEngine, RpmError, lib
from lpopc_amd.group import SweepGroup
from lpopc_amd.problem import Options

REINJECT = dict({k: 1e-12 for k in tp.TIGHT}, mu_strategy=0, mu_init=0.1, tol=1e-12)
CASES = [("quadrotor", 0), ("quadrotor", 1), ("bryson_denham", None), ("launch_2x5", None)]
CASE_IDS = ["quadrotor-band", "quadrotor-nested", "bryson_denham", "launch_2x5"]


def _params(case):
    """the parameters of a case: quadrotor the 12 initial states and tf, bryson_denham t0, launch the fixed initial states of
    phase 1 — all fixed in every instance"""
    name, n = case.name, case.eng.n
    fixed = case.XL[0] == case.XU[0]
    states = case.ipm.initial_state_variables(0)
    if name == "quadrotor":
        p = list(states) + [n - 1]
    elif name == "bryson_denham":
        p = [n - 2]
    else:
        p = [int(i) for i in states if fixed[i]]
    assert len(p) > 0 and fixed[p].all(), (name, p)
    return np.array(p, dtype=np.int32)


def _rhs_reference(case, st, params):
    """the rule of include/rpm_hip.h in numpy: (B, P, Nt), unknown order"""
    lay = case.lay
    fixed = case.XL[0] == case.XU[0]
    out = np.zeros((case.B, len(params), lay.nt))
    for b in range(case.B):
        x, lam = st["v"][b][:lay.n], st["lambda"][b]
        jac, hess = case.one.eval_jac_g(x), case.one.eval_h(x, 1.0, lam)
        for k, j in enumerate(params):
            acc = {}
            for e in np.nonzero((lay.hr == j) | (lay.hc == j))[0]:          # ascending triplet index
                i = int(lay.hc[e] if lay.hr[e] == j else lay.hr[e])
                if fixed[i]:
                    continue
                acc[i] = hess[e] if i not in acc else acc[i] + hess[e]
            for i, s in acc.items():
                out[b, k, i] = -s
            ents = np.nonzero(lay.jc == j)[0]
            assert np.unique(lay.jr[ents]).size == ents.size
            out[b, k, lay.nv + lay.jr[ents]] = -jac[ents]
    return out


def _converged_state(case):
    """the (x, lambda, z) of a real solve, pushed by 1e-12 only, with the monotone rule and tol = 1e-12 (so that a pass runs on)"""
    case.start()
    sol = case.ipm.solve(case.X0)
    z = case.ipm.bound_multipliers()
    print("%s: solve for the converged state: status %s" % (case.name, sol["status"]))
    case.set(**REINJECT)
    return sol["x"], sol["lambda"], z


def _state_inputs(case, state):
    return () if state == "interior" else _converged_state(case)


# ---------------------------------------------------------------------------------------------------- 3: right-hand sides
@pytest.mark.gpu
@pytest.mark.parametrize("state", ["interior", "converged"])
@pytest.mark.parametrize("name,nested", CASES, ids=CASE_IDS)
def test_right_hand_sides_bit_for_bit(built, name, nested, state):
    case = tp.Case(name, nested=nested)
    params = _params(case)
    st = case.start(*_state_inputs(case, state))
    assert not st["status"].any()
    got = case.ipm.debug_sensitivity_rhs(params)
    want = _rhs_reference(case, st, params)
    lay = case.lay
    dup = sum(int(((lay.hr == j) | (lay.hc == j)).sum()) for j in params)
    print("%s %s: %d parameters, %d Hessian triplets touch them, %d non-zero right-hand-side entries" %
          (name, state, len(params), dup, int((want != 0).sum())))
    assert (want != 0).any()
    assert np.array_equal(got, want), (name, state, np.argwhere(got != want)[:5].tolist())
    # slacks and fixed unknowns: nothing
    fixed = np.nonzero(case.XL[0] == case.XU[0])[0]
    assert not got[:, :, lay.n:lay.nv].any() and not got[:, :, fixed].any()
    case.close()


# ---------------------------------------------------------------------------------------------------- 4: solutions
@pytest.mark.gpu
@pytest.mark.parametrize("name,nested", CASES, ids=CASE_IDS)
def test_solutions_bit_for_bit_against_the_factor_hook(built, name, nested):
    case = tp.Case(name, nested=nested)
    lay = case.lay
    n, nv, nt = lay.n, lay.nv, lay.nt
    params = _params(case)
    inputs = _converged_state(case)
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
        rhs = case.ipm.debug_sensitivity_rhs(params)
        assert np.array_equal(rhs, _rhs_reference(case, st, params))
        stats = case.ipm.stats()
        sens = case.ipm.sensitivities(params)
        assert case.ipm.stats() == stats
        assert (sens["info"] == 0).all() and (sens["delta_w"] == 0).all(), (sens["info"], sens["delta_w"])
        dense = np.zeros((case.B, nt, nt))
        for b in range(case.B):
            low, _, _ = tp._dense_from_storage(case, out["K"][b])
            dense[b] = low + np.tril(low, -1).T
        for k, j in enumerate(params):
            sol, npos, _ = case.ipm.debug_solve_dense(dense, rhs[:, k, :])
            assert (npos == nv).all()
            assert np.array_equal(sens["dx"][:, k, ~fixed], sol[:, :n][:, ~fixed]), (name, on, k, "dx")
            assert np.array_equal(sens["dlambda"][:, k, :], sol[:, nv:]), (name, on, k, "dlambda")
            assert (sens["dx"][:, k, j] == 1.0).all()
            others = fixed.copy()
            others[j] = False
            assert not sens["dx"][:, k, others].any()
            assert not sol[:, :n][:, fixed].any()
            res = []
            for b in range(case.B):
                r = case.rows(st, b)
                K, _, _ = ref.kkt_13(lay, r["v"], r["vl"], r["vu"], r["zL"], r["zU"], out["jac"][b], out["hess"][b], 0.0, case.o["delta_c"])
                res.append(ref.relative_residual(K, sol[b], rhs[b, k]))
            print("sensitivity residual %s nested %s fused_fill %d column %d (variable %d): %s" %
                  (name, nested, on, k, j, ", ".join("%.2e" % v for v in res)))
        assert np.isfinite(sens["dx"]).all() and np.isfinite(sens["dlambda"]).all() and sens["dx"][:, :, ~fixed].any()
    assert ran >= 1
    case.close()


# ---------------------------------------------------------------------------------------------------- 5: instances, nothing disturbed
def _quadrotor_batch(B):
    eng = NLPEngine(problems.quadrotor(2, 4), ws._exact(), n_instances=B, device=0)
    XL, XU, idx = ws._quadrotor_bounds(eng, B)
    x0 = np.tile(eng.get_starting_point()[:eng.n], (B, 1))
    ipm = BatchedIPM(eng)
    ipm.set_all_bounds(XL, XU)
    return eng, ipm, XL, XU, x0, np.array(idx + [eng.n - 1], dtype=np.int32)


@pytest.mark.gpu
def test_every_instance_as_if_alone_and_nothing_disturbed(built):
    B = 37
    eng, ipm, XL, XU, x0, params = _quadrotor_batch(B)
    sol = ipm.solve(x0)
    assert (sol["status"] == 0).all()
    z = ipm.bound_multipliers()
    stats, times = ipm.stats(), ipm.kernel_times()
    sens = ipm.sensitivities(params)
    assert (sens["info"] == 0).all() and (sens["delta_w"] == 0).all()
    # the statistics, the bound multipliers and the next warm solve are what they are without the call
    assert ipm.stats() == stats and ipm.kernel_times() == times
    z2 = ipm.bound_multipliers()
    assert np.array_equal(z[0], z2[0]) and np.array_equal(z[1], z2[1])
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
    # a B = 1 solver on every instance
    e1 = NLPEngine(problems.quadrotor(2, 4), ws._exact(), n_instances=1, device=0)
    s1 = BatchedIPM(e1)
    for b in range(B):
        s1.set_all_bounds(XL[b:b + 1], XU[b:b + 1])
        one = s1.solve(x0[b:b + 1])
        assert np.array_equal(one["x"][0], sol["x"][b])
        alone = s1.sensitivities(params)
        for k in ("dx", "dlambda", "delta_w", "info"):
            assert np.array_equal(alone[k][0], sens[k][b]), (b, k)
    s1.close()
    e1.close()
    # a NaN in one instance's lambda: that instance is left out, every other one is bit-identical
    bad = 5
    lam = sol["lambda"].copy()
    lam[bad, 3] = np.nan
    ipm.debug_start(sol["x"], sol["lambda"], z)
    clean = ipm.sensitivities(params)
    st = ipm.debug_start(sol["x"], lam, z)
    assert st["status"][bad] == 5
    out = ipm.sensitivities(params)
    assert out["info"][bad] == 2 and np.isnan(out["dx"][bad]).all() and np.isnan(out["dlambda"][bad]).all() and np.isnan(out["delta_w"][bad])
    keep = np.arange(B) != bad
    assert (out["info"][keep] == 0).all()
    for k in ("dx", "dlambda", "delta_w"):
        assert np.array_equal(out[k][keep], clean[k][keep]), k
    ipm.close()
    eng.close()


# ---------------------------------------------------------------------------------------------------- 6, 7: end to end, predictor
def _fd_options():
    o = ws._exact()
    o.SetNumericValue("finite-difference-tol", 1e-4)
    return o


def _with_params(XL, XU, params, values):
    L, U = XL.copy(), XU.copy()
    L[:, params] = values
    U[:, params] = values
    return L, U


def _oracle_figure(prob, XL, XU, x0, params, h):
    """the CPU restatement's figure: sensitivities from a dense solve of the linearised KKT system at oracle/ipm_oracle.py's
    solution against central differences of its re-solves, worst over instances and columns"""
    from oracle import ipm_oracle
    from oracle.oracle import Oracle
    o = Oracle(prob, _fd_options())
    n, m = o.n, o.m
    _, _, gl, gu = o.bounds()
    ji, jj = ref.zero_based(*o.jac_structure(), m, n)
    hi, hj = ref.zero_based(*o.hess_structure(), n, n)
    lay = ref.Layout(n, m, gl, gu, ji, jj, hi, hj)
    worst = 0.0
    for b in range(len(XL)):
        solve = lambda L, U, start: ipm_oracle.solve(o, start, x_l=L, x_u=U, tol=1e-10)
        base = solve(XL[b], XU[b], x0[b])
        assert base["status"] == 0
        x = base["x"]
        S = _dense_sensitivities(o, lay, base, XL[b], XU[b], params)
        for k, j in enumerate(params):
            fd = []
            for sgn in (1.0, -1.0):
                L, U = XL[b].copy(), XU[b].copy()
                L[j] = U[j] = XL[b][j] + sgn * h
                r = solve(L, U, x)
                assert r["status"] == 0
                fd.append(r["x"])
            d = (fd[0] - fd[1]) / (2 * h)
            worst = max(worst, np.abs(d - S[k]).max() / max(1.0, np.abs(S[k]).max()))
    return worst


def _dense_sensitivities(o, lay, sol, xl, xu, params):
    """dx/dp of the barrier problem at the restatement's solution, by a dense solve of the linearised system: W and A there, Sigma
    from z = mu / (distance to the bound) at the barrier parameter of its last iteration (the restatement hands out x, the slacks
    and lambda, not z)"""
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
    jac, hess = o.eval_jac_g(x), o.eval_h(x, 1.0, lam)
    K, _, _ = ref.kkt_13(lay, v, vl, vu, zL, zU, jac, hess, 0.0, 1e-9)
    K = np.asarray(K, dtype=np.float64)
    W = np.zeros((n, n))
    np.add.at(W, (lay.hr, lay.hc), hess)
    W = W + np.tril(W, -1).T
    A = np.zeros((m, n))
    A[lay.jr, lay.jc] = jac
    out = []
    for j in params:
        rhs = np.zeros(nt)
        rhs[:n] = np.where(free[:n], -W[:, j], 0.0)
        rhs[nv:] = -A[:, j]
        d = np.linalg.solve(K, rhs)[:n]
        d[j] = 1.0
        out.append(d)
    return out


@pytest.mark.gpu
def test_predictor(built):
    """7: the predictor's arithmetic bit for bit (host form, device form, captured in a graph), and its quality: after a move of
    all 13 parameters by up to 0.05 it misses the re-solved x by at most a quarter of how far x moved (0.020 against 0.65 on the
    CPU restatement)"""
    import torch
    B = 3
    prob = problems.quadrotor(2, 4)
    eng = NLPEngine(prob, _fd_options(), n_instances=B, device=0)
    XL, XU, idx = ws._quadrotor_bounds(eng, B)
    params = np.array(idx + [eng.n - 1], dtype=np.int32)
    x0 = np.tile(eng.get_starting_point()[:eng.n], (B, 1))
    ipm = BatchedIPM(eng, tol=1e-10)
    ipm.set_all_bounds(XL, XU)
    sol = ipm.solve(x0)
    assert (sol["status"] == 0).all()
    z = ipm.bound_multipliers()
    sens = ipm.sensitivities(params)
    assert (sens["info"] == 0).all()
    d = np.concatenate([np.random.RandomState(3).uniform(-0.05, 0.05, 12), [0.05]])
    delta = np.tile(d, (B, 1))
    want_x, want_l = sol["x"].copy(), sol["lambda"].copy()
    for k in range(len(params)):
        want_x = want_x + sens["dx"][:, k, :] * delta[:, k, None]
        want_l = want_l + sens["dlambda"][:, k, :] * delta[:, k, None]
    got_x, got_l = ipm.apply_sensitivities(params, sens["dx"], delta, sol["x"], sens["dlambda"], sol["lambda"])
    assert np.array_equal(got_x, want_x) and np.array_equal(got_l, want_l)
    assert np.array_equal(ipm.apply_sensitivities(params, sens["dx"], delta, sol["x"]), want_x)      # x alone
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t_dx, t_dl, t_delta, t_x, t_lam = dev(sens["dx"]), dev(sens["dlambda"]), dev(delta), dev(sol["x"]), dev(sol["lambda"])
    t_xo, t_lo = torch.full_like(t_x, float("nan")), torch.full_like(t_lam, float("nan"))
    ipm.apply_sensitivities_dev(params, t_dx, t_delta, t_x, t_xo, t_dl, t_lam, t_lo)
    torch.cuda.synchronize()
    assert np.array_equal(t_xo.cpu().numpy(), want_x) and np.array_equal(t_lo.cpu().numpy(), want_l)
    # the device-resident sensitivities: the same bits as the host form's
    t_dx2, t_dl2 = torch.full_like(t_dx, float("nan")), torch.full_like(t_dl, float("nan"))
    rd = ipm.sensitivities_dev(params, t_dx2, t_dl2)
    assert np.array_equal(t_dx2.cpu().numpy(), sens["dx"]) and np.array_equal(t_dl2.cpu().numpy(), sens["dlambda"])
    assert np.array_equal(rd["info"], sens["info"]) and np.array_equal(rd["delta_w"], sens["delta_w"])
    # captured: one launch, nothing else
    t_xo.fill_(float("nan"))
    t_lo.fill_(float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ipm.apply_sensitivities_dev(params, t_dx, t_delta, t_x, t_xo, t_dl, t_lam, t_lo)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(t_xo.cpu().numpy(), want_x) and np.array_equal(t_lo.cpu().numpy(), want_l)
    # quality
    L2, U2 = _with_params(XL, XU, params, XL[:, params] + delta)
    ipm.set_all_bounds(L2, U2)
    moved = ipm.solve(sol["x"], sol["lambda"], z)
    assert (moved["status"] == 0).all()
    miss = np.abs(moved["x"] - want_x).max(axis=1)
    move = np.abs(moved["x"] - sol["x"]).max(axis=1)
    print("predictor: |x(p + d) - (x + S d)|_inf = %s, |x(p + d) - x|_inf = %s" % (miss, move))
    assert (miss <= 0.25 * move).all(), (miss, move)
    ipm.close()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 5, 14])
def test_predictor_arithmetic_on_several_workgroups(built, P):
    """the predictor's rule bit for bit on arbitrary arrays at quadrotor(8, 8): n = 1038 (three workgroups per instance), m = 769
    (odd: every other row of dlambda starts off a 16-byte boundary), with 1, 5 and all 14 fixed variables as parameters"""
    import torch
    B = 3
    eng = NLPEngine(problems.quadrotor(8, 8), ws._exact(), n_instances=B, device=0)
    ipm = BatchedIPM(eng)
    n, m = eng.n, eng.m
    assert n > 1024 and m % 2 == 1
    fixed = np.nonzero(np.equal(*eng.get_bounds_info()[:2]))[0]
    assert fixed.size == 14
    params = fixed[-P:].astype(np.int32)
    rng = np.random.RandomState(P)
    dx, dl = rng.standard_normal((B, P, n)), rng.standard_normal((B, P, m))
    delta, x, lam = rng.standard_normal((B, P)), rng.standard_normal((B, n)), rng.standard_normal((B, m))
    want_x, want_l = x.copy(), lam.copy()
    for k in range(P):
        want_x = want_x + dx[:, k, :] * delta[:, k, None]
        want_l = want_l + dl[:, k, :] * delta[:, k, None]
    got_x, got_l = ipm.apply_sensitivities(params, dx, delta, x, dl, lam)
    assert np.array_equal(got_x, want_x) and np.array_equal(got_l, want_l)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = [dev(a) for a in (dx, delta, x, dl, lam)]
    t_xo, t_lo = torch.full_like(t[2], float("nan")), torch.full_like(t[4], float("nan"))
    ipm.apply_sensitivities_dev(params, t[0], t[1], t[2], t_xo, t[3], t[4], t_lo)
    torch.cuda.synchronize()
    assert np.array_equal(t_xo.cpu().numpy(), want_x) and np.array_equal(t_lo.cpu().numpy(), want_l)
    ipm.close()
    eng.close()


@pytest.mark.gpu
def test_end_to_end_against_re_solves(built):
    """6: F = max_k |FD_k - dx_k|_inf / max(1, |dx_k|_inf), FD_k the central difference of the device's own re-solves at h = 1e-4,
    at most 10 x the same figure of the CPU restatement, computed here (measured figures: DESIGN.md f-2)"""
    B, h = 3, 1e-4
    prob = problems.quadrotor(2, 4)
    eng = NLPEngine(prob, _fd_options(), n_instances=B, device=0)
    XL, XU, idx = ws._quadrotor_bounds(eng, B)
    params = np.array(idx + [eng.n - 1], dtype=np.int32)
    x0 = np.tile(eng.get_starting_point()[:eng.n], (B, 1))
    ipm = BatchedIPM(eng, tol=1e-10)
    ipm.set_all_bounds(XL, XU)
    sol = ipm.solve(x0)
    assert (sol["status"] == 0).all()
    z = ipm.bound_multipliers()
    sens = ipm.sensitivities(params)
    assert (sens["info"] == 0).all()
    F = 0.0
    for k, j in enumerate(params):
        ends = []
        for sgn in (1.0, -1.0):
            L2, U2 = _with_params(XL, XU, [j], XL[:, [j]] + sgn * h)
            ipm.set_all_bounds(L2, U2)
            r = ipm.solve(sol["x"], sol["lambda"], z)
            assert (r["status"] == 0).all()
            ends.append(r["x"])
        fd = (ends[0] - ends[1]) / (2 * h)
        for b in range(B):
            F = max(F, np.abs(fd[b] - sens["dx"][b, k]).max() / max(1.0, np.abs(sens["dx"][b, k]).max()))
    F_ref = _oracle_figure(prob, XL, XU, x0, params, h)
    print("end to end: device figure %.3e, CPU restatement's figure %.3e" % (F, F_ref))
    assert F <= 10.0 * F_ref, (F, F_ref)
    ipm.close()
    eng.close()


# ---------------------------------------------------------------------------------------------------- 8: refusals
@pytest.mark.gpu
def test_refusals_on_a_live_solver(built):
    L = lib()
    eng, ipm, XL, XU, x0, params = _quadrotor_batch(2)
    n, m, P = eng.n, eng.m, len(params)
    free = int(np.nonzero(XL[0] != XU[0])[0][0])

    def refused(code, text, fn):
        with pytest.raises(RpmError) as ei:
            fn()
        assert ei.value.code == code and text in str(ei.value), (code, text, str(ei.value))

    refused(1, "valid after a finished solve", lambda: ipm.sensitivities(params))                # before any solve
    refused(1, "valid after a finished solve", lambda: ipm.debug_sensitivity_rhs(params))
    sol = ipm.solve(x0)
    assert ipm.sensitivities(params)["info"].tolist() == [0, 0]
    for call in (ipm.sensitivities, ipm.debug_sensitivity_rhs):
        refused(1, "var_index is NULL", lambda: call(None))
        refused(1, "outside 1 .. 32", lambda: call(np.zeros(0, dtype=np.int32)))
        refused(1, "outside 1 .. 32", lambda: call(np.arange(33)))
        refused(1, "is outside the", lambda: call([params[0], n]))
        refused(1, "is outside the", lambda: call([-1]))
        refused(1, "listed twice", lambda: call([params[0], params[1], params[0]]))
        refused(1, "variable %d " % free, lambda: call([params[0], free]))
        refused(1, "is free in the solver's plan", lambda: call([free]))
    vi = params.ctypes.data_as(C.POINTER(C.c_int))
    assert L.rpm_ipm_sensitivities(ipm._h, P, vi, None, None, None, None) == 1 and b"dx is NULL" in L.rpm_ipm_last_error(ipm._h)
    assert L.rpm_ipm_sensitivities_dev(ipm._h, P, vi, None, None, None, None, None) == 1
    assert L.rpm_ipm_debug_sensitivity_rhs(ipm._h, P, vi, None) == 1 and b"rhs is NULL" in L.rpm_ipm_last_error(ipm._h)
    # the predictor
    dx, delta = np.zeros((2, P, n)), np.zeros((2, P))
    refused(1, "x_out and x overlap", lambda: ipm._chk(L.rpm_ipm_apply_sensitivities(
        ipm._h, P, vi, *[a.ctypes.data_as(C.POINTER(C.c_double)) for a in (dx, dx, delta, sol["x"], sol["x"])], None, None)))
    refused(1, "dx, delta, x or x_out is NULL", lambda: ipm.apply_sensitivities(params, dx, None, sol["x"]))
    refused(1, "listed twice", lambda: ipm.apply_sensitivities([params[0], params[0]], dx, delta, sol["x"]))
    # the state of a debug solve hook is no state to take them at; nlp_scaling is out of scope
    ipm.set_option("nlp_scaling", 1)
    refused(2, "nlp_scaling", lambda: ipm.sensitivities(params))
    ipm.set_option("nlp_scaling", 0)
    assert ipm.sensitivities(params)["info"].tolist() == [0, 0]
    ipm.close()
    eng.close()
    # a limited-memory solver
    eng = NLPEngine(problems.quadrotor(2, 4), Options(), n_instances=2, device=0)
    ipm = BatchedIPM(eng)
    ipm.set_all_bounds(XL, XU)
    refused(2, "limited-memory", lambda: ipm.sensitivities(params))
    refused(2, "limited-memory", lambda: ipm.debug_sensitivity_rhs(params))
    ipm.close()
    eng.close()


# ---------------------------------------------------------------------------------------------------- 9: the sweep form
@pytest.mark.gpu
def test_sweep_form(built):
    B = 5
    eng, ipm, XL, XU, x0, params = _quadrotor_batch(B)
    sol = ipm.solve(x0)
    want = ipm.sensitivities(params)
    sweep = SweepGroup(problems.quadrotor(2, 4), [0, 0], B, ws._exact())
    assert [c for _, c in sweep.shares()] == [2, 3]
    for b in range(B):
        sweep.set_bounds(b, XL[b], XU[b])
    with pytest.raises(RpmError, match="valid after a finished solve"):
        sweep.sensitivities(params)
    got_sol = sweep.solve(x0)
    assert np.array_equal(got_sol["x"], sol["x"])
    got = sweep.sensitivities(params)
    for k in ("dx", "dlambda", "delta_w", "info"):
        assert np.array_equal(got[k], want[k]), k
    no_lam = sweep.sensitivities(params, want_lambda=False)
    assert no_lam["dlambda"] is None and np.array_equal(no_lam["dx"], want["dx"])
    with pytest.raises(RpmError, match="share 0"):
        sweep.sensitivities([params[0], params[0]])
    sweep.close()
    ipm.close()
    eng.close()
