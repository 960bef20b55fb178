"""What the exact Hessian with static parameters (hessian-approximation = exact-parameters) opens: the device solver with
the exact Hessian on parameter problems, LpopcApplication with the option, and the sensitivities of a plan to a static
parameter that is fixed in it (rpm_ipm_parameter_variables, rpm_ipm_sensitivities, the predictor)."""
import numpy as np
import pytest

import _param_hessian_cases as pc
import _param_hessian_reference as R
from lpopc_amd import problems
from lpopc_amd.engine import BatchedIPM, NLPEngine
from lpopc_amd.problem import LpopcException

pytestmark = pytest.mark.gpu


def _solve(prob, opts, nested, starts=None, **solver):
    B = 1 if starts is None else len(starts)
    eng = NLPEngine(prob, opts, n_instances=B, device=0)
    if nested is not None:
        eng.set_option("ipm_nested", nested)
    ipm = BatchedIPM(eng, **solver)
    r = ipm.solve(eng.get_starting_point()[None, :eng.n] if starts is None else starts)
    info = ipm.info()
    ipm.close()
    eng.close()
    return r, info


@pytest.mark.parametrize("nested", [0, 1])
def test_sled_reaches_the_closed_form_optimum(built, nested):
    """param_sled(2, 12): status 0 and |obj - 2.5| < 1e-6, the tolerance of tests/test_ipm_limited_memory.py."""
    r, info = _solve(problems.param_sled(2, 12), pc.options(), nested)
    print("sled nested %d: status %d, %d iterations, obj %.12g, border %d" % (nested, r["status"][0], r["iterations"][0], r["obj"][0], info["border"]))
    assert int(r["status"][0]) == 0 and abs(float(r["obj"][0]) - 2.5) < 1e-6


@pytest.mark.parametrize("nested", [0, 1])
def test_oscillator_ends_where_the_limited_memory_solve_ends(built, nested):
    """param_oscillator(): status 0 and the objective of the limited-memory solve within 1e-5 max(1, |obj|), the exact against
    limited-memory bound of tests/test_ipm_limited_memory.py."""
    lm, _ = _solve(problems.param_oscillator(), None, None)
    assert int(lm["status"][0]) == 0
    r, info = _solve(problems.param_oscillator(), pc.options(), nested)
    print("oscillator nested %d: status %d, %d iterations, obj %.12g (limited-memory %.12g in %d), border %d"
          % (nested, r["status"][0], r["iterations"][0], r["obj"][0], lm["obj"][0], lm["iterations"][0], info["border"]))
    assert int(r["status"][0]) == 0
    assert abs(float(r["obj"][0]) - float(lm["obj"][0])) <= 1e-5 * max(1.0, abs(float(lm["obj"][0])))


def test_seven_perturbed_starts_end_at_one_objective(built):
    prob, B = problems.param_oscillator(), 7
    e = NLPEngine(prob)
    x0 = e.get_starting_point()
    e.close()
    starts = x0[None, :] * (1 + 1e-2 * np.random.RandomState(1).uniform(-1, 1, size=(B, x0.size)))
    starts[0] = x0
    r, _ = _solve(prob, pc.options(), None, starts)
    print("objectives", r["obj"], "iterations", r["iterations"])
    assert (r["status"] == 0).all() and np.ptp(r["obj"]) < 1e-6


def test_application_takes_the_option(built):
    """LpopcApplication with hessian-approximation = exact-parameters and max-grid-num = 3: every NLP of the refinement loop is
    solved on the device with the exact Hessian — status 0 at the first attempt, objective 2.5 to the solver tests' 1e-6 with
    their tolerance (Ipopt-tol = 1e-8; at the application's default 1e-6 the solver stops 1.3e-5 short of it)."""
    from lpopc_amd.application import DeviceIPMSolver, LpopcApplication
    app = LpopcApplication(0)
    app.SetOptimalControlProblem(problems.param_sled(2, 12))
    app.Options().SetStringValue("hessian-approximation", "exact-parameters")
    app.Options().SetIntegerValue("max-grid-num", 3)
    app.Options().SetNumericValue("Ipopt-tol", 1e-8)
    solver = DeviceIPMSolver(app.Options().GetNumericValue("Ipopt-tol"))
    seen, orig = [], solver.SolveNlp

    def spy(nlp):
        ok = orig(nlp)
        seen.append((nlp.n, list(solver.attempts), float(solver.last["obj"][0])))
        return ok
    solver.SolveNlp = spy
    try:
        app.SolveOptimalProblem(nlp_solver=solver)
    except LpopcException as ex:     # "reach the max number of refine grid" is the reference's own ending for a bang-bang control
        assert "reach the max number" in str(ex)
    assert isinstance(app.last_solver, DeviceIPMSolver) and 1 <= len(seen) <= 3
    print("grids: (n, attempts, objective) =", seen)
    for _, attempts, obj in seen:
        assert attempts == [(None, 0, attempts[0][2])]          # one attempt, no bound-relax retry, status 0
        assert abs(obj - 2.5) < 1e-6
    assert abs(app.objective - 2.5) < 1e-6


# ---- sensitivities to a fixed static parameter -----------------------------------------------------------------------------------
P_FIXED, H_FD = 1.3, 1e-4


def _fixed_sled(p=P_FIXED):
    prob = problems.param_sled(2, 12)
    ph = prob.GetPhase(0)
    ph.vparametermin[0] = ph.vparametermax[0] = float(p)
    ph.vparameterguess[0] = float(p)
    return prob


def _fd_options():
    o = pc.options()
    o.SetNumericValue("finite-difference-tol", 1e-4)       # the finite-difference options of tests/test_ipm_sensitivities.py
    return o


def _dense_dx(prob, x, lam, zL, zU, xl, xu, j):
    """d x / d x_j by a dense numpy solve of the linearised KKT system at (x, lambda, z): W from the long-double helper, A from
    the oracle's Jacobian, Sigma from z and the distances to the bounds the solver relaxes by 1e-8 max(1, |bound|).  Unknowns:
    the free variables, one slack per inequality row (A has -1 there; its Sigma from |lambda_r|, which is its bound multiplier,
    over the distance to the nearer bound), the multipliers."""
    from oracle.oracle import Oracle
    from lpopc_amd.problem import Options
    oo = Options()
    oo.SetNumericValue("finite-difference-tol", 1e-4)
    o = Oracle(prob, oo)
    n, m = o.n, o.m
    ref = R.Reference(prob, R.Sled)
    W = ref.dense(x, 1.0, lam, 1e-4, ref.dependencies(o.starting_point())).astype(np.float64)
    ji, jj = o.jac_structure()
    A = np.zeros((m, n))
    A[ji, jj] = o.eval_jac_g(x)                      # (0-based; no duplicate entries)
    _, _, gl, gu = o.bounds()
    srow = np.flatnonzero(gl != gu)
    s_val = o.eval_g(x)[srow]
    s_sig = np.abs(lam[srow]) / np.maximum(np.minimum(s_val - gl[srow], gu[srow] - s_val), 1e-300)
    free = xl != xu
    rl = np.where(free & (xl > -1e19), xl - 1e-8 * np.maximum(1.0, np.abs(xl)), xl)
    ru = np.where(free & (xu < 1e19), xu + 1e-8 * np.maximum(1.0, np.abs(xu)), xu)
    sig = np.where(free & (xl > -1e19), zL / np.maximum(x - rl, 1e-300), 0.0) + np.where(free & (xu < 1e19), zU / np.maximum(ru - x, 1e-300), 0.0)
    f = np.flatnonzero(free)
    nf, ns = f.size, srow.size
    As = np.zeros((m, ns))
    As[srow, np.arange(ns)] = -1.0
    K = np.zeros((nf + ns + m, nf + ns + m))
    K[:nf, :nf] = W[np.ix_(f, f)] + np.diag(sig[f])
    K[nf:nf + ns, nf:nf + ns] = np.diag(s_sig)
    K[:nf, nf + ns:] = A[:, f].T
    K[nf:nf + ns, nf + ns:] = As.T
    K[nf + ns:, :nf] = A[:, f]
    K[nf + ns:, nf:nf + ns] = As
    K[nf + ns:, nf + ns:] = -1e-9 * np.eye(m)
    rhs = np.concatenate([-W[f, j], np.zeros(ns), -A[:, j]])
    d = np.zeros(n)
    d[f] = np.linalg.solve(K, rhs)[:nf]
    d[j] = 1.0
    return d


def test_sensitivities_to_a_fixed_parameter(built):
    """Sled with p fixed at 1.3 (the switch lies on the mesh point, so tf = 2 / sqrt(p) holds on this mesh).  Figures, each at
    most 10 x the same figure of the dense numpy solve (the form and margin of
    tests/test_ipm_sensitivities.py::test_end_to_end_against_re_solves): |d tf / dp + p^(-3/2)|, and the worst entry against
    central differences of the device's re-solves at h = 1e-4.  The predictor moved by 1e-3 lands closer to the re-solve than
    the unmoved plan.

    Everything is asserted on the call a user makes without knowing any option.  On an exact-parameters engine with static
    parameters that call refines its columns (sens_refine automatic = 2 rounds: factors at delta_w = 1e-8, residual against the
    matrix's sources without it): on this bang-bang plan W + Sigma is nearly singular on the states (no curvature, bounds
    inactive, Sigma ~ mu) and the pivot-free LDL^T at delta_w = 0 loses digits — with sens_refine = 0 d tf / dp is off by 1.1e-3
    (MI355X) where the dense solve is off by 5.0e-9, although the device's W matches the helper's to 1.6e-8; the refined
    columns agree with the dense solve to 3.8e-11.  The unrefined call is made afterwards and only printed."""
    prob = _fixed_sled()
    opts = _fd_options()
    eng = NLPEngine(prob, opts, device=0)
    n, m = eng.n, eng.m
    xl, xu, _, _ = eng.get_bounds_info()
    ipm = BatchedIPM(eng, tol=1e-10)
    ns = ipm.info()["n_slacks"]
    params = ipm.parameter_variables(0)
    assert params.tolist() == [n - 1] and xl[n - 1] == xu[n - 1] == P_FIXED
    sol = ipm.solve(eng.get_starting_point()[None, :])
    assert int(sol["status"][0]) == 0
    x, lam = sol["x"][0].copy(), sol["lambda"][0].copy()
    zL, zU = (z[0].copy() for z in ipm.bound_multipliers())
    assert abs(x[n - 2] - 2.0 / np.sqrt(P_FIXED)) < 1e-7
    # the right-hand side: the header's rule in numpy on the device's own triplets, bit for bit
    one = NLPEngine(prob, opts, device=0)
    hi, hj = one.eval_h_structure()
    ji, jj = one.eval_jac_g_structure()
    hess, jac = one.eval_h(x, 1.0, lam), one.eval_jac_g(x)
    one.close()
    fixed = xl == xu
    want = np.zeros(n + ns + m)                       # variables, slacks, multipliers
    acc = {}
    for e in np.nonzero((hi == n - 1) | (hj == n - 1))[0]:            # ascending triplet index, one addition after the other
        i = int(hj[e] if hi[e] == n - 1 else hi[e])
        if not fixed[i]:
            acc[i] = hess[e] if i not in acc else acc[i] + hess[e]
    for i, s in acc.items():
        want[i] = -s
    ents = np.nonzero(jj == n - 1)[0]
    assert np.unique(ji[ents]).size == ents.size and ents.size > 0
    want[n + ns + ji[ents]] = -jac[ents]
    got = ipm.debug_sensitivity_rhs(params)[0, 0]
    assert (want != 0).any() and np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    # the sensitivities
    sens = ipm.sensitivities(params)                                            # the default call
    assert int(sens["info"][0]) == 0
    assert np.array_equal(ipm.sensitivities(params)["dx"], sens["dx"])          # refinement is deterministic
    ipm.set_option("sens_refine", 0)
    plain = ipm.sensitivities(params)
    ipm.set_option("sens_refine", -1)
    dx = sens["dx"][0, 0]
    dense = _dense_dx(prob, x, lam, zL, zU, xl, xu, n - 1)
    exact = -P_FIXED ** -1.5
    fig_tf, fig_tf_dense = abs(dx[n - 2] - exact), abs(dense[n - 2] - exact)
    print("without refinement: |d tf / dp + p^(-3/2)| = %.3e, |dx - dense|_inf = %.3e; with: %.3e"
          % (abs(plain["dx"][0, 0][n - 2] - exact), np.abs(plain["dx"][0, 0] - dense).max(), np.abs(dx - dense).max()))
    ends = []
    for sgn in (1.0, -1.0):
        L, U = xl.copy(), xu.copy()
        L[n - 1] = U[n - 1] = P_FIXED + sgn * H_FD
        ipm.set_all_bounds(L[None, :], U[None, :])
        r = ipm.solve(sol["x"], sol["lambda"], (zL[None, :], zU[None, :]))
        assert int(r["status"][0]) == 0
        ends.append(r["x"][0])
    fd = (ends[0] - ends[1]) / (2 * H_FD)
    fig_fd = np.abs(fd - dx).max() / max(1.0, np.abs(dx).max())
    fig_fd_dense = np.abs(fd - dense).max() / max(1.0, np.abs(dense).max())
    print("d tf / dp: device %.12g, dense solve %.12g, -p^(-3/2) = %.12g" % (dx[n - 2], dense[n - 2], exact))
    print("|d tf / dp + p^(-3/2)|: device %.3e, dense solve %.3e" % (fig_tf, fig_tf_dense))
    print("against central differences of re-solves: device %.3e, dense solve %.3e" % (fig_fd, fig_fd_dense))
    # the predictor
    delta = 1e-3
    pred = ipm.apply_sensitivities(params, sens["dx"], np.array([[delta]]), sol["x"])
    L, U = xl.copy(), xu.copy()
    L[n - 1] = U[n - 1] = P_FIXED + delta
    ipm.set_all_bounds(L[None, :], U[None, :])
    moved = ipm.solve(sol["x"], sol["lambda"], (zL[None, :], zU[None, :]))
    assert int(moved["status"][0]) == 0
    miss, move = np.abs(moved["x"][0] - pred[0]).max(), np.abs(moved["x"][0] - x).max()
    print("predictor: |x(p + d) - (x + S d)|_inf = %.3e, |x(p + d) - x|_inf = %.3e" % (miss, move))
    ipm.close()
    eng.close()
    assert miss < move
    assert fig_tf <= 10.0 * fig_tf_dense, (fig_tf, fig_tf_dense)
    assert fig_fd <= 10.0 * fig_fd_dense, (fig_fd, fig_fd_dense)


@pytest.mark.parametrize("nested", [0, 1])
def test_sensitivities_of_a_batch_in_two_columns(built, nested):
    """Three instances of the sled with p fixed at 1.1, 1.3 and 1.6, two columns (t0 and p), band + border and nested layout,
    the default call: every instance and column bit for bit what a one-instance solver gives for it alone, info 0, and the
    figures of the issue's form — |d tf / dp + p^(-3/2)| and the worst entry of either column against central differences of
    the device's re-solves at h = 1e-4 — each at most 10 x the same figure of the dense numpy solve (independent sources: W
    from the long-double helper, A from the oracle, Sigma from the returned z; a slack row and active control bounds are in
    it).  A residual rule that drifted from the assembled matrix would move the refined columns away from that solve."""
    B, ps = 3, (1.1, 1.3, 1.6)
    prob, opts = _fixed_sled(), _fd_options()
    eng = NLPEngine(prob, opts, n_instances=B, device=0)
    eng.set_option("ipm_nested", nested)
    n = eng.n
    xl, xu, _, _ = eng.get_bounds_info()
    assert xl[n - 3] == xu[n - 3] == 0.0                       # t0 is fixed in the plan
    params = np.array([n - 3, n - 1], dtype=np.int32)
    XL, XU = np.tile(xl, (B, 1)), np.tile(xu, (B, 1))
    XL[:, n - 1] = XU[:, n - 1] = ps
    x0 = np.tile(eng.get_starting_point()[:n], (B, 1))
    x0[:, n - 1] = ps
    ipm = BatchedIPM(eng, tol=1e-10)
    ipm.set_all_bounds(XL, XU)
    sol = ipm.solve(x0)
    assert (sol["status"] == 0).all()
    zL, zU = ipm.bound_multipliers()
    sens = ipm.sensitivities(params)
    assert (sens["info"] == 0).all()
    for b in range(B):                                          # as if alone
        one_e = NLPEngine(prob, opts, device=0)
        one_e.set_option("ipm_nested", nested)
        one = BatchedIPM(one_e, tol=1e-10)
        one.set_all_bounds(XL[b:b + 1], XU[b:b + 1])
        r1 = one.solve(x0[b:b + 1])
        assert np.array_equal(r1["x"][0], sol["x"][b])
        assert np.array_equal(one.sensitivities(params)["dx"][0], sens["dx"][b]), b
        one.close()
        one_e.close()
    fd = []
    for j in params:
        ends = []
        for sgn in (1.0, -1.0):
            L, U = XL.copy(), XU.copy()
            L[:, j] = U[:, j] = XL[:, j] + sgn * H_FD
            ipm.set_all_bounds(L, U)
            r = ipm.solve(sol["x"], sol["lambda"], (zL, zU))
            assert (r["status"] == 0).all()
            ends.append(r["x"])
        fd.append((ends[0] - ends[1]) / (2 * H_FD))
    ipm.close()
    eng.close()
    for b in range(B):
        for k, j in enumerate(params):
            dx = sens["dx"][b, k]
            dense = _dense_dx(prob, sol["x"][b], sol["lambda"][b], zL[b], zU[b], XL[b], XU[b], int(j))
            fig = np.abs(fd[k][b] - dx).max() / max(1.0, np.abs(dx).max())
            fig_dense = np.abs(fd[k][b] - dense).max() / max(1.0, np.abs(dense).max())
            print("nested %d instance %d column %d: against re-solves device %.3e, dense %.3e; |dx - dense|_inf %.3e"
                  % (nested, b, k, fig, fig_dense, np.abs(dx - dense).max()))
            assert fig <= 10.0 * fig_dense, (b, k, fig, fig_dense)
            if j == n - 1:
                exact = -ps[b] ** -1.5
                assert abs(dx[n - 2] - exact) <= 10.0 * abs(dense[n - 2] - exact), (b, dx[n - 2], dense[n - 2], exact)
