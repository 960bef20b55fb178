"""The exact Lagrangian Hessian on the device (rpm_hess_kernel, rpm_hess_tt_kernel, rpm_hess_end_kernel) against the CPU
oracle, ENTRY BY ENTRY:

    |H_gpu - H_ref|_i  <=  C * 2^-52 * mag_i          (where mag_i == 0 the two must be equal)

mag = Oracle.eval_h_mag: the oracle's own walk with every F, multiplier, sigma, weight and factor replaced by its
absolute value and every subtraction by an addition — the sum of the magnitudes of the terms the entry is made of, 1/den
included, so the same C serves every step.  A global `tol * max|H|` (tests/test_gpu_parity.py::test_exact_hessian before
this module) is larger than 94 to 99 % of the nonzero entries of launch and climb: an entry zeroed or weighted with the
wrong multiplier row passed.

C = 16 = 8 * max(c_ref, 1) rounded up to a power of two, where c_ref is the same ratio between two builds of the oracle
(-ffp-contract=off against -mfma -ffp-contract=fast), measured over every case, step, iterate and draw below
(tests/test_oracle_hessian.py repeats the measurement; profiles/hessian_noise.json has every figure).  c_ref, maximum over
the meshes of a problem, at step 1e-3 / 1e-6:

    hypersensitive   1.06   / 1.14        bryson_denham   0.098 / 4.6e-7    brachistochrone  0.0016 / 1.1e-7
    climb            1.02   / 1.49        quadrotor       0.80  / 0.71      launch           0.81   / 0.52
    analytic first derivatives: hypersensitive 0.92 / 0.82, brachistochrone 0.56 / 0.56

The factor 8 is for what that experiment cannot show: the device's libm and hipcc's own contraction.

The step.  At the default step 1e-6 second differences divide rounding noise by ~1e-12 and the rule, although entrywise,
resolves almost nothing (under 2 % of the entries to 1e-6 of their value).  At step 1e-3 the same kernels, index arithmetic
and assembly run with a million times less noise: every case asserts that the rule then pins at least 70 % of its nonzero
reference entries (pooled over the case's iterates and draws) to 1e-6 of their own value.  The rest are second differences
that are analytically zero (pairs the dependency probe keeps because some output depends on both variables), which no step
resolves.

The iterates sit 15 to 30 % away from the guesses on purpose (tests/_hessian_cases.py::iterates): at the guesses the
functions cancel internally (hover, turnpike, launcher at rest in the rotating frame), and rounding noise then scales with
the cancelled terms, which no magnitude built from F bounds — c_ref there is 70 to 390.

The t0t0, tft0 and tftf scalars.  Every functor shipped here is autonomous: for the pair (t, t) the second difference and
the first-derivative piece are exactly 0 at every node, so eval_h hands rpm_hess_tt_kernel rows of zeros and the three
entries are 0.0 in the oracle and on the device whatever that kernel does.  No comparison of eval_h — N = 300 included —
can see its strided loop or its tree.  test_t0_tf_reduction_on_given_terms runs that kernel alone on random per-node terms
(rpm_debug_hess_tt) instead.  What stays unpinned: the per-node tt terms rpm_hess_kernel writes (kind 3), which are zeros
here and would need a non-autonomous functor with a twin in the oracle.
"""
import numpy as np
import pytest

import _hessian_cases as hc
from lpopc_amd import problems
from lpopc_amd.engine import NLPEngine

pytestmark = pytest.mark.gpu


def _oracle(prob, opts):
    from oracle.oracle import Oracle
    return Oracle(prob, opts)


def _against_the_oracle(prob, opts, coarse, what, name=None):
    eng, orc = NLPEngine(prob, opts, device=0), _oracle(prob, opts)
    assert eng.nnz_h == orc.nnz_h and eng.nnz_h > 0
    hi, hj = eng.eval_h_structure()
    if name is not None:      # the meshes are laid around this tile size: it must be the engine's
        assert eng.get_option("hess_tile_nodes") == hc.TH[name]
    oi, oj = orc.hess_structure()
    assert np.array_equal(hi, oi) and np.array_equal(hj, oj)
    n_ok = n_nz = 0
    worst = 0.0
    for ix, x in enumerate(hc.iterates(orc.starting_point())):
        for sigma, lam in hc.draws(eng.m):
            hv, hr, mag = eng.eval_h(x, sigma, lam), orc.eval_h(x, sigma, lam), orc.eval_h_mag(x, sigma, lam)
            ratio = hc.noise_ratio(hv, hr, mag)
            worst = max(worst, ratio)
            print("%s iterate %d sigma %g: max |d| / (2^-52 mag) = %.3g" % (what, ix, sigma, ratio))
            hc.assert_entrywise(hv, hr, mag, what="%s iterate %d sigma %g" % (what, ix, sigma))
            nz = hr != 0
            n_nz += int(nz.sum())
            n_ok += int(np.sum(hc.C_NOISE * hc.EPS * mag[nz] <= hc.RESOLVED_RTOL * np.abs(hr[nz])))
    eng.close()
    if coarse:
        assert n_ok >= hc.RESOLVED_SHARE * n_nz, (n_ok, n_nz)
    return worst


@pytest.mark.parametrize("step", hc.STEPS, ids=["step1e-3", "step1e-6"])
@pytest.mark.parametrize("cid,name,make", hc.CASES, ids=hc.CASE_IDS)
def test_every_problem_at_two_steps(built, cid, name, make, step):
    """N on both sides of the problem's TH (TH - 1, TH, TH + 1, 2 TH + 3 on ragged meshes), N = 300 (five tiles of 64; the
    t0/tf sums are zeros there as everywhere, see the module docstring), the smallest mesh, Delta-III with all four phases
    and three linkages; two iterates, two draws (one with sigma = 0); structure bit for bit."""
    _against_the_oracle(make(), hc.exact_options(step), step == 1e-3, "%s step %g" % (cid, step), name)


@pytest.mark.parametrize("step", hc.STEPS, ids=["step1e-3", "step1e-6"])
@pytest.mark.parametrize("cid,name,make", hc.ANALYTIC_CASES, ids=[c[0] for c in hc.ANALYTIC_CASES])
def test_analytic_first_derivatives(built, cid, name, make, step):
    """rpm_hess_kernel<P, true> (the D1 pieces of the t0/tf rows from the functor's analytic columns) on both problems
    that have one, over several tiles."""
    _against_the_oracle(make(), hc.exact_options(step, analytic=True), step == 1e-3, "%s step %g" % (cid, step), name)


LINEARITY = [c for c in hc.CASES if c[0] in ("hypersensitive_N131", "hypersensitive_N300", "bryson_denham_N67", "brachistochrone_N67",
                                             "climb_N67", "quadrotor_N11", "launch_N7_8_9_19", "launch_N19_9_8_7")]


@pytest.mark.parametrize("step", hc.STEPS, ids=["step1e-3", "step1e-6"])
@pytest.mark.parametrize("cid,name,make", LINEARITY, ids=[c[0] for c in LINEARITY])
def test_hessian_is_linear_in_sigma_and_lambda(built, cid, name, make, step):
    """eval_h(x, sigma, lambda) = sigma eval_h(x, 1, 0) + eval_h(x, 0, lambda) within 4 * 2^-52 * mag_i: the device against
    itself (the oracle only supplies the yardstick).  It catches a sigma or lambda factor that is missing, doubled or
    applied to the wrong term (sigma on a constraint term, a multiplier on the cost).  It does NOT catch a multiplier read
    from the wrong row: that is still linear, both sides move alike; the oracle comparisons at step 1e-3 catch those."""
    prob, opts = make(), hc.exact_options(step)
    eng, orc = NLPEngine(prob, opts, device=0), _oracle(prob, opts)
    sigma, lam = 0.7, hc.draws(eng.m)[0][1]
    for ix, x in enumerate(hc.iterates(orc.starting_point())):
        whole = eng.eval_h(x, sigma, lam)
        parts = sigma * eng.eval_h(x, 1.0, np.zeros(eng.m)) + eng.eval_h(x, 0.0, lam)
        mag = orc.eval_h_mag(x, sigma, lam)
        print("%s step %g iterate %d: max |d| / (2^-52 mag) = %.3g" % (cid, step, ix, hc.noise_ratio(whole, parts, mag)))
        hc.assert_entrywise(whole, parts, mag, c=4.0, what="%s step %g iterate %d" % (cid, step, ix))
    eng.close()


def _quadrotor_consts(b):
    base = problems.quadrotor(2, 5).GetOpimalProblemFuns().consts
    rng = np.random.RandomState(300 + b)
    return [c * (1.0 + 0.2 * rng.uniform(-1, 1)) for c in base]        # mass, inertia, arm, target, weights: all of them


def _launch_consts(b):
    base = problems.launch().GetOpimalProblemFuns().consts
    rng = np.random.RandomState(400 + b)
    return [c * (1.0 + 0.02 * rng.uniform(-1, 1)) for c in base]        # rotation rate, mu, drag, thrusts, Isp


BATCHES = [
    ("quadrotor", lambda: hc._BUILD["quadrotor"]([3, 4, 4]), _quadrotor_consts, 7),
    ("launch", lambda: hc.launch_with([[5, 2], [8], [4, 5], [6, 7, 6]]), _launch_consts, 5),
]


@pytest.mark.parametrize("name,make,consts_of,B", BATCHES, ids=[c[0] for c in BATCHES])
def test_batch_with_per_instance_constants(built, name, make, consts_of, B):
    """eval_h_dev of B instances, each with its own problem constants (K.consts + inst * consts_stride), equals bit for bit
    a one-instance engine built with that instance's constants; every slot of a NaN-filled output is written."""
    import torch
    opts = hc.exact_options(1e-3)
    many = NLPEngine(make(), opts, n_instances=B, device=0)
    for b in range(B):
        many.set_instance_constants(b, consts_of(b))
    x0 = many.get_starting_point()
    xs = np.stack([hc.iterates(x0)[b % 2] * (1.0 + 0.01 * b) for b in range(B)])
    lam = np.random.RandomState(6).uniform(-1, 1, (B, many.m))
    d_h = torch.full((B, many.nnz_h), np.nan, dtype=torch.float64, device="cuda")
    many.eval_h_dev(torch.from_numpy(xs).cuda(), 0.7, torch.from_numpy(lam).cuda(), d_h)
    torch.cuda.synchronize()
    h = d_h.cpu().numpy()
    many.close()
    assert not np.isnan(h).any()
    for b in range(B):
        prob = make()
        prob.GetOpimalProblemFuns().consts = [float(c) for c in consts_of(b)]
        one = NLPEngine(prob, opts, device=0)
        assert np.array_equal(one.eval_h(xs[b], 0.7, lam[b]), h[b]), b
        one.close()
    assert not np.array_equal(h[0], h[1])


TT_MESHES = [("hypersensitive_N255", lambda: hc._BUILD["hypersensitive"]([15] * 17), 1),
             ("hypersensitive_N257", lambda: hc._BUILD["hypersensitive"]([15] * 16 + [17]), 1),
             ("hypersensitive_N300", lambda: hc._BUILD["hypersensitive"]([15] * 20), 3),
             ("hypersensitive_N600", lambda: hc._BUILD["hypersensitive"]([15] * 40), 2),
             ("launch_N7_8_9_19", lambda: hc.launch_with([[5, 2], [8], [4, 5], [6, 7, 6]]), 3)]


@pytest.mark.parametrize("cid,make,B", TT_MESHES, ids=[c[0] for c in TT_MESHES])
def test_t0_tf_reduction_on_given_terms(built, cid, make, B):
    """rpm_hess_tt_kernel alone on random per-node terms: the three sums of every phase and instance land in the t0t0, tft0
    and tftf slots and equal the exactly rounded sums (math.fsum) within (N - 1) 2^-53 sum|t_i|, the bound of any summation
    order in double precision.  N on both sides of the kernel's 256 threads, and two and three passes of its strided loop;
    a term dropped or counted twice is off by ~1, a million million times the bound."""
    import math
    eng = NLPEngine(make(), hc.exact_options(1e-3), n_instances=B, device=0)
    Ns = [eng.phase_tables(p)["points"].size for p in range(eng.n_phases)]
    rng = np.random.RandomState(9)
    tmp = rng.uniform(-1, 1, (B, 3 * sum(Ns))) * np.exp(rng.uniform(-3, 3, (B, 3 * sum(Ns))))
    out = eng.debug_hess_tt(tmp)
    eng.close()
    off = 0
    for p, N in enumerate(Ns):
        for b in range(B):
            rows = tmp[b, off:off + 3 * N].reshape(3, N)            # terms of t0t0, tftf, tft0
            for slot, row in ((0, rows[0]), (2, rows[1]), (1, rows[2])):
                want, bound = math.fsum(row), (N - 1) * 2.0 ** -53 * float(np.sum(np.abs(row)))
                assert abs(out[b, p, slot] - want) <= bound, (p, b, slot, out[b, p, slot], want)
        off += 3 * N


# ---- the finite-difference Jacobian at a non-default step -------------------------------------------------------------------
G_TOL, JFD_TOL = 1e-12, 1e-8          # tests/test_gpu_parity.py: "a 1-ulp difference in f divided by h ~ 1e-6"
FD_STEP = 1e-3


def rel_err(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def _launch_ragged():
    p = problems.launch()
    meshes = [([-1, -0.6, 0.1, 1], [5, 23, 2]), ([-1, 0.5, 1], [16, 17]), ([-1, 1], [33]),
              ([-1, -0.9, -0.5, 0.0, 0.25, 1], [3, 4, 7, 12, 16])]
    for i, (mesh, nodes) in enumerate(meshes):
        problems.set_mesh(p.GetPhase(i), mesh, nodes)
    return p


JAC_CASES = [("launch_ragged", _launch_ragged), ("climb_16x16", lambda: problems.min_time_climb(16, 16)),
             ("quadrotor_8x8", lambda: problems.quadrotor(8, 8))]


@pytest.mark.parametrize("name,make", JAC_CASES, ids=[c[0] for c in JAC_CASES])
def test_jacobian_at_a_coarse_step_in_all_three_layouts(built, name, make):
    """finite-difference-tol = 1e-3 reaches K.tol of the tile kernels and o->tol of the oracle.  The project's rule for the
    finite-difference Jacobian is one ulp of f divided by h: JFD_TOL * (1e-6 / step) = 1e-11 (two builds of the oracle
    agree to 8e-14 there).  The three layouts stay bit-identical to each other."""
    import torch
    from lpopc_amd.problem import Options
    opts = Options()
    opts.SetNumericValue("finite-difference-tol", FD_STEP)
    prob, B = make(), 3
    orc = _oracle(prob, opts)
    xl, xu, _, _ = orc.bounds()
    xs = np.stack([problems.seeded_iterate(orc.starting_point(), xl, xu, 60 + b) for b in range(B)])
    dx = torch.from_numpy(xs).cuda()
    out = {}
    for layout in ("one_role", "role_looped", "pipelined"):
        eng = NLPEngine(prob, opts, n_instances=B, device=0, role_loop=0 if layout == "one_role" else 1)
        if layout != "one_role":
            eng.set_option("pipeline", 1 if layout == "pipelined" else 0)
        dg = torch.full((B, eng.m), np.nan, dtype=torch.float64, device="cuda")
        dv = torch.full((B, eng.nnz_jac), np.nan, dtype=torch.float64, device="cuda")
        eng.eval_pair_dev(dx, dg, dv)
        torch.cuda.synchronize()
        assert eng.get_option("pipeline_active") == (1 if layout == "pipelined" else 0)
        assert eng.get_option("role_loop") == (0 if layout == "one_role" else 1)
        out[layout] = (dg.cpu().numpy(), dv.cpu().numpy())
        eng.close()
    g, v = out["one_role"]
    assert not np.isnan(g).any() and not np.isnan(v).any()
    for layout in ("role_looped", "pipelined"):
        assert np.array_equal(out[layout][0], g) and np.array_equal(out[layout][1], v), layout
    for b in range(B):
        g_ref, v_ref = orc.eval_g(xs[b]), orc.eval_jac_g(xs[b])
        print("%s instance %d: g %.3g, jac %.3g" % (name, b, rel_err(g[b], g_ref), rel_err(v[b], v_ref)))
        assert rel_err(g[b], g_ref) <= G_TOL
        assert rel_err(v[b], v_ref) <= JFD_TOL * (1e-6 / FD_STEP)
    # the step did reach the kernels: the default step gives another Jacobian
    eng = NLPEngine(prob, device=0)
    assert rel_err(eng.eval_jac_g(xs[0]), v[0]) > 1e-9
    eng.close()
