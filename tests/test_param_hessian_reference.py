"""The long-double reference of the parameter Hessian (tests/_param_hessian_reference.py) against mathematics, the host
structure of hessian-approximation = exact-parameters against the reference's, and the set-up — all without a device.

1  The dense sum of the walk's triplets (layer b) against central second differences of the Lagrangian written from its
   definition (layer a), both in long double, for all three functors; for sled and oscillator also against central second
   differences, in double, of sigma eval_f + lambda . eval_g of the oracle (whose f and g support nq > 0).
   The figure is max |H_b - H_fd| / max(1, max |H_fd|).  It is neither derivable nor in the project: what it shows is the
   truncation error of FORWARD second differences, O(step) times third derivatives (zero for the sled: bilinear), plus the
   noise of the differences it is compared with.  Measured here over the functors, hc.iterates and hc.draws, worst per step:

       against layer (a), long double:     step 1e-3   sled 1.0e-8   oscillator 8.2e-4   probe 3.2e-4
                                           step 1e-6   sled 3.7e-8   oscillator 8.2e-7   probe 3.3e-7
       against the oracle's f and g:       step 1e-3   sled 9.1e-8   oscillator 8.2e-4
                                           step 1e-6   sled 9.1e-8   oscillator 8.2e-7

   Allowed: 8 x the worst of a row over the functors (the project's own factor in C_NOISE, for compilers and libm the
   experiment cannot show).  A term left out of the walk, a wrong weight or a wrong sign is off by O(1).
   The meshes are small (5 to 7 nodes per phase): the dense differences cost O(n^2) evaluations of the Lagrangian, and every
   formula of the walk is exercised at any N; the meshes of the device tests are checked for their resolved share (2).
2  The resolved share of every case of the device tests at step 1e-3, from the reference alone.
3  nnz_h, hes_i / hes_j of the host structure (rpm_debug_hess_structure: no device) equal the reference's bit for bit; lower
   triangular; the counts of the issue; the right phase's own N in the link columns; with nq = 0 the structure of exact.
4  exact with nq > 0 is still refused; the Options table takes the new value and rejects a misspelt one."""
import numpy as np
import pytest

import _hessian_cases as hc
import _param_hessian_cases as pc
import _param_hessian_reference as R
from lpopc_amd import problems
from lpopc_amd.engine import NLPEngine, RpmError
from lpopc_amd.problem import LpopcException, Options

SMALL = {"sled": (7,), "oscillator": (5, 6), "probe": (5, 6)}
# 8 x the worst measured figure of the row (module docstring)
TOL_A = {1e-3: 8 * 8.2e-4, 1e-6: 8 * 8.2e-7}
TOL_ORACLE = {1e-3: 8 * 8.2e-4, 1e-6: 8 * 8.2e-7}


def _figure(Hb, Hfd):
    return float(np.max(np.abs(Hb - Hfd))) / max(1.0, float(np.max(np.abs(Hfd))))


def _small(functor):
    prob = pc.make(functor, SMALL[functor])
    ref = R.Reference(prob, pc.FUNCTOR[functor])
    x0, m = pc.starting_point(prob)
    return prob, ref, x0, m, ref.dependencies(x0)


@pytest.mark.parametrize("functor", ["sled", "oscillator", "probe"])
def test_walk_against_central_differences_of_the_definition(built, functor):
    prob, ref, x0, m, dep = _small(functor)
    worst = {s: 0.0 for s in hc.STEPS}
    for x in hc.iterates(x0):
        for sigma, lam in hc.draws(m):
            Ha = ref.dense_central(x, sigma, lam)
            assert float(np.max(np.abs(Ha))) > 0.1
            for step in hc.STEPS:
                worst[step] = max(worst[step], _figure(ref.dense(x, sigma, lam, step, np.ones_like(dep)), Ha))
    print("%s against the definition: %s" % (functor, {s: "%.3g" % v for s, v in worst.items()}))
    for step in hc.STEPS:
        assert worst[step] <= TOL_A[step], (step, worst[step])


@pytest.mark.parametrize("functor", ["sled", "oscillator"])
def test_walk_against_central_differences_of_the_oracle(built, functor):
    from oracle.oracle import Oracle
    prob, ref, x0, m, dep = _small(functor)
    o = Oracle(prob)
    assert (o.n, o.m) == (ref.n, m)
    pairs = ref.coupled_pairs()
    worst = {s: 0.0 for s in hc.STEPS}
    for x in hc.iterates(x0):
        for sigma, lam in hc.draws(m):
            fun = lambda y: sigma * o.eval_f(y) + float(lam @ o.eval_g(y))      # noqa: E731
            h = 1e-4 * (1 + np.abs(x))
            H = np.zeros((o.n, o.n))
            f0 = fun(x)
            for i in range(o.n):
                e = np.zeros(o.n)
                e[i] = h[i]
                H[i, i] = (fun(x + e) - 2 * f0 + fun(x - e)) / (h[i] * h[i])
            for (i, j) in pairs:
                ei, ej = np.zeros(o.n), np.zeros(o.n)
                ei[i], ej[j] = h[i], h[j]
                H[i, j] = H[j, i] = (fun(x + ei + ej) - fun(x + ei - ej) - fun(x - ei + ej) + fun(x - ei - ej)) / (4 * h[i] * h[j])
            for step in hc.STEPS:
                worst[step] = max(worst[step], _figure(ref.dense(x, sigma, lam, step, np.ones_like(dep)).astype(np.float64), H))
    print("%s against the oracle's f and g: %s" % (functor, {s: "%.3g" % v for s, v in worst.items()}))
    for step in hc.STEPS:
        assert worst[step] <= TOL_ORACLE[step], (step, worst[step])


@pytest.mark.parametrize("cid", pc.CASE_IDS)
def test_resolved_share_of_the_device_cases(built, cid):
    share = pc.pooled_resolved_share(pc.reference(cid, 1e-3)["runs"])
    print("%s: resolved share %.3f" % (cid, share))
    assert share >= hc.RESOLVED_SHARE


STRUCTURES = [("sled", (7,)), ("sled", (33,)), ("oscillator", (5, 9)), ("oscillator", (33, 31)), ("probe", (9, 5)), ("probe", (2, 40))]


@pytest.mark.parametrize("functor,per_phase", STRUCTURES, ids=["%s_%s" % (f, "_".join(map(str, n))) for f, n in STRUCTURES])
def test_host_structure_without_a_device(built, functor, per_phase):
    prob = pc.make(functor, per_phase)
    ref = R.Reference(prob, pc.FUNCTOR[functor])
    eng = NLPEngine(prob, pc.options(), probe_hessian=False)
    assert eng.nnz_h is None and eng.n == ref.n
    dep = ref.dependencies(eng.get_starting_point())
    hi, hj = eng.debug_hess_structure(dep)
    ri, rj = ref.structure(dep)
    assert hi.size == ri.size and np.array_equal(hi, ri) and np.array_equal(hj, rj)
    assert np.all(hi >= hj) and hj.min() >= 0 and hi.max() < eng.n
    # the counts: what exact has for the dependency pattern, plus the parameter rows
    D = dep.reshape(-1)
    off = 0
    total = 0
    for d, (nI, nE) in zip(ref.ph, ref.counts(dep)):
        nx, nu, nq, nc, N = d.nx, d.nu, d.nq, d.nc, d.N
        nv, nout = nx + nu, nx + nc
        M = D[off:off + nv * nout].reshape(nv, nout).T
        off += nv * nout
        H = (M.T @ M) != 0
        np.fill_diagonal(H, True)
        nnzH = int(H.sum())
        assert nI == N * ((nnzH - nv) // 2 + nv) + 2 * nv * N + 3 + nq * (nv * N + 2) + nq * (nq + 1) // 2
        assert nE == (2 * nx) * (2 * nx - 1) // 2 + 2 * nx + 4 * nx + 3 + nq * (2 * nx + 2) + nq * (nq + 1) // 2
        total += nI + nE
    for (l, r, _, _) in ref.links:
        a, b = ref.ph[l], ref.ph[r]
        w = a.nx + a.nq + b.nx + b.nq          # [xfL, pL, x0R, pR]: the lower triangle of a dense block
        total += w * (w + 1) // 2
    assert hi.size == total
    if ref.links and len(set(per_phase)) > 1:
        # the link columns on the right phase's initial states use ITS node count (no parameter problem needs the border promotion
        # of the reference's left-count quirk): every column of a link entry is a final state of the left phase, an initial
        # state of the right phase or a parameter
        a, b = ref.ph[0], ref.ph[1]
        allowed = ({a.var0 + i * (a.N + 1) + a.N for i in range(a.nx)} | {b.var0 + i * (b.N + 1) for i in range(b.nx)} |
                   {a.p0 + j for j in range(a.nq)} | {b.p0 + j for j in range(b.nq)})
        n_link = sum(1 for _, _, r in ref.entries(dep) if r[0] == "link")
        assert n_link > 0 and set(hj[-n_link:].tolist()) <= allowed and set(hi[-n_link:].tolist()) <= allowed
        assert (b.var0 + (b.N + 1)) in set(hj[-n_link:].tolist()) and a.N != b.N
    eng.close()


@pytest.mark.parametrize("name", ["bryson_denham", "launch"])
def test_without_parameters_the_structure_is_that_of_exact(built, name):
    make = (lambda: problems.bryson_denham()) if name == "bryson_denham" else (lambda: hc.launch_with([[5, 2], [8], [4, 5], [6, 7, 6]]))
    a = NLPEngine(make(), hc.exact_options(), probe_hessian=False)
    b = NLPEngine(make(), pc.options(), probe_hessian=False)
    prob = make()
    n_dep = 0
    for i in range(prob.GetPhaseNum()):
        nx, nu, _, nc, _ = prob.GetPhase(i).get_optimal_info()
        n_dep += (nx + nc) * (nx + nu)
    for seed in (0, 1):
        dep = np.random.RandomState(seed).randint(0, 2, n_dep)
        (ai, aj), (bi, bj) = a.debug_hess_structure(dep), b.debug_hess_structure(dep)
        assert ai.size > 0 and np.array_equal(ai, bi) and np.array_equal(aj, bj)
    a.close()
    b.close()


def test_set_up(built):
    ex = Options()
    ex.SetStringValue("hessian-approximation", "exact")
    with pytest.raises(RpmError) as ei:
        NLPEngine(problems.param_sled(), ex)
    assert "static parameters" in str(ei.value) and "exact-parameters" in str(ei.value)
    o = Options()
    assert o.SetStringValue("hessian-approximation", "exact-parameters")
    assert o.GetStringValue("hessian-approximation") == "exact-parameters"
    with pytest.raises(LpopcException):
        o.SetStringValue("hessian-approximation", "exact-parameter")
    # the value reaches the description the engine is created from
    from lpopc_amd import _abi
    desc, _ = _abi.lower(problems.param_sled(), o, 1, 0, 0, 1)
    assert desc.hessian_approximation == 2
    e = NLPEngine(problems.param_sled(), o, probe_hessian=False)      # accepted, host only
    with pytest.raises(RpmError):
        e.debug_hess_structure(np.zeros(3, dtype=np.int32))             # (nx + nc) (nx + nu) = 6 flags are wanted
    e.close()
