"""The exact Hessian with static parameters (hessian-approximation = exact-parameters) on the device, ENTRY BY ENTRY against
the long-double reference of tests/_param_hessian_reference.py (the oracle's Hessian is nq = 0 only):

    |H_gpu - H_ref|_i  <=  C_i * 2^-52 * mag_i          (where mag_i == 0 the two must be equal)

C_i = hc.C_NOISE (tests/_hessian_cases.py) for an entry computed at one node or endpoint; for the entries
rpm_hess_tt_kernel sums over the nodes — t0t0, tft0, tftf and the parameter scalars (p, t0), (p, tf), (p, p') — plus one per
addition level: ceil(log2(min(N, 256))) of the tree and ceil(N / 256) of the strided loop.  Steps, iterates and draws are
those of tests/test_gpu_hessian.py; at step 1e-3 the pooled resolved share is asserted as there.

The probe functor (tests/user_problems/param_hessian_probe.hpp) is non-autonomous and has parameters in every callback: the
kind-3 per-node terms, the reduction's strided loop (N = 300) and the reduced parameter rows all see non-zero data here,
which no shipped functor gives tests/test_gpu_hessian.py."""
import numpy as np
import pytest

import _hessian_cases as hc
import _param_hessian_cases as pc
from lpopc_amd.engine import NLPEngine, RpmError

pytestmark = pytest.mark.gpu


def _engine(case, step, **kw):
    _, functor, per_phase, analytic = case
    return NLPEngine(pc.make(functor, per_phase), pc.options(step, analytic), device=0, **kw)


@pytest.mark.parametrize("step", hc.STEPS, ids=["step1e-3", "step1e-6"])
@pytest.mark.parametrize("case", pc.CASES, ids=pc.CASE_IDS)
def test_entry_by_entry(built, case, step):
    """Sled N = 2, 31, 32, 33, 67, 300; oscillator and probe on phases (31, 33), (67, 32), (2, 300); sled with analytic first
    derivatives (rpm_hess_kernel<P, true>).  Structure bit for bit, TH = 32 asserted, two iterates, two draws."""
    r = pc.reference(case[0], step)
    eng = _engine(case, step)
    hi, hj = eng.eval_h_structure()
    assert eng.get_option("hess_tile_nodes") == pc.TH
    assert np.array_equal(hi, r["structure"][0]) and np.array_equal(hj, r["structure"][1])
    c = pc.entry_constants(r["reduced"])
    for ix, (x, sigma, lam, href, mag) in enumerate(r["runs"]):
        hv = eng.eval_h(x, sigma, lam)
        ratio = hc.noise_ratio(hv, href, mag)
        print("%s step %g run %d sigma %g: max |d| / (2^-52 mag) = %.3g" % (case[0], step, ix, sigma, ratio))
        assert np.all(np.isfinite(hv))
        d = np.abs(hv - href)
        bad = np.flatnonzero(~(d <= c * hc.EPS * mag))
        assert bad.size == 0, ("%d of %d entries off; first %d (%d, %d): got %.17g, reference %.17g, |d| = %.3g * 2^-52 mag"
                               % (bad.size, hv.size, bad[0], hi[bad[0]], hj[bad[0]], hv[bad[0]], href[bad[0]],
                                  d[bad[0]] / max(hc.EPS * mag[bad[0]], 1e-300)))
    eng.close()
    if step == 1e-3:
        assert pc.pooled_resolved_share(r["runs"]) >= hc.RESOLVED_SHARE


def test_hessian_is_linear_in_sigma_and_lambda(built):
    """eval_h(x, sigma, lambda) = sigma eval_h(x, 1, 0) + eval_h(x, 0, lambda) within 4 * 2^-52 * mag_i on the probe functor
    (the check of tests/test_gpu_hessian.py, the device against itself)."""
    case = pc.CASES[pc.CASE_IDS.index("probe_N67_32")]
    for step in hc.STEPS:
        r = pc.reference(case[0], step)
        eng = _engine(case, step)
        for ix in (0, 2):                        # the sigma = 0.7 draw of either iterate
            x, sigma, lam, _, mag = r["runs"][ix]
            whole = eng.eval_h(x, sigma, lam)
            parts = sigma * eng.eval_h(x, 1.0, np.zeros(eng.m)) + eng.eval_h(x, 0.0, lam)
            print("step %g run %d: max |d| / (2^-52 mag) = %.3g" % (step, ix, hc.noise_ratio(whole, parts, mag)))
            hc.assert_entrywise(whole, parts, mag, c=4.0, what="step %g run %d" % (step, ix))
        eng.close()


def test_batch_with_per_instance_constants(built):
    """n_instances = 3 of the oscillator, each with its own damping and weight: every instance is bit for bit what it is alone."""
    import torch
    B, opts = 3, pc.options(1e-3)
    make = lambda: pc.make("oscillator", (67, 32))         # noqa: E731
    consts = lambda b: [0.4 * (1.0 + 0.1 * b), 0.05 * (1.0 - 0.2 * b)]     # noqa: E731
    many = NLPEngine(make(), opts, n_instances=B, device=0)
    for b in range(B):
        many.set_instance_constants(b, consts(b))
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
        prob.GetOpimalProblemFuns().consts = [float(c) for c in consts(b)]
        one = NLPEngine(prob, opts, device=0)
        assert np.array_equal(one.eval_h(xs[b], 0.7, lam[b]), h[b]), b
        one.close()
    assert not np.array_equal(h[0], h[1])


def test_without_parameters_it_is_exact_bit_for_bit(built):
    """exact-parameters on brachistochrone (nq = 0): structure and eval_h are those of exact, bit for bit."""
    prob = hc._BUILD["brachistochrone"](hc._split(67, 32))
    a, b = NLPEngine(prob, hc.exact_options(1e-3), device=0), NLPEngine(prob, pc.options(1e-3), device=0, probe_hessian=False)
    assert b.nnz_h is None                       # (set up on the host only: the probe runs with the first call that needs it)
    for u, v in zip(a.eval_h_structure(), b.eval_h_structure()):
        assert np.array_equal(u, v)
    assert a.nnz_h == b.nnz_h
    for x in hc.iterates(a.get_starting_point()):
        for sigma, lam in hc.draws(a.m):
            assert np.array_equal(a.eval_h(x, sigma, lam), b.eval_h(x, sigma, lam))
    a.close()
    b.close()


def test_reduction_hook_refuses_parameter_rows(built):
    eng = _engine(pc.CASES[0], 1e-3)
    with pytest.raises(RpmError) as ei:
        eng.debug_hess_tt(np.zeros((1, 3 * 2)))
    assert "parameter rows" in str(ei.value)
    eng.close()


def _directional_second_difference(fun, x, d, h):
    return (fun(x + h * d) - 2.0 * fun(x) + fun(x - h * d)) / (h * h)


def test_oracle_free_end_to_end(built):
    """Central second differences of the engine's own sigma eval_f + lambda . eval_g (paths with their own parity tests) along
    three random directions against d' H d of the device Hessian, probe functor.  The tolerance is 8 x what the helper's dense
    Hessian shows against the same differences (their worst over the three directions).  Step 1e-3: what the helper shows is
    the truncation error of forward second differences, O(step), which the device shares; at the default step 1e-6 the helper
    (long double) is off by 2e-7 while any evaluation in double carries 2^-52 mag / step^2 ~ 1e-5 of rounding noise (measured:
    1e-5 to 4e-5 on the device) — a bound from the helper's error then says nothing about a double-precision Hessian, and the
    entrywise rule above is what pins that step."""
    case = pc.CASES[pc.CASE_IDS.index("probe_N31_33")]
    step = 1e-3
    r = pc.reference(case[0], step)
    eng = _engine(case, step)
    hi, hj = eng.eval_h_structure()
    x, sigma, lam, _, _ = r["runs"][0]
    hv = eng.eval_h(x, sigma, lam)
    H = np.zeros((eng.n, eng.n))
    np.add.at(H, (hi, hj), hv)
    H = H + np.tril(H, -1).T
    H_ref = r["ref"].dense(x, sigma, lam, step, r["dep"]).astype(np.float64)
    fun = lambda y: sigma * eng.eval_f(y) + float(lam @ eng.eval_g(y))     # noqa: E731
    rng = np.random.RandomState(12)
    figures = []
    for it in range(3):
        d = rng.uniform(-1, 1, eng.n)
        d /= np.linalg.norm(d)
        want = _directional_second_difference(fun, x, d, 1e-3)
        scale = max(1.0, abs(want))
        figures.append((abs(float(d @ H @ d) - want) / scale, abs(float(d @ H_ref @ d) - want) / scale))
        print("direction %d: differences %.12g, device off by %.3g, helper off by %.3g (relative)" % ((it, want) + figures[-1]))
    eng.close()
    tol = 8 * max(f[1] for f in figures)
    assert all(f[0] <= tol for f in figures), (figures, tol)
