"""The line-search half of the reference (tests/_ipm_pass_reference.py: trial point, theta, the barrier sum, phi, filter_accepts,
line_search_verdict, the correction's constraints, (16), (22), (33)/(34)) checked without the kernels, and the fixture of start
states (tests/golden/ipm/line_search_states.npz) against its generator.

The line search: at iterates recorded from oracle solves of launch(2, 5) the CPU oracle (oracle/ipm_oracle.py) runs the iteration
again from the recorded iterate, filter and filter bounds; the reference functions, driven here in long double with their own trial
points, corrections (a dense solve of (13) from ref.kkt_13 / ref.rhs_13) and evaluations, must take the same sequence of accepted /
corrected / halved trial points and end with the same ls, correction count and armijo flag."""
import importlib.util
import os

import numpy as np
import pytest

import _ipm_pass_reference as ref
from lpopc_amd import problems
from oracle import ipm_oracle
from oracle import oracle as orc

LD = ref.LD
HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_ipm_line_search_states", os.path.join(HERE, "golden", "make_ipm_line_search_states.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gen(built):
    return _generator()


@pytest.fixture(scope="module")
def states(gen):
    return dict(np.load(gen.PATH))


@pytest.fixture(scope="module")
def launch(gen):
    o = orc.Oracle(problems.launch(2, 5), gen.exact())
    xl, xu, gl, gu = o.bounds()
    jr, jc = ref.zero_based(*o.jac_structure(), o.m, o.n)
    hr, hc = ref.zero_based(*o.hess_structure(), o.n, o.n)
    lay = ref.Layout(o.n, o.m, gl, gu, jr, jc, hr, hc)
    vl, vu = np.concatenate([xl, gl[lay.srow]]), np.concatenate([xu, gu[lay.srow]])
    free = vl != vu
    vl = np.where(free & (vl > -ref.INF), vl - 1e-8 * np.maximum(1.0, np.abs(vl)), vl)       # bound_relax_factor
    vu = np.where(free & (vu < ref.INF), vu + 1e-8 * np.maximum(1.0, np.abs(vu)), vu)
    return o, lay, vl, vu, gl


def test_generator_reproduces_the_fixture(gen, states):
    """From the committed iterates the generator derives again what the file holds beside them — the sequence of trial points the
    oracle takes from every injected state: verdicts and counts exactly, step lengths, theta and phi to 1e-6 — and its checks of
    them hold (every decision 1e-6 from equality, the constructed state between the two step lengths).  The iterates themselves
    come from whole solves, which LAPACK's rounding takes another way on another machine (gen.solves)."""
    fresh = gen.derive(states)
    assert set(fresh) < set(states)
    for k in sorted(fresh):
        a, b = np.asarray(fresh[k]), states[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":
            assert np.allclose(a, b, rtol=1e-6, atol=0.0), k
        else:
            assert np.array_equal(a, b), k


def _reference_line_search(launch, z, i):
    """the line search of recorded iterate i by the reference functions -> (events [(is_soc, step, accepted)], final state)"""
    o_, lay, vl, vu, gl = launch
    o = dict(ref.OPTS, mu_strategy=0)
    n, nv = lay.n, lay.nv
    v, lam, zL, zU, mu = z["v"][i], z["lam"][i], z["zL"][i], z["zU"][i], z["mu"][i]
    x = v[:n]
    f, grad, g, jac, hess = o_.eval_f(x), o_.eval_grad_f(x), o_.eval_g(x), o_.eval_jac_g(x), o_.eval_h(x, 1.0, lam)
    c, _ = ref.constraints(lay, v, g, gl)
    glag, _, _ = ref.grad_lagrangian(lay, grad, jac, lam)
    sca, _, _ = ref.residual_scalars(lay, v, vl, vu, zL, zU, lam, c, glag)
    theta, theta_min = sca["theta"], LD(z["theta_min"][i])
    phi, _ = ref.barrier_objective(f, mu, sca["lnsum"])
    tau = max(o["tau_min"], 1.0 - mu)
    K, _, _ = ref.kkt_13(lay, v, vl, vu, zL, zU, jac, hess, z["delta_w"][i], o["delta_c"])
    K64 = K.astype(np.float64)

    def solve(rhs):
        s = np.linalg.solve(K64, np.asarray(rhs, dtype=np.float64))
        for _ in range(2):                      # refined against the long-double matrix
            s = s + np.linalg.solve(K64, (LD(rhs) - K @ LD(s)).astype(np.float64))
        return s

    rhs, _ = ref.rhs_13(lay, v, vl, vu, glag, c, mu)
    sol = solve(rhs)
    dv = sol[:nv]
    q = ref.step_quantities(lay, o, v, vl, vu, zL, zU, grad, dv, mu, tau, theta, theta_min)
    cur = dict(theta=theta, theta_min=theta_min, theta_max=LD(z["theta_max"][i]), phi=phi, dphi=q["dphi"])
    S = dict(alpha=q["alpha_max"], ls=0, accepted=0, armijo=0, soc_on=0, soc_req=0, soc_p=0, th_old_soc=LD(0), use_soc=0, n_soc=0, enter_resto=0,
             status=0, theta=theta, alpha_min=ref.alpha_min_23(o, theta, theta_min, q["dphi"]), err0=z["err0"][i], n_recalc=0)
    filt = [tuple(e) for e in z["filt"][i][:z["nfilt"][i]]]
    events, csoc, ct, dv2, a_soc = [], None, None, None, None
    for _ in range(o["max_ls"] + o["max_soc"] + 3):
        if S["accepted"] or S["status"] or S["enter_resto"]:
            break
        if S["soc_req"]:
            csoc, _ = ref.correction_constraints(c if S["soc_p"] == 0 else csoc, ct, S["alpha"] if S["soc_p"] == 0 else a_soc)
            r2, _ = ref.rhs_13(lay, v, vl, vu, glag, csoc, mu)
            dv2 = solve(r2)[:nv]
            a_soc = ref.step_quantities(lay, o, v, vl, vu, zL, zU, grad, dv2, mu, tau, theta, theta_min)["alpha_max"]
            S["soc_req"] = 0
        step, d = (a_soc, dv2) if S["soc_on"] else (S["alpha"], dv)
        vt, vt_mag = ref.trial_point(v, vl, vu, d, step)
        xt = vt[:n].astype(np.float64)
        with np.errstate(all="ignore"):
            ft, gt = o_.eval_f(xt), o_.eval_g(xt)
            ct, _ = ref.trial_constraints(lay, vt, vt_mag, gt, gl)
            th, _, _ = ref.theta_1(ct)
            ln, _, _ = ref.barrier_log_sum(vt, vl, vu)
            phit, _ = ref.barrier_objective(ft, mu, ln)
        finite = bool(np.isfinite(np.array([ft, th, phit], dtype=np.float64)).all())
        ok, armijo, _, _ = ref.filter_accepts(o, cur, th, phit, S["alpha"], filt, finite)
        events.append((bool(S["soc_on"]), float(step), ok))
        S, _ = ref.line_search_verdict(o, S, ok, armijo, th, finite)
    return events, S


@pytest.mark.parametrize("which", [(40, 0), (41, 11), (40, 80), (40, 85), (41, 79)], ids=lambda w: "seed%d_it%d" % w)
def test_reference_line_search_follows_the_oracle(gen, states, launch, which):
    z = states
    i = [tuple(s) for s in z["state"]].index(which)
    o_ = launch[0]
    st = dict(v=z["v"][i], lam=z["lam"][i], zL=z["zL"][i], zU=z["zU"][i], mu=z["mu"][i], filt=[tuple(e) for e in z["filt"][i][:z["nfilt"][i]]],
              theta_max=z["theta_max"][i], theta_min=z["theta_min"][i], delta_w_last=z["delta_w_last"][i])
    r = ipm_oracle.solve(o_, z["v"][i][:o_.n], mu_strategy="monotone", mu_init=z["mu"][i], max_iter=1, record_iterations=[0], start_state=st)
    rec = r["recorded"][0]
    # the oracle, started again from the recorded iterate, does what it did in the recorded solve (the fixture holds that)
    k = z["ev_count"][i]
    assert len(rec["events"]) == k and [e[0] == "soc" for e in rec["events"]] == list(z["ev_kind"][i][:k] != 0)
    assert [e[2] for e in rec["events"]] == list(z["ev_took"][i][:k] != 0)
    assert (rec["ls"], rec["soc"], rec["armijo"]) == (z["ev_ls"][i], z["ev_soc"][i], bool(z["ev_armijo"][i]))
    events, S = _reference_line_search(launch, z, i)
    assert [(e[0], e[2]) for e in events] == [(e[0] == "soc", e[2]) for e in rec["events"]], (events, rec["events"])
    for mine, theirs in zip(events, rec["events"]):      # (the step lengths come from two solves of an ill-conditioned (13): a loose figure)
        assert abs(mine[1] - theirs[1]) <= 1e-6 * theirs[1], (mine, theirs)
    assert S["ls"] == rec["ls"] and bool(S["armijo"]) == rec["armijo"] and bool(S["accepted"]) == rec["accepted"]
    assert S["n_soc"] == (1 if rec["soc"] else 0) and (S["soc_p"] + 1 if S["use_soc"] else 0) == rec["soc"]
    print(which, "events", events, "ls", S["ls"], "soc", rec["soc"], "armijo", S["armijo"])


def test_scenarios_cover_the_branches(states):
    """what the device tests rely on: every branch of the line search has a scenario whose predicted sequence takes it"""
    z = states
    sc = {str(nm): k for k, nm in enumerate(z["scenario"])}
    k = sc["correction_accepted"]
    assert (z["sc_ls"][k], z["sc_soc"][k], z["sc_accepted"][k]) == (0, 1, 1)
    k = sc["armijo"]
    assert (z["sc_ls"][k], z["sc_soc"][k], z["sc_armijo"][k], z["sc_accepted"][k]) == (0, 0, 1, 1)
    k = sc["dominated_alpha_min"]
    assert z["sc_accepted"][k] == 0 and str(z["sc_gave_up"][k]) == "restoration" and z["sc_ls"][k] == 25 and z["sc_kind"][k][:z["sc_count"][k]].sum() == 1
    k = sc["dominated_max_ls"]
    assert z["sc_accepted"][k] == 0 and str(z["sc_gave_up"][k]) == "restoration" and z["sc_ls"][k] == 4
    for i in (0, 1):                      # the cold starts: one correction that is dropped, then three halvings
        n_ev = z["ev_count"][i]
        assert list(z["ev_kind"][i][:n_ev]) == [0, 1, 0, 0, 0] and list(z["ev_took"][i][:n_ev]) == [0, 0, 0, 0, 1] and z["ev_ls"][i] == 3


def test_restoration_start_satisfies_its_equations(states):
    """(33), (34): p - n = c and the stationarity of rho (p + n) - mu_R (log p + log n) on p - n = c, 2 rho = mu_R / p + mu_R / n, to
    1e-15 relative; over constraint values of both signs and twelve orders of magnitude"""
    o = ref.OPTS
    rng = np.random.RandomState(3)
    c = np.concatenate([rng.standard_normal(400) * 10.0 ** rng.uniform(-9, 3, 400), [0.0, 1e-300, -1e-300, 31.9, -31.9]])
    for mu in (0.1, 1e-9, 50.0):
        cinf = float(np.abs(c).max())
        r = ref.restoration_start(o, c, mu, cinf, np.array([0.5, -3.0, 0.0]))
        assert r["mu_r"] == max(mu, cinf) and (r["pp"] > 0).all() and (r["nn"] > 0).all()
        rho, mu_r = LD(o["resto_rho"]), r["mu_r"]
        e1 = np.abs(r["pp"] - r["nn"] - LD(c)) / np.maximum(np.abs(LD(c)), r["pp"])
        e2 = np.abs(2 * rho - mu_r / r["pp"] - mu_r / r["nn"]) / (2 * rho)
        assert e1.max() <= 1e-15 and e2.max() <= 1e-15, (mu, float(e1.max()), float(e2.max()))
        assert np.array_equal(r["zp"], mu_r / r["pp"]) and np.array_equal(r["zn"], mu_r / r["nn"])
        assert np.allclose(r["dr2"].astype(np.float64), [1.0, 1.0 / 9.0, 1.0], rtol=1e-15)


def test_reset_16_and_filter_entry():
    """(16) keeps z inside [mu / (kappa s), kappa mu / s] and leaves it alone there; (22) by its definition"""
    o = ref.OPTS
    s = LD(np.array([1e-8, 1.0, 1e3, 2.0]))
    mu = LD(1e-3)
    z = LD(np.array([1e30, 1e-3, 1e-30, 5.0]))
    r = ref.reset_16(o, z, s, mu)
    ks = LD(o["kappa_sigma"])
    assert r[0] == ks * mu / s[0] and r[1] == z[1] and r[2] == mu / (ks * s[2]) and r[3] == z[3]
    (ft, fp), _ = ref.filter_entry_22(o, 31.9, -0.25)
    assert abs(ft - LD(31.9) * (1 - LD(1e-5))) <= 1e-18 * 31.9 and abs(fp - (LD(-0.25) - LD(1e-8) * LD(31.9))) <= 1e-18
