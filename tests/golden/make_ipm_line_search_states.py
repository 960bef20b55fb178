"""Start states of the line-search tests (tests/test_ipm_line_search.py, tests/test_ipm_line_search_reference.py) ->
tests/golden/ipm/line_search_states.npz.  Outputs of this repository's own CPU restatement (oracle/ipm_oracle.py), like the other
fixtures of row f-2.

What it holds
  * iterates (v, lambda, zL, zU, mu) of oracle solves of launch(2, 5), exact Hessian, mu_strategy monotone, started from
    problems.seeded_iterate(start, xl, xu, seed) with seeds 40 and 41, at the start of the iterations STATES names, each with what
    the line search of that iteration did there (the filter it met, its bounds, every trial point's step length, verdict, theta and
    phi): the material of the CPU test of the reference;
  * for every scenario of the device tests (SCENARIOS) what the oracle does when such an iterate is injected again as iteration 0
    the way the device test injects it — the warm start of rpm_ipm_solve_warm with every push at 1e-12 and mu_init = the recorded
    mu, restated in reinject() — with the filter and the options of the scenario: the sequence of trial points it predicts;
  * one constructed state (uncorrected_step_length_*), for the rule that the switching condition (19) and the Armijo test (20) of a
    CORRECTED trial point use the step length of the uncorrected step (A-5.8).  No iterate of these solves, injected again at any
    mu, has a correction whose verdict depends on which of the two step lengths is used (they differ by 3 % where they differ at all).
    So iterate (40, 85) — theta <= theta_min, alpha 0.1228, alpha_soc 0.1266 — is moved along a fixed random direction, x (1 + eps d),
    which raises theta and leaves the step alone, until the step length at which (19) switches, theta^s_theta / (-dphi)^s_phi, lies
    midway between alpha and alpha_soc.  With a filter entry equal to the first trial point (which the test takes from the device)
    the correction opens and is accepted: by (18), armijo 0, with alpha in (19); by (20), armijo 1, were alpha_soc used.
  * the converged points of quadrotor(2, 4) with the instance bounds of the device tests, and what the oracle does (mu_strategy
    monotone, the dominating filter entry) when they are injected again: with tol = 1e-12 it gives up at the acceptable level
    (quadrotor_acceptable_*); with QUADROTOR_LAMBDA in the place of the multipliers and tol = 1e-4 it gives up at a feasible point
    whose multipliers are off, recalc_y, after up to three corrections (quadrotor_recalc_*).
Every decision of every predicted sequence is at least 1e-6 (relative) away from equality, checked here with the reference
functions of tests/_ipm_pass_reference.py on the oracle's own theta and phi.

Run from the repo root:  python tests/golden/make_ipm_line_search_states.py        (about a minute of dense linear algebra)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import _ipm_pass_reference as ref  # noqa: E402
from lpopc_amd import problems  # noqa: E402
from lpopc_amd.problem import Options  # noqa: E402

PATH = os.path.join(HERE, "ipm", "line_search_states.npz")
PUSH = 1e-12                       # every warm_start_* push of the injection
STATES = [(40, 0), (41, 0), (41, 11), (40, 63), (40, 80), (41, 98), (40, 85), (41, 79), (41, 80)]      # (seed, iteration)
DOMINATING = [(0.0, -1e300)]       # a filter entry that takes no trial point
# name -> (state, filter injected with it, options beside mu_strategy monotone, mu_init = the state's mu)
SCENARIOS = {
    "correction_accepted": ((41, 11), [], {}),
    "correction_accepted_b": ((40, 80), [], {}),
    # (injected again, (40, 63) takes the full step by (18) without a correction, and (41, 98) comes within 5e-7 of equality in (18))
    "armijo": ((40, 85), [], {}),
    "armijo_b": ((41, 79), [], {}),
    "armijo_c": ((41, 80), [], {}),
    "dominated_alpha_min": ((41, 11), DOMINATING, {}),
    "dominated_max_ls": ((41, 11), DOMINATING, {"max_ls": 3}),
}
MARGIN = 1e-6
QUADROTOR_TOL = {"acceptable": 1e-12, "recalc": 1e-4}


def quadrotor_lambda(m):
    """the multipliers of the recalc_y scenario: those tests/test_ipm_warm_start.py::_start_case draws for B = 3"""
    return np.random.RandomState(21).standard_normal((3, m)) * 3.0
EV = 64                            # room for the events of one line search


def exact():
    o = Options()
    o.SetStringValue("hessian-approximation", "exact")
    return o


def reinject(orc, x, lam, zLx, zUx, push=PUSH, relax=1e-8, mult_max=1e6, x_l=None, x_u=None):
    """The state rpm_ipm_solve_warm starts from (include/rpm_hip.h) for x, lambda and the bound multipliers of x: relaxed bounds, x
    and the slacks g(x) pushed inside them, lambda clipped, z floored, the slacks' multipliers from lambda"""
    from oracle import ipm_oracle
    xl, xu, gl, gu = orc.bounds()
    if x_l is not None:
        xl, xu = x_l, x_u
    n = orc.n
    ineq = np.nonzero(gl != gu)[0]
    vl, vu = np.concatenate([xl, gl[ineq]]), np.concatenate([xu, gu[ineq]])
    free = vl != vu
    vl = np.where(free & (vl > -ipm_oracle.INF), vl - relax * np.maximum(1.0, np.abs(vl)), vl)
    vu = np.where(free & (vu < ipm_oracle.INF), vu + relax * np.maximum(1.0, np.abs(vu)), vu)
    lo, up = free & (vl > -ipm_oracle.INF), free & (vu < ipm_oracle.INF)
    po = {"bound_push": push, "bound_frac": push}
    xs = np.where(xl == xu, xl, ipm_oracle._push(np.asarray(x, float), vl[:n], vu[:n], po))
    s = ipm_oracle._push(orc.eval_g(xs)[ineq], vl[n:], vu[n:], po)
    lam = np.clip(lam, -mult_max, mult_max)
    zL = np.concatenate([np.maximum(zLx, push), np.maximum(-lam[ineq], push)])
    zU = np.concatenate([np.maximum(zUx, push), np.maximum(lam[ineq], push)])
    return dict(v=np.concatenate([xs, s]), lam=lam, zL=np.where(lo, zL, 0.0), zU=np.where(up, zU, 0.0))


def check_sequence(rec, o_ls, what, margin=MARGIN):
    """The oracle's line search of one iteration replayed by the reference functions on the oracle's own theta and phi: the same
    verdicts and the same bookkeeping, and no decision closer than `margin`.  -> the smallest margin"""
    o = dict(ref.OPTS, **o_ls)
    cur = {k: rec[k] for k in ("theta", "theta_min", "theta_max", "phi", "dphi")}
    S = dict(alpha=rec["alpha_max"], ls=0, accepted=0, armijo=0, soc_on=0, soc_req=0, soc_p=0, th_old_soc=0.0, use_soc=0, n_soc=0,
             enter_resto=0, status=0, theta=rec["theta"], alpha_min=rec["alpha_min"], err0=rec["err0"], n_recalc=0)
    worst = 1.0
    for kind, step, took, th, phit in rec["events"]:
        assert (kind == "soc") == bool(S["soc_on"]) and S["status"] == 0 and not S["accepted"] and not S["enter_resto"], (what, kind, S)
        if kind == "trial":
            assert step == S["alpha"], (what, step, S["alpha"])
        finite = bool(np.isfinite([th, phit]).all())
        ok, armijo, _, dec = ref.filter_accepts(o, cur, th, phit, S["alpha"], rec["filt"], finite)
        assert ok == took, (what, kind, step, dec)
        S, dec2 = ref.line_search_verdict(o, S, ok, armijo, th, finite)
        for name, _, mg in dec + dec2:
            assert mg >= margin, (what, kind, step, name, mg)
            worst = min(worst, mg)
    assert bool(S["accepted"]) == rec["accepted"] and S["ls"] == rec["ls"] and S["n_soc"] == (rec["soc"] > 0) and bool(S["armijo"]) == rec["armijo"], (what, S, rec["ls"], rec["soc"])
    if not rec["accepted"]:
        want = {"acceptable": (6, 0), "restoration": (0, 1), "recalc_y": (0, 2), "failed": (3, 0)}[rec["gave_up"]]
        assert (S["status"], S["enter_resto"]) == want, (what, S, rec["gave_up"])
    return worst


def first_trial_in_filter(orc, rec, x):
    """x with the duals and mu of the iterate `rec`, injected with its own first trial point in the filter -> (x, the oracle's record
    of that line search, the step length at which (19) switches, alpha, alpha_soc)"""
    from oracle import ipm_oracle
    n = orc.n
    o = dict(ref.OPTS)
    kw = dict(mu_strategy="monotone", mu_init=rec["mu"], max_iter=1, record_iterations=[0])
    st = reinject(orc, x, rec["lam"], rec["zL"][:n], rec["zU"][:n])
    st.update(mu=rec["mu"])
    first = ipm_oracle.solve(orc, x, start_state=st, **kw)["recorded"][0]
    st["filt"] = [first["events"][0][3:5]]
    r = ipm_oracle.solve(orc, x, start_state=st, **kw)["recorded"][0]
    assert r["mu"] == rec["mu"] and r["dphi"] < 0 and r["theta"] <= r["theta_min"]
    soc = [e for e in r["events"] if e[0] == "soc"]
    assert len(r["events"]) == 2 and len(soc) == 1 and soc[0][2], r["events"]
    return x, r, r["theta"] ** o["s_theta"] * o["delta"] / (-r["dphi"]) ** o["s_phi"], r["alpha_max"], soc[0][1]


def uncorrected_step_length_state(orc, rec, verbose=False):
    """see the module's header: -> (x, the oracle's record of the line search there with the first trial point in the filter)"""
    n = orc.n
    d = np.random.RandomState(5).standard_normal(n)

    def at(eps):
        return first_trial_in_filter(orc, rec, rec["v"][:n] * (1.0 + eps * d))

    lo, hi = 1e-10, 2.2e-10
    for _ in range(12):
        eps = np.sqrt(lo * hi)
        x, r, switch_at, a, a_soc = at(eps)
        assert a_soc > a * 1.02
        if switch_at < np.sqrt(a * a_soc):
            lo = eps
        else:
            hi = eps
    assert a * 1.005 < switch_at < a_soc / 1.005, (a, switch_at, a_soc)
    if verbose:
        print("uncorrected step length: eps %.4g theta %.4g alpha %.5g < (19) switches at %.5g < alpha_soc %.5g; armijo %d" % (eps, r["theta"], a, switch_at, a_soc, r["armijo"]))
    return x, r


def pack_events(recs):
    kind, step, took = np.zeros((len(recs), EV), dtype=np.int8), np.zeros((len(recs), EV)), np.zeros((len(recs), EV), dtype=np.int8)
    th, phit = np.zeros((len(recs), EV)), np.zeros((len(recs), EV))
    for i, r in enumerate(recs):
        assert len(r["events"]) <= EV
        for k, (kd, st, ok, t_, p_) in enumerate(r["events"]):
            kind[i, k], step[i, k], took[i, k], th[i, k], phit[i, k] = kd == "soc", st, ok, t_, p_
    return dict(kind=kind, step=step, took=took, theta=th, phi=phit, count=np.array([len(r["events"]) for r in recs], dtype=np.int32),
                ls=np.array([r["ls"] for r in recs], dtype=np.int32), soc=np.array([r["soc"] for r in recs], dtype=np.int32),
                armijo=np.array([r["armijo"] for r in recs], dtype=np.int8), accepted=np.array([r["accepted"] for r in recs], dtype=np.int8),
                gave_up=np.array([r["gave_up"] or "" for r in recs]))


def _oracles():
    from oracle.oracle import Oracle
    return Oracle(problems.launch(2, 5), exact()), Oracle(problems.quadrotor(2, 4), exact())


def _quadrotor_bounds(qo, b):
    """instance bounds of tests/test_ipm_warm_start.py::_quadrotor_bounds, B = 3"""
    ql, qu, _, _ = qo.bounds()
    fixed = np.random.RandomState(8).uniform(-0.2, 0.2, size=(3, 12))
    idx = [i * 9 for i in range(12)]
    l, u = ql.copy(), qu.copy()
    l[idx] = u[idx] = fixed[b]
    return l, u


def solves(verbose=False):
    """The iterates: what whole oracle solves visit.  Dense LAPACK rounds differently from machine to machine and a long launch
    solve then visits other iterates (tests/test_ipm.py::test_restatement_reproduces_ipm_fixture allows it an iteration either way),
    so this part of the file is reproduced bit for bit only on the machine that made it; derive() below is checked everywhere."""
    from oracle import ipm_oracle
    out = {}
    orc, qo = _oracles()
    xl, xu, _, _ = orc.bounds()
    recs = {}
    for seed in sorted({s for s, _ in STATES}):
        x0 = problems.seeded_iterate(orc.starting_point(), xl, xu, seed)
        its = [i for s, i in STATES if s == seed]
        r = ipm_oracle.solve(orc, x0, mu_strategy="monotone", record_iterations=its, max_iter=max(its) + 1)
        for rec in r["recorded"]:
            recs[(seed, rec["it"])] = rec
    assert sorted(recs) == sorted(STATES), sorted(recs)
    order = [recs[k] for k in STATES]
    out["state"] = np.array(STATES, dtype=np.int32)
    for k in ("v", "lam", "zL", "zU", "dv", "dlam"):
        out[k] = np.stack([r[k] for r in order])
    for k in ("mu", "theta_max", "theta_min", "theta", "phi", "dphi", "alpha_max", "alpha_z", "alpha_min", "err0", "delta_w", "delta_w_last"):
        out[k] = np.array([r[k] for r in order])
    nf = max(len(r["filt"]) for r in order)
    out["filt"] = np.zeros((len(order), max(nf, 1), 2))
    out["nfilt"] = np.array([len(r["filt"]) for r in order], dtype=np.int32)
    for i, r in enumerate(order):
        if r["filt"]:
            out["filt"][i, :len(r["filt"])] = np.array(r["filt"])
    for k, a in pack_events(order).items():
        out["ev_" + k] = a
    for key, r in zip(STATES, order):
        worst = check_sequence(r, {}, "state %s" % (key,), margin=1e-9)     # (what the device tests inject is held to MARGIN below)
        if verbose:
            print("state", key, "mu %.3g theta %.3g: ls %d soc %d armijo %d accepted %d, %d trial points, smallest margin %.2g"
                  % (r["mu"], r["theta"], r["ls"], r["soc"], r["armijo"], r["accepted"], len(r["events"]), worst))
    # ---- the constructed state of the A-5.8 step length
    key = (40, 85)
    out["uncorrected_step_length_x"], _ = uncorrected_step_length_state(orc, recs[key], verbose)
    out["uncorrected_step_length_state"] = np.array(STATES.index(key), dtype=np.int32)
    # ---- the converged quadrotor points
    sol = {k: [] for k in ("x", "lam", "zL", "zU")}
    for b in range(3):
        l, u = _quadrotor_bounds(qo, b)
        x0 = problems.seeded_iterate(qo.starting_point(), *qo.bounds()[:2], 40 + b)
        r = ipm_oracle.solve(qo, x0, l, u, record_iterations=list(range(200)))
        assert r["status"] == 0, r["status"]
        last = r["recorded"][-1]             # the iterate the last step started from: converged to a few digits more than tol asks
        sol["x"].append(r["x"]); sol["lam"].append(r["lambda"]); sol["zL"].append(last["zL"][:qo.n]); sol["zU"].append(last["zU"][:qo.n])
        if verbose:
            print("quadrotor instance", b, "converged in", r["iterations"], "E_0", r["kkt_error"])
    for k, a in sol.items():
        out["quadrotor_" + k] = np.stack(a)
    return out


def derive(base, verbose=False):
    """What the oracle does when the iterates of `base` (solves(), or the committed file) are injected again: one iteration each"""
    from oracle import ipm_oracle
    out = {}
    orc, qo = _oracles()
    n = orc.n
    # ---- the scenarios of the device tests
    names, srecs = sorted(SCENARIOS), []
    for name in names:
        key, filt, opts = SCENARIOS[name]
        i = STATES.index(key)
        mu = float(base["mu"][i])
        st = reinject(orc, base["v"][i][:n], base["lam"][i], base["zL"][i][:n], base["zU"][i][:n])
        st.update(mu=mu, filt=filt)
        q = ipm_oracle.solve(orc, base["v"][i][:n], mu_strategy="monotone", mu_init=mu, max_iter=1, record_iterations=[0], start_state=st, **opts)
        assert len(q["recorded"]) == 1, (name, q["status"])
        sr = q["recorded"][0]
        worst = check_sequence(sr, opts, name)
        srecs.append(sr)
        if verbose:
            print("scenario", name, key, "mu %.3g theta %.3g: ls %d soc %d armijo %d accepted %d gave up %s, %d trial points, alpha %.3g alpha_min %.3g, margin %.2g"
                  % (sr["mu"], sr["theta"], sr["ls"], sr["soc"], sr["armijo"], sr["accepted"], sr["gave_up"], len(sr["events"]), sr["alpha"], sr["alpha_min"], worst))
    out["scenario"] = np.array(names)
    out["scenario_state"] = np.array([STATES.index(SCENARIOS[k][0]) for k in names], dtype=np.int32)
    for k, a in pack_events(srecs).items():
        out["sc_" + k] = a
    # ---- the constructed state: what it was built for
    i = int(base["uncorrected_step_length_state"])
    rec = dict(v=base["v"][i], lam=base["lam"][i], zL=base["zL"][i], zU=base["zU"][i], mu=float(base["mu"][i]))
    _, ra, switch_at, a, a_soc = first_trial_in_filter(orc, rec, base["uncorrected_step_length_x"])
    assert a * 1.005 < switch_at < a_soc / 1.005, (a, switch_at, a_soc)
    cur = {k: ra[k] for k in ("theta", "theta_min", "theta_max", "phi", "dphi")}
    th_s, phi_s = ra["events"][1][3:5]
    with_alpha = ref.filter_accepts(dict(ref.OPTS), cur, th_s, phi_s, a, [])
    with_alpha_soc = ref.filter_accepts(dict(ref.OPTS), cur, th_s, phi_s, a_soc, [])
    assert with_alpha[:2] == (True, False) and with_alpha_soc[:2] == (True, True) and not ra["armijo"] and ra["soc"] == 1
    assert min(x_[2] for x_ in with_alpha[3] + with_alpha_soc[3]) >= MARGIN
    # ---- the converged quadrotor points, injected again
    qrecs = {"acceptable": [], "recalc": []}
    lam_off = quadrotor_lambda(qo.m)
    for b in range(3):
        l, u = _quadrotor_bounds(qo, b)
        x, zl, zu = base["quadrotor_x"][b], base["quadrotor_zL"][b], base["quadrotor_zU"][b]
        for name in sorted(qrecs):
            opts = dict(tol=QUADROTOR_TOL[name], mu_strategy="monotone", max_iter=1, record_iterations=[0])
            st = reinject(qo, x, base["quadrotor_lam"][b] if name == "acceptable" else lam_off[b], zl, zu, x_l=l, x_u=u)
            st.update(mu=0.1, filt=DOMINATING)
            # (the filter empties when mu changes: the second run starts at the mu the first one's barrier update ends at, as the device
            # test's filter is injected after that update)
            st["mu"] = ipm_oracle.solve(qo, x, l, u, start_state=st, **opts)["recorded"][0]["mu"]
            qr = ipm_oracle.solve(qo, x, l, u, start_state=st, **opts)["recorded"][0]
            assert qr["mu"] == st["mu"] and len(qr["filt"]) == 1
            worst = check_sequence(qr, {"tol": QUADROTOR_TOL[name]}, "quadrotor %s %d" % (name, b))
            qrecs[name].append(qr)
            if verbose:
                print("  quadrotor", b, name, "mu %.3g theta %.3g E_0 %.3g: ls %d, %d corrections tried, gave up: %s, margin %.2g"
                      % (qr["mu"], qr["theta"], qr["err0"], qr["ls"], sum(e[0] == "soc" for e in qr["events"]), qr["gave_up"], worst))
    for name, rs in qrecs.items():
        for k, a_ in pack_events(rs).items():
            out["quadrotor_%s_%s" % (name, k)] = a_
        out["quadrotor_%s_mu" % name] = np.array([r_["mu"] for r_ in rs])
    return out


def build(verbose=False):
    out = solves(verbose)
    out.update(derive(out, verbose))
    return out


if __name__ == "__main__":
    data = build(verbose=True)
    np.savez_compressed(PATH, **data)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
