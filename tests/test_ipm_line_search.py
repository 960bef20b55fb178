"""The second half of an interior-point iteration on injected states — the filter line search with its second-order corrections
and the update (ipm_trial_kernel, ipm_accept_kernel, ipm_soc_rhs_kernel, ipm_soc_direction_kernel, ipm_update_kernel,
ipm_launch_jt_lambda_into) — through rpm_ipm_debug_line_search and rpm_ipm_debug_update, which run the solve loop's own
IpmLoop::line_search_round and IpmLoop::update after rpm_ipm_debug_pass(stage 3), against the long-double reference of
tests/_ipm_pass_reference.py.  tests/test_ipm_pass.py checks the first half the same way; its rule of comparison holds unchanged:
  a single expression or a maximum     |dev - ref| <= 8 * 2^-52 * M,               M = sum of the magnitudes of its operands
  a sum of k terms                     |dev - ref| <= (k + 8) * 2^-52 * sum |term|
and bit equality where the code is a copy or one IEEE operation.  The operands of every check are the DEVICE's results of the
step before.  The record holds theta and phi of the trial point, not its sum of logarithms: phi = f - mu ln is held to the single
rule of |f| + |mu ln| plus mu times the sum rule of ln over its terms.

The line search runs one round per hook call.  After every round, for every instance: the trial point, c there, theta, phi; the
correction a round computed (c_soc, its right-hand side, the step lengths of the corrected step); then every decision — dominance
from the filter that was injected, filter_accepts, and the branch after it — replayed in double from the device's own theta, phi and
record, which must give exactly the record the device left (and the counts the host read); and on the reference's theta and phi no
decision may be closer than 1e-9 to equality.

States: the cold starts of quadrotor(2, 4), bryson_denham(2, 8), launch(2, 5) and launch(16, 8); iterates of the CPU oracle on
launch(2, 5) and converged points of the quadrotor (tests/golden/ipm/line_search_states.npz, with the sequence of trial points the
oracle predicts for each: the device must take the same), injected through the warm start with every push at 1e-12."""
import os

import numpy as np
import pytest

import _ipm_pass_reference as ref
import test_ipm_pass as tp
import test_ipm_warm_start as ws
from lpopc_amd.engine import RpmError

LD = ref.LD
STATES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ipm", "line_search_states.npz")
PUSHES = {k: 1e-12 for k in tp.TIGHT}
DOMINATING = [(0.0, -1e300)]
# names of rpm_ipm_set_option -> the reference's
OPTION_NAMES = {"max_line_search": "max_ls", "max_soc": "max_soc", "restoration": "resto", "restoration_penalty": "resto_rho"}
N_FILTER = 4


class Case(tp.Case):
    def set(self, **opts):
        super().set(**opts)
        for k, v in opts.items():
            if k in OPTION_NAMES:
                self.o[OPTION_NAMES[k]] = v

    def plain_bounds(self):
        """the bounds without the two opened ones of instance 0: the problem the oracle's iterates belong to"""
        if self.name.startswith("quadrotor"):
            self.XL, self.XU, _ = ws._quadrotor_bounds(self.eng, self.B)
        else:
            xl, xu, _, _ = self.eng.get_bounds_info()
            self.XL, self.XU = np.tile(xl, (self.B, 1)), np.tile(xu, (self.B, 1))
        self.ipm.set_all_bounds(self.XL, self.XU)

    def start(self, X0=None, lam=None, z=None, warm=True):
        if warm:
            return super().start(X0, lam, z)
        X0 = self.X0 if X0 is None else X0
        st = self.ipm.debug_start(X0, warm=False)
        want = ws._reference_start(self.one, self.XL, self.XU, X0, None, None, dict(ws.DEFAULTS, **self.opts), warm=False)
        st["vl"], st["vu"], st["sc"], st["sf"] = want["vl"], want["vu"], want["sc"], want["sf"]
        return st


def _record(inst, b):
    return {k: float(a[b]) for k, a in inst.items()}


def _int_fields(R):
    for k in ("ls", "accepted", "armijo", "soc_on", "soc_req", "soc_p", "use_soc", "n_soc", "enter_resto", "status", "n_recalc", "nfilt"):
        R[k] = int(R[k])
    return R


def _pending(R):
    """its line search goes on: running, no trial point taken yet and not given up"""
    return R["status"] == 0 and not R["accepted"] and not R["enter_resto"]


class Search:
    """one stage-3 pass of a case, then the line search round by round with every check of the module's header, then the update"""

    def __init__(self, case, st, filt=None, edge_rounds=0):
        """edge_rounds: in that many first rounds the injected filter holds the device's own theta and phi of the trial point, bit for
        bit — a comparison at equality on purpose, decided by the device's bits alone: the reference's verdict, which sees the same
        numbers a rounding apart, is not asked there"""
        self.case, self.st, self.edge_rounds = case, st, edge_rounds
        self.B = case.B
        self.p3 = case.ipm.debug_pass(3)
        self.filt = [list(f) for f in filt] if filt is not None else [[] for _ in range(self.B)]
        self.inject = filt
        self.R = [_int_fields(_record(self.p3["inst"], b)) for b in range(self.B)]
        self.first = [dict(r) for r in self.R]
        self.events = [[] for _ in range(self.B)]            # (corrected, step length, accepted) per trial point
        self.last = None
        self.rounds = 0
        self.min_margin = 1.0
        self.corrections = self.max_soc_p = 0

    # ---- one round
    def round(self):
        case = self.case
        ls = case.ipm.debug_line_search(1, self.inject if self.rounds == 0 else None)
        want2 = want3 = 0
        for b in range(self.B):
            R0 = self.R[b]
            if self.rounds == 0:
                assert R0["nfilt"] == 0
                R0["nfilt"] = len(self.filt[b])
            R1 = _int_fields(_record(ls["inst"], b))
            if not _pending(R0):
                changed = {k for k in R0 if not (R0[k] == R1[k] or (R0[k] != R0[k] and R1[k] != R1[k]))}
                assert not changed, (case.name, b, "an instance whose line search is over changed", changed)
                if self.last is not None:
                    for k in ("xt", "ct", "csoc", "dv2", "dlam2", "dzL2", "dzU2"):
                        assert np.array_equal(ls[k][b].view(np.uint64), self.last[k][b].view(np.uint64)), (case.name, b, k)
                continue
            S1 = self._check_instance(b, R0, R1, ls)
            want2 += int(S1["status"] == 0 and not S1["accepted"] and not S1["enter_resto"] and not S1["soc_req"])
            want3 += int(S1["soc_req"])
            self.R[b] = R1
        assert ls["counts"] == (want2, want3), (case.name, self.rounds, ls["counts"], want2, want3)
        self.last = ls
        self.rounds += 1
        return ls["counts"] == (0, 0)

    def _check_instance(self, b, R0, R1, ls):
        case, st, p3 = self.case, self.st, self.p3
        lay, o, r = case.lay, case.o, case.rows(st, b)
        n, nv = lay.n, lay.nv
        tag = "%s instance %d round %d" % (case.name, b, self.rounds)
        free, lo, up = ref.bound_kinds(r["vl"], r["vu"])
        v, mu = r["v"], R0["mu"]
        soc = bool(R0["soc_on"])
        # ---- the correction this round computed (A-5.5 / A-5.9, A-5.6)
        if R0["soc_req"]:
            self.corrections += 1
            self.max_soc_p = max(self.max_soc_p, R0["soc_p"])
            first = R0["soc_p"] == 0
            c_prev, mix = (p3["c"][b], R0["alpha"]) if first else (self.last["csoc"][b], R0["alpha_soc"])
            cs, cs_mag = ref.correction_constraints(c_prev, self.last["ct"][b], mix)
            tp._close(ls["csoc"][b], cs, ref.single_tol(cs_mag), tag + " c_soc")
            rhs, rmag = ref.rhs_13(lay, v, r["vl"], r["vu"], p3["glag"][b], ls["csoc"][b], mu)
            assert np.array_equal(ls["soc_rhs"][b][nv:], -ls["csoc"][b]), tag + " right-hand side at the multipliers"
            tp._close(ls["soc_rhs"][b][:nv], rhs[:nv], ref.single_tol(rmag[:nv]), tag + " right-hand side at the unknowns")
            dv2 = ls["dv2"][b]
            assert (dv2[~free] == 0.0).all() and np.array_equal(dv2[free], ls["rhs"][b][:nv][free]), tag + " dv2: a copy"
            assert np.array_equal(ls["dlam2"][b], ls["rhs"][b][nv:]), tag + " dlam2: a copy"
            q = ref.step_quantities(lay, o, v, r["vl"], r["vu"], r["zL"], r["zU"], p3["grad"][b], dv2, mu, R0["tau"], R0["theta"], R0["theta_min"],
                                    dz_for_alpha=(ls["dzL2"][b], ls["dzU2"][b]))
            tp._close(ls["dzL2"][b], q["dzL"], ref.single_tol(q["dzL_mag"]), tag + " dzL2")
            tp._close(ls["dzU2"][b], q["dzU"], ref.single_tol(q["dzU_mag"]), tag + " dzU2")
            assert (ls["dzL2"][b][~lo] == 0.0).all() and (ls["dzU2"][b][~up] == 0.0).all(), tag
            tp._close(R1["alpha_soc"], q["alpha_max"], ref.single_tol(abs(q["alpha_max"])), tag + " alpha_soc")
            tp._close(R1["az_soc"], q["alpha_z"], ref.single_tol(abs(q["alpha_z"])), tag + " az_soc")
            assert np.isfinite(dv2).all()
        else:
            assert R1["alpha_soc"] == R0["alpha_soc"] and R1["az_soc"] == R0["az_soc"], tag
        step, d = (R1["alpha_soc"], ls["dv2"][b]) if soc else (R0["alpha"], p3["dv"][b])
        # ---- the trial point and c there
        vt_ref, vt_mag = ref.trial_point(v, r["vl"], r["vu"], d, step)
        tp._close(ls["xt"][b], vt_ref[:n], ref.single_tol(vt_mag[:n]), tag + " xt")
        assert np.array_equal(ls["xt"][b][~free[:n]], v[:n][~free[:n]]), tag + " xt at fixed variables"
        vt = np.concatenate([ls["xt"][b], v[n:] + step * d[n:]])          # (the slacks' trial values: the same two IEEE operations)
        gt, ft = ls["gt"][b], ls["objt"][b]
        ct_ref, ct_mag = ref.trial_constraints(lay, vt, vt_mag, gt, r["gl_rows"])
        tp._close(ls["ct"][b], ct_ref, ref.single_tol(ct_mag), tag + " ct")
        if not case.opts.get("nlp_scaling"):
            plain = np.ones(lay.m, dtype=bool)
            plain[lay.srow] = False
            assert np.array_equal(ls["ct"][b][plain], (gt - case.gl)[plain]), tag + " ct bits"
        else:
            assert np.array_equal(gt, case.one.eval_g(ls["xt"][b]) * r["sc"]) and ft == case.one.eval_f(ls["xt"][b]) * r["sf"], tag + " scaled evaluation"
        th_dev, phi_dev = R1["th_trial"], R1["phi_trial"]
        th_ref, th_mag, th_cnt = ref.theta_1(ls["ct"][b])
        tp._close(th_dev, th_ref, ref.sum_tol(th_cnt, th_mag), tag + " theta of the trial point")
        with np.errstate(all="ignore"):
            ln_ref, ln_mag, ln_cnt = ref.barrier_log_sum(vt, r["vl"], r["vu"])
        finite = bool(np.isfinite(np.array([ft, float(th_ref), float(ln_ref)])).all())
        assert finite, tag             # (no state of this module leaves the domain of the logarithms)
        phi_ref, phi_mag = ref.barrier_objective(ft, mu, ln_ref)
        tp._close(phi_dev, phi_ref, ref.single_tol(phi_mag) + mu * ref.sum_tol(ln_cnt, ln_mag), tag + " phi of the trial point")
        # ---- the decisions: on the reference none is close ...
        S0 = {k: R0[k] for k in ref.LS_STATE + ("theta", "alpha_min", "err0", "n_recalc")}
        S0["soc_req"] = 0
        cur = {k: R0[k] for k in ("theta", "theta_min", "theta_max", "phi", "dphi")}
        edge = self.rounds < self.edge_rounds
        ok_r, arm_r, dom_r, dec = ref.filter_accepts(o, {k: LD(x) for k, x in cur.items()}, th_ref, phi_ref, LD(R0["alpha"]), self.filt[b])
        S_r, dec2 = ref.line_search_verdict(o, dict(S0), ok_r, arm_r, th_ref)
        if not edge:
            tight = [x for x in dec + dec2 if x[2] <= 1e-9]
            assert not tight, (tag, tight)
            self.min_margin = min([self.min_margin] + [x[2] for x in dec + dec2])
        # ... and replayed in double from the device's own theta and phi they give what the device left
        dominated = any(th_dev >= ft_ and phi_dev >= fp_ for ft_, fp_ in self.filt[b])
        ok, arm, dom, _ = ref.filter_accepts(o, cur, th_dev, phi_dev, R0["alpha"], self.filt[b])
        assert dom == dominated, tag
        assert edge or (dom == dom_r and ok == ok_r and arm == arm_r), (tag, dom, dom_r, ok, ok_r)
        S1, _ = ref.line_search_verdict(o, dict(S0), ok, arm, th_dev)
        got = {k: R1[k] for k in ref.LS_STATE}
        assert got == {k: S1[k] for k in ref.LS_STATE}, (tag, got, {k: S1[k] for k in ref.LS_STATE})
        if S1["ls"] == R0["ls"] + 1:
            assert R1["alpha"] == 0.5 * R0["alpha"], tag
        unchanged = [k for k in R0 if k not in ref.LS_STATE + ("alpha_soc", "az_soc", "th_trial", "phi_trial", "nfilt") and R0[k] != R1[k] and R0[k] == R0[k]]
        assert not unchanged and R1["nfilt"] == len(self.filt[b]), (tag, unchanged)
        self.events[b].append((soc, step, bool(ok)))
        return S1

    def run(self, limit=None):
        limit = limit or self.case.o["max_ls"] + self.case.o["max_soc"] + 3
        for _ in range(limit):
            if self.round():
                break
        else:
            raise AssertionError("%s: the line search did not end in %d rounds" % (self.case.name, limit))
        return self

    def follows(self, b, kinds, took):
        """the sequence of trial points the oracle predicts"""
        got = self.events[b]
        assert [e[0] for e in got] == [bool(k) for k in kinds] and [e[2] for e in got] == [bool(k) for k in took], (self.case.name, b, got, list(kinds), list(took))

    # ---- the update
    def update(self):
        case, st, p3 = self.case, self.st, self.p3
        lay, o = case.lay, case.o
        n, nv, m = lay.n, lay.nv, lay.m
        up = case.ipm.debug_update(N_FILTER)
        for b in range(self.B):
            R, U = self.R[b], _int_fields(_record(up["inst"], b))
            r = case.rows(st, b)
            tag = "%s instance %d update" % (case.name, b)
            free, lo, upb = ref.bound_kinds(r["vl"], r["vu"])
            moved = {k for k in R if R[k] != U[k] and R[k] == R[k]}
            same = lambda *keys: all(np.array_equal(up[k][b], {"v": r["v"], "zL": r["zL"], "zU": r["zU"], "lambda": r["lam"]}[k]) for k in keys)
            nf0 = len(self.filt[b])
            kept = np.array(self.filt[b], dtype=np.float64).reshape(nf0, 2)
            assert np.array_equal(up["filter"][b][:nf0], kept), tag + " the filter's earlier entries"
            entry, emag = ref.filter_entry_22(o, R["theta"], R["phi"])
            trace = case.ipm.trace(b)
            if R["status"] != 0:
                assert not moved and same("v", "zL", "zU") and len(trace) == 0, (tag, moved)
                continue
            if R["enter_resto"] == 2:                    # recalc_y: the next pass computes least-squares multipliers, nothing else moves
                assert moved == {"mode", "enter_resto", "skip_update"} and (U["mode"], U["enter_resto"], U["skip_update"]) == (3, 0, -1), (tag, moved)
                assert same("v", "zL", "zU", "lambda") and len(trace) == 0, tag
                continue
            if R["enter_resto"] == 1:                    # the restoration phase starts from this point
                rs = ref.restoration_start(o, p3["c"][b], R["mu"], R["cinf"], r["v"])
                assert same("v") and np.array_equal(up["vR"][b], r["v"]), tag + " v_R"
                tp._close(up["dr2"][b], rs["dr2"], ref.single_tol(rs["dr2"].astype(np.float64)), tag + " D_R^2")
                rho = o["resto_rho"]
                assert np.array_equal(up["zL"][b], np.minimum(rho, r["zL"])) and np.array_equal(up["zU"][b], np.minimum(rho, r["zU"])), tag + " z clipped"
                tp._close(up["nn"][b], rs["nn"], ref.single_tol(rs["nn_mag"]), tag + " n (33)")
                tp._close(up["pp"][b], rs["pp"], ref.single_tol(rs["pp_mag"]), tag + " p (34)")
                assert U["mu_r"] == max(R["mu"], R["cinf"]), tag
                tp._close(up["zp"][b], LD(U["mu_r"]) / LD(up["pp"][b]), ref.single_tol(np.abs(up["zp"][b])), tag + " z_p")
                tp._close(up["zn"][b], LD(U["mu_r"]) / LD(up["nn"][b]), ref.single_tol(np.abs(up["zn"][b])), tag + " z_n")
                assert (up["lambda"][b] == 0.0).all(), tag
                tp._close(U["zeta"], np.sqrt(LD(U["mu_r"])), ref.single_tol(U["zeta"]), tag + " zeta")
                assert (U["th0"], U["mode"], U["resto_it"], U["nrfilt"], U["enter_resto"]) == (R["theta"], 2, 0, 0, 0), tag
                assert moved <= {"mode", "enter_resto", "mu_r", "zeta", "th0", "nfilt", "resto_it", "nrfilt"}, (tag, moved)
                assert U["nfilt"] == nf0 + 1 and U["iter"] == 0 and len(trace) == 0, tag
                tp._close(up["filter"][b][nf0], np.array(entry), ref.single_tol(np.array(emag)), tag + " filter entry (22)")
                continue
            assert R["accepted"], tag
            corrected = bool(R["use_soc"])
            a, az = (R["alpha_soc"], R["az_soc"]) if corrected else (R["alpha"], R["alpha_z"])
            src = self.last if corrected else p3
            d, dl, dzl, dzu = (src[k + ("2" if corrected else "")][b] for k in ("dv", "dlam", "dzL", "dzU"))
            v_ref, v_mag = ref.trial_point(r["v"], r["vl"], r["vu"], d, a)
            tp._close(up["v"][b], v_ref, ref.single_tol(v_mag), tag + " v")
            assert np.array_equal(up["v"][b][:n], self.last["xt"][b]), tag + " v is the accepted trial point"
            q = ref.apply_step(o, r["vl"], r["vu"], up["v"][b], r["zL"], r["zU"], r["lam"], dl, dzl, dzu, a, az, R["mu"])
            tp._close(up["lambda"][b], q["lam"], ref.single_tol(q["lam_mag"]), tag + " lambda")
            tp._close(up["zL"][b][lo], q["zL"][lo], ref.single_tol(q["zL_mag"][lo]), tag + " zL (16)")
            tp._close(up["zU"][b][upb], q["zU"][upb], ref.single_tol(q["zU_mag"][upb]), tag + " zU (16)")
            for k, src0 in (("v", r["v"]), ("zL", r["zL"]), ("zU", r["zU"])):
                assert np.array_equal(up[k][b][~free], src0[~free]), tag + " fixed unknowns of " + k
            assert np.array_equal(up["zL"][b][~lo], r["zL"][~lo]) and np.array_equal(up["zU"][b][~upb], r["zU"][~upb]), tag
            if R["armijo"]:                              # (22): no filter entry after a step taken by the Armijo test
                assert U["nfilt"] == nf0 and moved == {"iter"}, (tag, moved, U["nfilt"])
            else:
                assert U["nfilt"] == nf0 + 1 and moved == {"iter", "nfilt"}, (tag, moved, U["nfilt"])
                tp._close(up["filter"][b][nf0], np.array(entry), ref.single_tol(np.array(emag)), tag + " filter entry (22)")
            assert U["iter"] == 1 and trace.shape == (1, 8), tag
            row = np.array([R["f"], R["theta"], R["mu"], a, az, R["delta_w"], R["err0"], float(R["ls"])])
            assert np.array_equal(trace[0].view(np.uint64), row.view(np.uint64)), (tag, trace[0], row)
            if case.hessian != "exact":
                gl_ref, gl_mag, gl_cnt = ref.grad_lagrangian(lay, p3["grad"][b], p3["jac"][b], up["lambda"][b])
                tp._close(up["lb_gold"][b], gl_ref[:n], ref.sum_tol(gl_cnt[:n], gl_mag[:n]), tag + " grad_x L(x_old, lambda_new)")
        self.up = up
        return up


def _case(name, opts=None, hessian="exact", B=None, plain=False):
    case = Case(name, dict(opts or {}), B=B, hessian=hessian)
    case.set(trace=4)
    if plain:
        case.plain_bounds()
    return case


def _report(s, what):
    print("%s: %d rounds, %d corrections, smallest margin of a decision %.2g; %s" % (
        what, s.rounds, s.corrections, s.min_margin,
        " | ".join("instance %d: ls %d soc %d armijo %d accepted %d enter_resto %d status %d" % (
            b, R["ls"], R["soc_p"] + 1 if R["soc_on"] or R["use_soc"] else 0, R["armijo"], R["accepted"], R["enter_resto"], R["status"])
            for b, R in enumerate(s.R))))


# ---------------------------------------------------------------------------------------------------------------- the full step
@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["exact", "limited-memory", "nlp_scaling"])
@pytest.mark.parametrize("name", ["quadrotor", "bryson_denham"])
def test_full_step_and_update(built, name, variant):
    """the cold start: the oracle takes the full fraction-to-the-boundary step by (18) there, no correction, no halving"""
    case = _case(name, tp.SCALED if variant == "nlp_scaling" else {}, hessian="limited-memory" if variant == "limited-memory" else "exact")
    st = case.start(warm=False)
    s = Search(case, st).run()
    for b in range(case.B):
        R = s.R[b]
        assert R["accepted"] or R["enter_resto"] or R["status"], (name, b, R)
        if variant == "exact":               # (what the oracle does on this problem; the other variants take whatever branch they take)
            assert (R["accepted"], R["ls"], R["soc_on"], R["use_soc"], R["armijo"]) == (1, 0, 0, 0, 0), (name, b, R)
            assert R["alpha"] == R["alpha_max"]
    s.update()
    _report(s, "%s %s cold start" % (name, variant))
    case.close()


@pytest.mark.gpu
def test_dominance_at_equality(built):
    """a filter entry that equals the trial point in theta and in phi, bit for bit, dominates it (>=, paper section 2.3: the filter
    holds the pairs that are NOT acceptable); an entry whose phi is the next double above does not.  bryson_denham from the cold start:
    without a filter the first trial point is taken; its theta and phi, as the device computed them, go into the filter of a second,
    identical pass."""
    case = _case("bryson_denham")
    s0 = Search(case, case.start(warm=False)).run()
    assert all(len(e) == 1 and e[0][2] for e in s0.events)
    th, phi = [R["th_trial"] for R in s0.R], [R["phi_trial"] for R in s0.R]
    filt = [[(th[0], phi[0])], [(th[1], float(np.nextafter(phi[1], np.inf)))]]
    s = Search(case, case.start(warm=False), filt=filt, edge_rounds=1).run()
    assert s.events[0][0][2] is False and s.R[0]["ls"] + s.corrections >= 1, s.events[0]          # dominated: the search went on
    assert s.events[1] == s0.events[1] and s.R[1]["accepted"] == 1                                 # not dominated: as without a filter
    s.update()
    _report(s, "bryson_denham, filter entries at the first trial point")
    case.close()


# ---------------------------------------------------------------------------------------------------------------- launch(2, 5)
def _launch_case(z, scenarios, **opts):
    """launch(2, 5), B = 2: instance b starts from the recorded iterate of scenarios[b]"""
    case = _case("launch_2x5", dict(PUSHES, mu_strategy=0), plain=True)
    names = [str(s_) for s_ in z["scenario"]]
    ks = [names.index(s_) for s_ in scenarios]
    idx = [int(z["scenario_state"][k]) for k in ks]
    n = case.lay.n
    assert z["v"].shape[1] == case.lay.nv and z["lam"].shape[1] == case.lay.m
    case.set(**opts)
    mus = z["mu"][idx]
    assert len(set(mus.tolist())) == 1, "mu_init is one option for the batch"
    case.set(mu_init=float(mus[0]))
    st = case.start(z["v"][idx][:, :n], z["lam"][idx], (z["zL"][idx][:, :n], z["zU"][idx][:, :n]))
    return case, st, ks


def test_scenario_batches_share_mu():
    """(CPU) the pairs below are built from iterates with the same mu"""
    z = np.load(STATES)
    names = [str(s_) for s_ in z["scenario"]]
    for pair in LAUNCH_PAIRS:
        mus = {float(z["mu"][z["scenario_state"][names.index(p)]]) for p in pair[0]}
        assert len(mus) == 1, pair


# (scenarios of the two instances, the filter injected per instance, options)
LAUNCH_PAIRS = [
    (("correction_accepted", "dominated_alpha_min"), ([], DOMINATING), {}),
    (("dominated_max_ls", "dominated_max_ls"), (DOMINATING, DOMINATING), {"max_line_search": 3}),
    (("dominated_max_ls", "correction_accepted"), (DOMINATING, []), {"max_line_search": 3, "restoration": 0}),
    (("armijo", "armijo"), ([], []), {}),
    (("armijo_b", "armijo_c"), ([], []), {}),
    (("correction_accepted_b", "correction_accepted_b"), ([], []), {}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", LAUNCH_PAIRS, ids=["+".join(p[0]) + ("" if p[2].get("restoration", 1) else "-no_restoration") for p in LAUNCH_PAIRS])
def test_launch_branches(built, pair):
    """iterates of the oracle injected again: the device takes the sequence of trial points the oracle takes from the same state"""
    scenarios, filt, opts = pair
    z = np.load(STATES)
    case, st, ks = _launch_case(z, scenarios, **opts)
    assert not st["status"].any()
    s = Search(case, st, filt=list(filt)).run()
    for b, k in enumerate(ks):
        cnt = z["sc_count"][k]
        s.follows(b, z["sc_kind"][k][:cnt], z["sc_took"][k][:cnt])
        R = s.R[b]
        if z["sc_accepted"][k]:
            assert (R["accepted"], R["armijo"], R["use_soc"]) == (1, z["sc_armijo"][k], int(z["sc_soc"][k] > 0)), (scenarios[b], R)
            assert R["ls"] == z["sc_ls"][k]
        elif opts.get("restoration", 1):
            assert (R["accepted"], R["enter_resto"], R["status"]) == (0, 1, 0) and R["ls"] == z["sc_ls"][k], (scenarios[b], R)
        else:                                            # the restoration phase switched off: the solve ends with status 3
            assert (R["accepted"], R["enter_resto"], R["status"]) == (0, 0, 3) and R["ls"] == z["sc_ls"][k], (scenarios[b], R)
        if scenarios[b] == "dominated_alpha_min":
            assert R["alpha"] < R["alpha_min"] and R["ls"] <= case.o["max_ls"]
        if scenarios[b] == "dominated_max_ls":
            assert R["alpha"] >= R["alpha_min"] and R["ls"] == case.o["max_ls"] + 1
    s.update()
    _report(s, "launch_2x5 " + " / ".join(scenarios))
    case.close()


@pytest.mark.gpu
def test_corrected_trial_point_is_tested_with_the_uncorrected_step_length(built):
    """A-5.8: the switching condition (19) and the Armijo test (20) of a corrected trial point use alpha, not alpha_soc.  The state is
    built for it (tests/golden/make_ipm_line_search_states.py): theta <= theta_min, and the step length at which (19) switches lies
    between alpha and alpha_soc.  With the first trial point itself in the filter the correction opens and is accepted — by (18),
    armijo 0, a filter entry follows; with alpha_soc in (19) it would be taken by (20), armijo 1, and none would."""
    z = np.load(STATES)
    case = _case("launch_2x5", dict(PUSHES, mu_strategy=0), plain=True)
    i, n = int(z["uncorrected_step_length_state"]), case.lay.n
    two = lambda a: np.tile(a, (case.B, 1))
    inputs = (two(z["uncorrected_step_length_x"]), two(z["lam"][i]), (two(z["zL"][i][:n]), two(z["zU"][i][:n])))
    case.set(mu_init=float(z["mu"][i]))
    s0 = Search(case, case.start(*inputs))
    s0.round()
    filt = [[(R["th_trial"], R["phi_trial"])] for R in s0.R]
    s = Search(case, case.start(*inputs), filt=filt, edge_rounds=1).run()
    o = case.o
    for b in range(case.B):
        R = s.R[b]
        assert [(e[0], e[2]) for e in s.events[b]] == [(False, False), (True, True)], s.events[b]
        assert (R["accepted"], R["use_soc"], R["armijo"], R["ls"]) == (1, 1, 0, 0), R
        assert R["theta"] <= R["theta_min"] and R["dphi"] < 0
        switches_at = o["delta"] * R["theta"] ** o["s_theta"] / (-R["dphi"]) ** o["s_phi"]
        assert R["alpha"] * 1.001 < switches_at < R["alpha_soc"] / 1.001, (R["alpha"], switches_at, R["alpha_soc"])
        cur = {k: R[k] for k in ("theta", "theta_min", "theta_max", "phi", "dphi")}
        assert ref.filter_accepts(o, cur, R["th_trial"], R["phi_trial"], R["alpha_soc"], [])[:2] == (True, True)     # what the wrong step length gives
    up = s.update()
    assert (up["inst"]["nfilt"] == 2).all()
    _report(s, "launch_2x5, (19) switches between alpha and alpha_soc")
    case.close()


@pytest.mark.gpu
def test_launch_cold_start_correction_dropped_then_halvings(built):
    """launch(2, 5) from the seeded starts 40 and 41: a correction is opened, dropped after one, then three halvings"""
    z = np.load(STATES)
    case = _case("launch_2x5", {"mu_strategy": 0}, plain=True)
    st = case.start(warm=False)
    s = Search(case, st).run()
    for b in range(2):
        assert tuple(z["state"][b]) == (40 + b, 0)
        cnt = z["ev_count"][b]
        s.follows(b, z["ev_kind"][b][:cnt], z["ev_took"][b][:cnt])
        assert (s.R[b]["ls"], s.R[b]["accepted"], s.R[b]["use_soc"], s.R[b]["n_soc"]) == (3, 1, 0, 0)
    s.update()
    _report(s, "launch_2x5 cold start")
    case.close()


# ---------------------------------------------------------------------------------------------------------------- giving up at a feasible point
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["acceptable", "recalc"])
def test_give_up_at_a_feasible_point(built, which):
    """the converged quadrotor points injected again with a filter entry that takes no trial point.  acceptable: tol = 1e-12, E_0 is
    at the acceptable level, status 6.  recalc: other multipliers and tol = 1e-4, so theta <= tol with a large E_0: enter_resto 2,
    after more than max_ls halvings and, on two instances, four corrections (soc_p up to 3)."""
    z = np.load(STATES)
    case = _case("quadrotor", dict(PUSHES, mu_strategy=0), plain=True)
    assert np.array_equal(case.XL[:, [0, 9]], z["quadrotor_x"][:, [0, 9]])          # the instance bounds the fixture was made with
    tol = {"acceptable": 1e-12, "recalc": 1e-4}[which]
    case.set(tol=tol)
    lam = z["quadrotor_lam"] if which == "acceptable" else case.lam
    st = case.start(z["quadrotor_x"], lam, (z["quadrotor_zL"], z["quadrotor_zU"]))
    s = Search(case, st, filt=[DOMINATING] * case.B).run()
    pre = "quadrotor_%s_" % which
    for b in range(case.B):
        cnt = z[pre + "count"][b]
        s.follows(b, z[pre + "kind"][b][:cnt], z[pre + "took"][b][:cnt])
        R = s.R[b]
        assert R["accepted"] == 0 and R["ls"] == z[pre + "ls"][b]
        if which == "acceptable":
            assert (R["status"], R["enter_resto"]) == (6, 0) and R["err0"] <= case.o["acceptable_tol"]
        else:
            assert (R["status"], R["enter_resto"]) == (0, 2) and R["theta"] <= tol and R["ls"] == case.o["max_ls"] + 1
    tried = sum(int(z[pre + "kind"][b][:z[pre + "count"][b]].sum()) for b in range(case.B))
    assert s.corrections == tried
    if which == "recalc":                                # second and later corrections ran (A-5.9), up to the last one max_soc allows
        assert tried >= 8 and s.max_soc_p == case.o["max_soc"] - 1, (tried, s.max_soc_p)
    s.update()
    _report(s, "quadrotor " + which)
    case.close()


# ---------------------------------------------------------------------------------------------------------------- several workgroups per instance
@pytest.mark.gpu
def test_launch_16x8_several_workgroups(built):
    """launch(16, 8), B = 2, from the cold start, whatever branch it takes: ipm_accept_kernel and ipm_update_kernel run several
    workgroups per instance — the slices of the trial sums and of apply_step, one record write"""
    case = _case("launch_16x8", {"mu_strategy": 0})
    assert case.lay.nv >= 4096 and case.B <= 32 and (max(case.lay.nv, case.lay.m) + 1023) // 1024 >= 2
    st = case.start(warm=False)
    s = Search(case, st).run()
    s.update()
    assert all(R["accepted"] or R["enter_resto"] or R["status"] for R in s.R)
    _report(s, "launch_16x8 cold start")
    case.close()


# ---------------------------------------------------------------------------------------------------------------- a NaN instance
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["quadrotor", "launch_2x5"])
def test_nan_instance_touches_no_other(built, name):
    """state (d) of tests/test_ipm_pass.py: the instance with a NaN in lambda has status 5; every other instance is bit-identical
    through the line search and the update to the batch without it"""
    case = _case(name)
    bad = case.B - 1
    lam = case.lam.copy()
    lam[bad, 3] = np.nan
    runs = []
    for lam_ in (case.lam, lam):
        st = case.start(lam=lam_)
        case.ipm.debug_pass(3)
        rounds = []
        for _ in range(case.o["max_ls"] + case.o["max_soc"] + 3):
            rounds.append(case.ipm.debug_line_search(1))
            if rounds[-1]["counts"] == (0, 0):
                break
        runs.append((st, rounds, case.ipm.debug_update(N_FILTER), [case.ipm.trace(b) for b in range(case.B)]))
    (_, clean, clean_up, clean_tr), (st, dirty, dirty_up, dirty_tr) = runs
    assert st["status"][bad] == 5 and not st["status"][:bad].any()
    keep = [b for b in range(bad) if clean[-1]["inst"]["accepted"][b] or clean[-1]["inst"]["enter_resto"][b]]
    assert keep, "no other instance ran to the end of its line search"
    # (the batch without the NaN may run more rounds, for the instance that is the bad one in the other batch)
    # The correction's arrays only after the last round: before an instance's first correction they hold what the run before left.
    for i, (ra, rb) in enumerate(zip(clean, dirty)):
        last = i == min(len(clean), len(dirty)) - 1
        for k in ("xt", "objt", "gt", "ct", "record") + (("csoc", "dv2", "dlam2", "dzL2", "dzU2") if last else ()):
            a_, b_ = np.ascontiguousarray(ra[k][:bad]), np.ascontiguousarray(rb[k][:bad])
            assert np.array_equal(a_.view(np.uint64), b_.view(np.uint64)), (name, i, k)
        assert rb["inst"]["status"][bad] == 5
    for k in ("v", "zL", "zU", "lambda", "filter", "record"):
        a_, b_ = np.ascontiguousarray(clean_up[k][keep]), np.ascontiguousarray(dirty_up[k][keep])
        assert np.array_equal(a_.view(np.uint64), b_.view(np.uint64)), (name, k)
    assert dirty_up["inst"]["status"][bad] == 5 and dirty_up["inst"]["iter"][bad] == 0 and len(dirty_tr[bad]) == 0
    for b in keep:
        assert np.array_equal(clean_tr[b], dirty_tr[b])
    case.close()


# ---------------------------------------------------------------------------------------------------------------- misuse
@pytest.mark.gpu
def test_misuse_of_the_hooks(built):
    case = _case("bryson_denham")
    ipm = case.ipm
    case.start()
    with pytest.raises(RpmError, match="directly after rpm_ipm_debug_pass"):        # a start is no stage-3 pass
        ipm.debug_line_search(1)
    with pytest.raises(RpmError, match="directly after rpm_ipm_debug_line_search"):
        ipm.debug_update()
    ipm.debug_pass(2)
    with pytest.raises(RpmError, match="directly after rpm_ipm_debug_pass"):        # nor is a stage-2 pass
        ipm.debug_line_search(1)
    case.start()
    ipm.debug_pass(3)
    with pytest.raises(RpmError, match="directly after rpm_ipm_debug_line_search"):
        ipm.debug_update()
    with pytest.raises(RpmError, match="rounds >= 1"):
        ipm.debug_line_search(0)
    with pytest.raises(RpmError, match="at most 1024 filter entries"):
        ipm.debug_line_search(1, [[(0.0, 0.0)] * 1025] * case.B)
    ipm.debug_line_search(1)                             # (the refused calls left the state alone)
    ipm.debug_line_search(1)                             # valid after itself
    ipm.debug_update()
    with pytest.raises(RpmError, match="directly after rpm_ipm_debug_line_search"):  # one update per line search
        ipm.debug_update()
    with pytest.raises(RpmError, match="directly after rpm_ipm_debug_pass"):
        ipm.debug_line_search(1)
    case.start()
    ipm.debug_pass(3)
    ipm.solve(case.X0)                                   # a solve in between
    with pytest.raises(RpmError, match="directly after rpm_ipm_debug_pass"):
        ipm.debug_line_search(1)
    with pytest.raises(RpmError, match="stage 1, 2 or 3"):                            # the stage-1..3 hook still refuses stage 4
        ipm.debug_pass(4)
    # a converged point: the stage-3 pass leaves no instance running, so there is no line search to run
    sol = ipm.solve(case.X0)
    assert (sol["status"] == 0).all()
    zb = ipm.bound_multipliers()
    case.set(**dict(PUSHES, mu_init=1e-9))
    case.start(sol["x"], sol["lambda"], zb)
    out = ipm.debug_pass(3)
    assert (out["inst"]["status"] == 1).all()
    with pytest.raises(RpmError, match="left an instance running"):
        ipm.debug_line_search(1)
    case.close()
