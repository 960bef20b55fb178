"""Reference of one interior-point pass for tests/test_ipm_pass.py (device) and tests/test_ipm_pass_reference.py (CPU).  Not a test
module.

Written from Waechter & Biegler, "On the implementation of an interior-point filter line-search algorithm for large-scale nonlinear
programming" (Math. Program. 106, 2006; equation numbers below are the paper's) and from the option documentation in
include/rpm_hip.h; it shares no table, no order of operations and no code with the kernels.  Arithmetic is numpy.longdouble (wider
than double on x86-64; where it is not, the comparisons of the device tests still hold with the same bounds, the reference is then
one more double evaluation).  Dense matrices, one instance at a time.

The problem as the solver holds it: unknowns v = (x, s), one slack s per inequality row (rows with g_l != g_u, ascending), bounds
vl <= v <= vu (relaxed; vl == vu: a fixed unknown, which takes no part), constraints c(v) = 0 with c_r = g_r - g_l,r on an equality
row and c_r = g_r - s on an inequality row, multipliers lambda (m), zL, zU (nv).  With nlp_scaling the caller passes scaled g, grad,
jac, hess, the scaled row bounds and sf.

The comparison rule of the device tests (stated once here and in DESIGN.md f-2): a single expression or a maximum,
|dev - ref| <= 8 * 2^-52 * M with M the sum of the magnitudes of its operands; a sum of k terms, (k + 8) * 2^-52 * sum |term|.  Every
quantity below therefore comes with its M (`mag`) and, for sums, its k (`cnt`).
"""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
INF = 1e19                   # Ipopt's nlp_lower_bound_inf / nlp_upper_bound_inf: a bound beyond it does not exist

# paper section 4 / Ipopt's defaults, and the options of rpm_ipm_set_option (include/rpm_hip.h)
OPTS = dict(tol=1e-8, mu_init=0.1, kappa_eps=10.0, kappa_mu=0.2, theta_mu=1.5, tau_min=0.99, s_max=100.0,
            gamma_theta=1e-5, gamma_phi=1e-8, delta=1.0, s_theta=1.1, s_phi=2.3, gamma_alpha=0.05, delta_c=1e-9,
            max_iter=3000, acceptable_tol=1e-6, acceptable_iter=15, mu_strategy=1, mu_max_fact=1e3, mu_red_fact=0.9999,
            dual_inf_tol=1.0, constr_viol_tol=1e-4, compl_inf_tol=1e-4,
            acc_dual_inf_tol=1e10, acc_constr_viol_tol=1e-2, acc_compl_inf_tol=1e-2,
            delta_w_first=1e-4, kw_inc_first=100.0)          # Algorithm IC's first rungs (IpmOpts; no option sets them)


def single_tol(mag):
    return 8.0 * EPS * np.asarray(mag, dtype=np.float64)


def sum_tol(cnt, mag):
    return (np.asarray(cnt, dtype=np.float64) + 8.0) * EPS * np.asarray(mag, dtype=np.float64)


def ulps(a, b):
    """distance of two doubles in units of the spacing at the larger one"""
    a, b = np.float64(a), np.float64(b)
    if a == b:
        return 0.0
    return float(abs(a - b) / np.spacing(max(abs(a), abs(b))))


class Layout:
    """Sizes and structures, 0-based: Jacobian triplets (row, column), Hessian triplets of the lower triangle (duplicates are
    summed), the slack of every inequality row."""

    def __init__(self, n, m, gl, gu, jac_rows, jac_cols, hess_rows=None, hess_cols=None):
        self.n, self.m = int(n), int(m)
        self.srow = np.nonzero(np.asarray(gl) != np.asarray(gu))[0]
        self.ns = self.srow.size
        self.nv, self.nt = self.n + self.ns, self.n + self.ns + self.m
        self.jr, self.jc = np.asarray(jac_rows, dtype=np.int64), np.asarray(jac_cols, dtype=np.int64)
        assert self.jr.min() >= 0 and self.jr.max() < m and self.jc.min() >= 0 and self.jc.max() < n
        if hess_rows is None:
            self.hr = self.hc = None
        else:
            a, b = np.asarray(hess_rows, dtype=np.int64), np.asarray(hess_cols, dtype=np.int64)
            self.hr, self.hc = np.maximum(a, b), np.minimum(a, b)
            assert self.hc.min() >= 0 and self.hr.max() < n


def zero_based(rows, cols, n_rows, n_cols):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    if rows.max() == n_rows or cols.max() == n_cols:          # 1-based triplets
        return rows - 1, cols - 1
    return rows, cols


def bound_kinds(vl, vu):
    free = vl != vu
    return free, free & (vl > -INF), free & (vu < INF)


# ------------------------------------------------------------------------------------------------------------- c, grad_x L
def constraints(lay, v, g, gl_rows):
    """c and the magnitude of its operands; gl_rows: the (scaled) g_l of every row"""
    c = LD(g) - LD(gl_rows)
    mag = np.abs(g) + np.abs(gl_rows)
    c[lay.srow] = LD(g[lay.srow]) - LD(v[lay.n:])
    mag[lay.srow] = np.abs(g[lay.srow]) + np.abs(v[lay.n:])
    return c, mag


def grad_lagrangian(lay, grad, jac, lam):
    """grad f + A' lambda on x, -lambda_r on the slack of row r (the slack's column of the constraint Jacobian is -1); per entry
    the sum of the magnitudes of the terms and their number"""
    terms = LD(jac) * LD(lam)[lay.jr]
    gx = LD(grad).copy()
    np.add.at(gx, lay.jc, terms)
    mag = np.abs(grad).astype(np.float64)
    np.add.at(mag, lay.jc, np.abs(terms).astype(np.float64))
    cnt = np.ones(lay.n)
    np.add.at(cnt, lay.jc, 1.0)
    gs = -LD(lam)[lay.srow]
    return np.concatenate([gx, gs]), np.concatenate([mag, np.abs(lam[lay.srow])]), np.concatenate([cnt, np.ones(lay.ns)])


# ------------------------------------------------------------------------------------------------------------- (5), (6)
def residual_scalars(lay, v, vl, vu, zL, zU, lam, c, glag, row_scale=None):
    """The scalars of the optimality error from c (m) and grad_x L (nv) as given (long double or the device's doubles): values
    `val`, operand magnitudes `mag`, term counts `cnt` (sums only)."""
    free, lo, up = bound_kinds(vl, vu)
    v, vl, vu, zL, zU, lam, c, glag = (LD(a) for a in (v, vl, vu, zL, zU, lam, c, glag))
    val, mag, cnt = {}, {}, {}
    dres = (glag - zL + zU)[free]
    val["dinf"] = np.abs(dres).max() if dres.size else LD(0)
    mag["dinf"] = float((np.abs(glag) + np.abs(zL) + np.abs(zU))[free].max()) if dres.size else 0.0
    val["cinf"] = np.abs(c).max() if c.size else LD(0)
    mag["cinf"] = float(val["cinf"])
    val["theta"], mag["theta"], cnt["theta"] = np.abs(c).sum(), float(np.abs(c).sum()), c.size
    dl, du = (v - vl)[lo], (vu - v)[up]
    prod = np.concatenate([zL[lo] * dl, zU[up] * du])
    z = np.concatenate([zL[lo], zU[up]])
    d = np.concatenate([dl, du])
    nzb = prod.size
    val["nzb"] = nzb
    val["comp_max"] = max(prod.max(), LD(0)) if nzb else LD(0)
    val["comp_min"] = min(prod.min(), LD(1e300)) if nzb else LD(1e300)
    mag["comp_max"], mag["comp_min"] = float(abs(val["comp_max"])), float(abs(val["comp_min"]))
    val["sum_z"], mag["sum_z"], cnt["sum_z"] = z.sum(), float(np.abs(z).sum()), nzb
    logs = np.log(d)
    val["lnsum"], mag["lnsum"], cnt["lnsum"] = logs.sum(), float(np.abs(logs).sum()), nzb
    val["sum_lam"], mag["sum_lam"], cnt["sum_lam"] = np.abs(lam).sum(), float(np.abs(lam).sum()), lam.size
    # what the adaptive rule's KKT error needs (squared 2-norms; all terms positive)
    val["psum"], val["psq"] = prod.sum(), (prod * prod).sum()
    val["dsq"], val["nfree"] = (dres * dres).sum(), int(free.sum())
    val["csq"] = (c * c).sum()
    cu = c if row_scale is None else c / LD(row_scale)
    val["cinf_u"] = np.abs(cu).max() if c.size else LD(0)
    return val, mag, cnt


def scaling_6(o, sum_lam, sum_z, m, nzb):
    """s_d and s_c of (6)"""
    s_max = o["s_max"]
    s_d = max(s_max, (sum_lam + sum_z) / max(1, m + nzb)) / s_max
    s_c = max(s_max, sum_z / nzb) / s_max if nzb > 0 else 1.0
    return s_d, s_c


def error_5(o, mu, dinf, cinf, comp_max, comp_min, s_d, s_c, nzb):
    """E_mu of (5); |XZe - mu e|_inf from the extreme products"""
    comp = max(abs(comp_max - mu), abs(comp_min - mu)) if nzb > 0 else 0.0
    return max(dinf / s_d, cinf, comp / s_c)


def decide(o, s, f, mu_in, m, sf=1.0, iteration=0, n_acc=0):
    """Termination verdict and barrier update of the first pass of a solve from the scalars `s` (a dict as residual_scalars gives,
    long double or double): -> (what the pass leaves in the record, the relative margin of every yes/no decision taken).  status is
    the device's: 0 running, 1 converged, 6 acceptable level, 2 iteration limit."""
    margins = []

    def le(a, b, what):         # a <= b, with its margin on record
        scale = max(abs(a), abs(b))
        margins.append((what, float(abs(a - b) / scale) if scale > 0 else 1.0))
        return a <= b

    nzb = s["nzb"]
    s_d, s_c = scaling_6(o, s["sum_lam"], s["sum_z"], m, nzb)
    out = {"s_d": s_d, "s_c": s_c}
    e0 = error_5(o, 0.0, s["dinf"], s["cinf"], s["comp_max"] if nzb else 0.0, s["comp_max"] if nzb else 0.0, s_d, s_c, nzb)
    out["err0"] = e0
    dinf_u, cm = s["dinf"] / sf, (s["comp_max"] if nzb else 0.0) / sf
    out.update(status=0, n_acc=n_acc, nfilt=0, fixed_mode=0, nrefs=0, refs0=0.0, mu=mu_in, mu_max=0.0, falls=0)
    if all([le(e0, o["tol"], "E_0 <= tol"), le(dinf_u, o["dual_inf_tol"], "dual_inf_tol"), le(s["cinf_u"], o["constr_viol_tol"], "constr_viol_tol"),
            le(cm, o["compl_inf_tol"], "compl_inf_tol")]):
        out["status"] = 1
        return out, margins
    acc = all([le(e0, o["acceptable_tol"], "E_0 <= acceptable_tol"), le(dinf_u, o["acc_dual_inf_tol"], "acc dual"),
               le(s["cinf_u"], o["acc_constr_viol_tol"], "acc constr"), le(cm, o["acc_compl_inf_tol"], "acc compl")])
    out["n_acc"] = n_acc + 1 if acc else 0
    if o["acceptable_iter"] > 0 and out["n_acc"] >= o["acceptable_iter"]:
        out["status"] = 6
        return out, margins
    if iteration >= o["max_iter"]:
        out["status"] = 2
        return out, margins
    th = s["theta"]
    out["theta_max"], out["theta_min"] = 1e4 * max(1.0, th), 1e-4 * max(1.0, th)        # filter bounds (paper section 2.3, 3.3 of Ipopt's defaults)
    mu_min = o["tol"] / 10.0
    mu = mu_in
    if o["mu_strategy"] == 1 and nzb > 0:
        # Ipopt's adaptive strategy, first pass (no history: progress by definition, the free mode): the LOQO rule
        #   mu = sigma avg,  sigma = 0.1 min(0.05 (1 - xi) / xi, 2)^3,  xi = min_i(z_i d_i) / avg,  avg = the mean product,
        # kept inside [mu_min, mu_max], mu_max = mu_max_fact avg fixed at the first pass; the KKT error of the globalisation
        # (2-norm-squared, each part over its count) becomes the first reference value; a changed mu empties the filter
        avg = s["psum"] / nzb
        out["mu_max"] = o["mu_max_fact"] * avg
        out["refs0"] = s["dsq"] / max(1, s["nfree"]) + (s["csq"] / m if m else 0.0) + s["psq"] / nzb
        out["nrefs"] = 1
        xi = s["comp_min"] / avg
        ratio = 0.05 * (1.0 - xi) / xi
        margins.append(("LOQO ratio against 2", float(abs(ratio - 2.0) / max(abs(ratio), 2.0))))
        fac = min(ratio, 2.0)
        cand = 0.1 * fac * fac * fac * avg
        margins.append(("mu against mu_min", float(abs(cand - mu_min) / max(abs(cand), mu_min))))
        mu = max(mu_min, min(cand, out["mu_max"]))
        margins.append(("mu changed", float(abs(mu - mu_in) / max(abs(mu), abs(mu_in)))))
    else:
        # monotone rule (7): mu falls for as long as the barrier problem is solved to kappa_eps mu
        for _ in range(64):
            emu = error_5(o, mu, s["dinf"], s["cinf"], s["comp_max"], s["comp_min"], s_d, s_c, nzb)
            if not le(emu, o["kappa_eps"] * mu, "E_mu <= kappa_eps mu (fall %d)" % out["falls"]):
                break
            if mu <= mu_min:
                break
            mu = max(mu_min, min(o["kappa_mu"] * mu, mu ** o["theta_mu"]))
            if mu != mu_min:
                margins.append(("mu above mu_min", float((mu - mu_min) / mu)))
            out["falls"] += 1
    out["mu"] = mu
    out["tau"] = max(o["tau_min"], 1.0 - mu)                                             # (8)
    out["phi"] = f - mu * s["lnsum"]
    out["phi_mag"] = float(abs(f) + abs(mu * s["lnsum"]))
    return out, margins


# ------------------------------------------------------------------------------------------------------------- (13)
def kkt_13(lay, v, vl, vu, zL, zU, jac, hess, delta_w, delta_c, sigma=None):
    """The reduced matrix [[W + Sigma + delta_w I, A'], [A, -delta_c I]] over (x, s, lambda), dense and symmetric, with the
    magnitude sum and the number of terms of every entry.  Fixed unknowns: an identity row.  hess None: sigma I for W on x."""
    n, nv, nt = lay.n, lay.nv, lay.nt
    free, lo, up = bound_kinds(vl, vu)
    K, M, N = np.zeros((nt, nt), dtype=LD), np.zeros((nt, nt)), np.zeros((nt, nt))

    def add(r, c, val):
        np.add.at(K, (r, c), LD(val))
        np.add.at(M, (r, c), np.abs(np.asarray(val, dtype=np.float64)))
        np.add.at(N, (r, c), 1.0)

    if hess is not None:
        keep = free[lay.hr] & free[lay.hc]
        add(lay.hr[keep], lay.hc[keep], hess[keep])
    idx = np.nonzero(free)[0]
    if sigma is not None:
        ix = idx[idx < n]
        add(ix, ix, np.full(ix.size, sigma))
    add(idx, idx, np.full(idx.size, delta_w))
    il, iu = np.nonzero(lo)[0], np.nonzero(up)[0]
    sl = LD(zL[il]) / (LD(v[il]) - LD(vl[il]))
    su = LD(zU[iu]) / (LD(vu[iu]) - LD(v[iu]))
    np.add.at(K, (il, il), sl); np.add.at(M, (il, il), np.abs(sl).astype(np.float64)); np.add.at(N, (il, il), 1.0)
    np.add.at(K, (iu, iu), su); np.add.at(M, (iu, iu), np.abs(su).astype(np.float64)); np.add.at(N, (iu, iu), 1.0)
    fx = np.nonzero(~free)[0]
    K[fx, fx], M[fx, fx], N[fx, fx] = 1.0, 1.0, 1.0
    keep = free[lay.jc]
    assert not (N[nv + lay.jr[keep], lay.jc[keep]] > 0).any() and np.unique(lay.jr[keep] * n + lay.jc[keep]).size == keep.sum()   # one entry per slot
    add(nv + lay.jr[keep], lay.jc[keep], jac[keep])
    add(nv + lay.srow, n + np.arange(lay.ns), np.full(lay.ns, -1.0))
    r = nv + np.arange(lay.m)
    add(r, r, np.full(lay.m, -delta_c))
    low = np.tril(np.ones((nt, nt), dtype=bool))
    K, M, N = np.where(low, K, 0), np.where(low, M, 0), np.where(low, N, 0)
    K = K + np.tril(K, -1).T
    return K, M + np.tril(M, -1).T, N + np.tril(N, -1).T


def rhs_13(lay, v, vl, vu, glag, c, mu):
    """-(grad phi_mu + A' lambda, c) of (13): on a free unknown -(grad_x L - mu / (v - l) + mu / (u - v)) with grad_x L WITHOUT the
    bound multipliers (glag as grad_lagrangian gives it), 0 on a fixed one; -c on the rows.  With the operands' magnitudes."""
    free, lo, up = bound_kinds(vl, vu)
    v, vl, vu, mu = LD(v), LD(vl), LD(vu), LD(mu)
    r, mag = LD(glag).copy(), np.abs(np.asarray(glag, dtype=np.float64))
    tl, tu = np.zeros(lay.nv, dtype=LD), np.zeros(lay.nv, dtype=LD)
    tl[lo] = mu / (v - vl)[lo]
    tu[up] = mu / (vu - v)[up]
    r = np.where(free, -(r - tl + tu), LD(0))
    mag = np.where(free, mag + np.abs(tl).astype(np.float64) + np.abs(tu).astype(np.float64), 0.0)
    return np.concatenate([r, -LD(c)]), np.concatenate([mag, np.abs(np.asarray(c, dtype=np.float64))])


# ------------------------------------------------------------------------------------------------------------- (12), (15), (23)
def step_quantities(lay, o, v, vl, vu, zL, zU, grad, dv, mu, tau, theta, theta_min, dz_for_alpha=None):
    """From a step dv (nv): dz (12), the fraction-to-the-boundary step lengths (15), the slope of the barrier objective and
    alpha_min (23).  dz_for_alpha = (dzL, dzU): the multipliers' steps (15b) is evaluated on (the device's own); default: these."""
    free, lo, up = bound_kinds(vl, vu)
    v, vl, vu, zL, zU, d, mu = LD(v), LD(vl), LD(vu), LD(zL), LD(zU), LD(dv), LD(mu)
    nv = lay.nv
    dzL, dzU, mL, mU = np.zeros(nv, dtype=LD), np.zeros(nv, dtype=LD), np.zeros(nv), np.zeros(nv)
    sL, sU = np.where(lo, v - vl, LD(1)), np.where(up, vu - v, LD(1))
    tL = np.stack([mu / sL, -zL, -zL / sL * d])                   # (12): dz = mu / s - z - (z / s) ds, ds = dv at a lower bound
    tU = np.stack([mu / sU, -zU, zU / sU * d])                    #       ds = -dv at an upper bound
    dzL[lo], dzU[up] = tL.sum(0)[lo], tU.sum(0)[up]
    mL[lo], mU[up] = np.abs(tL).sum(0).astype(np.float64)[lo], np.abs(tU).sum(0).astype(np.float64)[up]
    out = {"dzL": dzL, "dzU": dzU, "dzL_mag": mL, "dzU_mag": mU}
    # (15a): largest alpha in (0, 1] with s + alpha ds >= (1 - tau) s
    cand = [LD(1)]
    m_ = lo & (d < 0)
    cand += list((-tau * sL / np.where(m_, d, LD(1)))[m_])
    m_ = up & (d > 0)
    cand += list((tau * sU / np.where(m_, d, LD(1)))[m_])
    out["alpha_max"] = min(cand)
    # (15b) on the multipliers
    eL, eU = (dzL, dzU) if dz_for_alpha is None else (LD(dz_for_alpha[0]), LD(dz_for_alpha[1]))
    cand = [LD(1)]
    m_ = lo & (eL < 0)
    cand += list((-tau * zL / np.where(m_, eL, LD(1)))[m_])
    m_ = up & (eU < 0)
    cand += list((-tau * zU / np.where(m_, eU, LD(1)))[m_])
    out["alpha_z"] = min(cand)
    # slope of phi_mu = f - mu sum log(slack) along dv
    gphi = np.concatenate([LD(grad), np.zeros(lay.ns, dtype=LD)])
    gmag = np.abs(gphi).astype(np.float64)
    a, b = np.where(lo, mu / sL, LD(0)), np.where(up, mu / sU, LD(0))
    gphi = gphi - a + b
    gmag = gmag + np.abs(a).astype(np.float64) + np.abs(b).astype(np.float64)
    out["dphi"] = (gphi * d)[free].sum()
    out["dphi_mag"] = float((gmag * np.abs(d).astype(np.float64))[free].sum())
    out["dphi_cnt"] = int(free.sum())
    return out


def alpha_min_23(o, theta, theta_min, dphi):
    """(23)"""
    a = o["gamma_theta"]
    if dphi < 0:
        a = min(a, o["gamma_phi"] * theta / (-dphi))
        if theta <= theta_min:
            a = min(a, o["delta"] * theta ** o["s_theta"] / (-dphi) ** o["s_phi"])
    return o["gamma_alpha"] * a


# ------------------------------------------------------------------------------------------------------------- dense solve
def solve_ld(A, b):
    """A x = b by Gaussian elimination with partial pivoting in long double (numpy.linalg has none), then iterative refinement
    with the same factors (element growth on a quasi-definite matrix with delta_c = 1e-9 costs four digits otherwise)"""
    A0, b0 = np.array(A, dtype=LD), np.array(b, dtype=LD)
    LU, n = A0.copy(), b0.size
    perm = np.arange(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(LU[k:, k])))
        if p != k:
            LU[[k, p]], perm[[k, p]] = LU[[p, k]], perm[[p, k]]
        f = LU[k + 1:, k] / LU[k, k]
        nz = np.nonzero(f)[0]
        if nz.size:
            LU[k + 1 + nz, k + 1:] -= np.outer(f[nz], LU[k, k + 1:])
        LU[k + 1:, k] = f

    def lu_solve(r):
        y = r[perm].copy()
        for k in range(n):
            y[k] -= LU[k, :k] @ y[:k]
        for k in range(n - 1, -1, -1):
            y[k] = (y[k] - LU[k, k + 1:] @ y[k + 1:]) / LU[k, k]
        return y

    x = lu_solve(b0)
    for _ in range(4):
        x = x + lu_solve(b0 - A0 @ x)
    return x


def relative_residual(K, x, r):
    """max_i |K x - r|_i / (|K| |x| + |r|)_i"""
    K, x, r = np.asarray(K, dtype=LD), LD(x), LD(r)
    den = np.abs(K) @ np.abs(x) + np.abs(r)
    res = np.abs(K @ x - r)
    ok = den > 0
    return float((res[ok] / den[ok]).max()) if ok.any() else 0.0


# ------------------------------------------------------------------------------------------------------------- the line search
# Section 2.3 / Algorithm A of the paper, steps A-5.1 .. A-5.10 and A-6 .. A-7, for tests/test_ipm_line_search.py (device) and
# tests/test_ipm_line_search_reference.py (CPU).  Constants the first half of the pass does not need:
LS_OPTS = dict(eta_phi=1e-8, kappa_soc=0.99, max_soc=4, max_ls=40, kappa_sigma=1e10, resto=1, resto_rho=1000.0, max_recalc_y=3)
OPTS.update(LS_OPTS)


def _margin(a, b):
    scale = max(abs(a), abs(b))
    return float(abs(a - b) / scale) if scale > 0 else 1.0


def trial_point(v, vl, vu, dv, alpha):
    """v + alpha dv on the free unknowns (a fixed one stays), with the magnitude of the operands"""
    free = np.asarray(vl) != np.asarray(vu)
    step = LD(alpha) * LD(dv)
    return np.where(free, LD(v) + step, LD(v)), np.abs(np.asarray(v, dtype=np.float64)) + np.where(free, np.abs(step).astype(np.float64), 0.0)


def trial_constraints(lay, vt, vt_mag, gt, gl_rows):
    """c at a trial point vt (nv) from g there: g - g_l on a row without slack, g - s on a row with one"""
    c = LD(gt) - LD(gl_rows)
    mag = np.abs(gt) + np.abs(gl_rows)
    c[lay.srow] = LD(gt[lay.srow]) - LD(vt[lay.n:])
    mag[lay.srow] = np.abs(gt[lay.srow]) + np.asarray(vt_mag, dtype=np.float64)[lay.n:]
    return c, mag


def theta_1(c):
    """theta = |c|_1: value, magnitude, number of terms"""
    t = np.abs(LD(c)).sum() if np.size(c) else LD(0)
    return t, float(t), int(np.size(c))


def barrier_log_sum(vt, vl, vu):
    """sum of log(slack) over the bounds of the free unknowns at vt: value, magnitude, number of terms"""
    _, lo, up = bound_kinds(vl, vu)
    vt, vl, vu = LD(vt), LD(vl), LD(vu)
    with np.errstate(all="ignore"):
        logs = np.concatenate([np.log((vt - vl)[lo]), np.log((vu - vt)[up])])
    return logs.sum(), float(np.abs(logs).sum()), int(logs.size)


def barrier_objective(f, mu, lnsum):
    """phi_mu = f - mu sum log(slack): value, magnitude"""
    return LD(f) - LD(mu) * LD(lnsum), float(abs(f) + abs(mu * lnsum))


def filter_accepts(o, cur, th, phit, a_test, filt, finite=True):
    """Does the filter line search take the trial point (th, phit)?  cur: theta, theta_min, theta_max, phi, dphi of the current
    iterate; a_test: the step length of the switching and Armijo tests — of the UNCORRECTED step also for a corrected trial point
    (A-5.8); filt: the filter's (theta, phi) pairs.  -> (accepted, armijo, dominated, decisions) with decisions a list of
    (name, outcome, relative margin) in the order they are taken; a composite's margin is that of its deciding part."""
    dec = []
    theta, phi, dphi = cur["theta"], cur["phi"], cur["dphi"]
    slack = 10.0 * EPS * abs(phi)                       # Ipopt's allowance for rounding in the comparisons of phi
    if not finite:
        dec.append(("finite", False, 1.0))
        return False, False, False, dec
    ok_max = th <= cur["theta_max"]
    dec.append(("theta <= theta_max", ok_max, _margin(th, cur["theta_max"])))
    if not ok_max:
        return False, False, False, dec
    dominated = False
    for k, (ft, fp) in enumerate(filt):                 # (th, phit) is in the filter when an entry is no worse in both measures
        in_t, in_p = th >= ft, phit >= fp
        mt, mp = _margin(th, ft), _margin(phit, fp)
        both = in_t and in_p
        mg = min(mt, mp) if both else max(m_ for m_, inside in ((mt, in_t), (mp, in_p)) if not inside)
        dec.append(("filter entry %d" % k, both, mg))
        dominated = dominated or both
    if dominated:
        return False, False, True, dec
    sw = False
    if dphi < 0:                                        # (19)
        lhs, rhs = a_test * (-dphi) ** o["s_phi"], o["delta"] * theta ** o["s_theta"]
        sw = lhs > rhs
        dec.append(("switching condition (19)", sw, _margin(lhs, rhs)))
    else:
        dec.append(("dphi < 0", False, 1.0 if dphi > 0 else 0.0))
    small = theta <= cur["theta_min"]
    dec.append(("theta <= theta_min", small, _margin(theta, cur["theta_min"])))
    if small and sw:                                    # case I: Armijo (20)
        bound = phi + o["eta_phi"] * a_test * dphi + slack
        ok = phit <= bound
        dec.append(("Armijo (20)", ok, _margin(phit, bound)))
        return ok, ok, False, dec
    b18 = (1.0 - o["gamma_theta"]) * theta              # case II: sufficient decrease (18)
    ok_t, m_t = th <= b18, _margin(th, b18)
    bphi = phi - o["gamma_phi"] * theta + slack
    ok_p, m_p = phit <= bphi, _margin(phit, bphi)
    ok = ok_t or ok_p
    mg = max(m_ for m_, y in ((m_t, ok_t), (m_p, ok_p)) if y) if ok else min(m_t, m_p)
    dec.append(("sufficient decrease (18)", ok, mg))
    return ok, False, False, dec


LS_STATE = ("alpha", "ls", "accepted", "armijo", "soc_on", "soc_req", "soc_p", "th_old_soc", "use_soc", "n_soc", "enter_resto", "status")


def line_search_verdict(o, S, ok, armijo, th, finite=True):
    """What follows the test of one trial point (A-5.4 .. A-5.10), as a new copy of the state S: alpha (the uncorrected step
    length), ls, accepted, armijo, soc_on (corrected trial points are being tried), soc_req (the next round computes a correction),
    soc_p (corrections computed before the pending one), th_old_soc, use_soc, n_soc, enter_resto, status; S also holds theta, alpha_min,
    err0, n_recalc.  -> (state, decisions).  Giving up (alpha < alpha_min, or more than max_ls halvings): status 6 when E_0 is at the
    acceptable level; else the restoration phase (enter_resto 1) from an infeasible point; else, up to max_recalc_y times,
    least-squares multipliers at this point (enter_resto 2); else status 3.
    One step is Ipopt 3.12's and not the paper's: a corrected trial point that the filter rejects counts like any other rejected one
    (the paper's A-5.7 ends the corrections there)."""
    S, dec = dict(S), []
    if armijo:
        S["armijo"] = 1
    if ok:
        S["accepted"] = 1
        if S["soc_on"]:
            S["use_soc"], S["n_soc"] = 1, S["n_soc"] + 1
        return S, dec
    halve = True
    if S["soc_on"]:                                     # A-5.9
        more = finite and S["soc_p"] + 1 < o["max_soc"]
        if more:
            bound = o["kappa_soc"] * S["th_old_soc"]
            more = th <= bound
            dec.append(("theta_soc <= kappa_soc theta_old", more, _margin(th, bound)))
        if more:
            S["soc_p"], S["th_old_soc"], S["soc_req"] = S["soc_p"] + 1, th, 1
            halve = False
        else:
            S["soc_on"] = 0
    elif S["ls"] == 0 and o["max_soc"] > 0 and finite:  # A-5.5
        opens = th >= S["theta"]
        dec.append(("theta_trial >= theta (A-5.5)", opens, _margin(th, S["theta"])))
        if opens:
            S["soc_on"], S["soc_p"], S["th_old_soc"], S["soc_req"] = 1, 0, S["theta"], 1
            halve = False
    if not halve:
        return S, dec
    S["alpha"], S["ls"] = 0.5 * S["alpha"], S["ls"] + 1  # A-5.10
    small = S["alpha"] < S["alpha_min"]
    dec.append(("alpha < alpha_min", small, _margin(S["alpha"], S["alpha_min"])))
    if small or S["ls"] > o["max_ls"]:
        acc = S["err0"] <= o["acceptable_tol"]
        dec.append(("E_0 <= acceptable_tol", acc, _margin(S["err0"], o["acceptable_tol"])))
        if acc:
            S["status"] = 6
        else:
            infeasible = S["theta"] > o["tol"]
            dec.append(("theta > tol", infeasible, _margin(S["theta"], o["tol"])))
            if o["resto"] and infeasible:
                S["enter_resto"] = 1
            elif o["resto"] and S["n_recalc"] < o["max_recalc_y"]:
                S["enter_resto"] = 2
            else:
                S["status"] = 3
    return S, dec


def correction_constraints(c_prev, ct, mix):
    """c_soc = mix c_prev + c(trial): A-5.5 with mix = alpha and c_prev = c, A-5.9 with mix = alpha_soc and c_prev = c_soc"""
    t = LD(mix) * LD(c_prev)
    return t + LD(ct), np.abs(t).astype(np.float64) + np.abs(np.asarray(ct, dtype=np.float64))


# ------------------------------------------------------------------------------------------------------------- the step, (16), (22)
def reset_16(o, z, s, mu):
    """(16): z <- max(min(z, kappa_sigma mu / s), mu / (kappa_sigma s))"""
    ks = LD(o["kappa_sigma"])
    return np.maximum(np.minimum(z, ks * mu / s), mu / (ks * s))


def apply_step(o, vl, vu, v_new, zL, zU, lam, dlam, dzL, dzU, a, az, mu):
    """The duals after a step: lambda + a dlambda and z + az dz, then (16) with the slacks of the new point v_new (as given).
    -> dict lam, zL, zU with *_mag"""
    free, lo, up = bound_kinds(vl, vu)
    a, az, mu, v_new = LD(a), LD(az), LD(mu), LD(v_new)
    out = {"lam": LD(lam) + a * LD(dlam), "lam_mag": np.abs(lam) + np.abs(np.asarray(a * LD(dlam), dtype=np.float64))}
    for key, z, dz, here, s in (("zL", zL, dzL, lo, v_new - LD(vl)), ("zU", zU, dzU, up, LD(vu) - v_new)):
        s = np.where(here, s, LD(1))
        t = az * LD(dz)
        r = reset_16(o, LD(z) + t, s, mu)
        out[key] = np.where(here, r, LD(z))
        out[key + "_mag"] = np.where(here, np.maximum(np.abs(z) + np.abs(t).astype(np.float64), np.abs(r).astype(np.float64)), 0.0)
    return out


def filter_entry_22(o, theta, phi):
    """(22): the pair added to the filter, with magnitudes"""
    theta, phi = LD(theta), LD(phi)
    t = LD(o["gamma_phi"]) * theta
    return ((LD(1) - LD(o["gamma_theta"])) * theta, phi - t), (float(abs(theta)), float(abs(phi) + abs(t)))


# ------------------------------------------------------------------------------------------------------------- (33), (34)
def restoration_start(o, c, mu, cinf, v):
    """The start of the restoration phase (section 3.3) at the point v with constraint values c: mu_R = max(mu, |c|_inf), zeta =
    sqrt(mu_R), D_R^2 = 1 / max(1, |v|)^2, and the p, n that minimise rho sum(p + n) - mu_R sum(log p + log n) subject to
    p - n = c: (33), (34), with their multipliers z = mu_R / p, mu_R / n.  n is evaluated without cancellation:
    h + sqrt(h^2 + q) = q / (sqrt(h^2 + q) - h) for h < 0."""
    rho, c = LD(o["resto_rho"]), LD(c)
    mu_r = max(LD(mu), LD(cinf))
    h = (mu_r - rho * c) / (2 * rho)
    q = mu_r * c / (2 * rho)
    root = np.sqrt(h * h + q)
    with np.errstate(all="ignore"):
        nn = np.where(h < 0, q / np.where(h < 0, root - h, LD(1)), h + root)
    pp = c + nn
    out = dict(mu_r=mu_r, zeta=np.sqrt(mu_r), nn=nn, pp=pp, zp=mu_r / pp, zn=mu_r / nn)
    out["nn_mag"] = np.abs(h).astype(np.float64) + root.astype(np.float64)
    out["pp_mag"] = np.abs(c).astype(np.float64) + out["nn_mag"]
    sc = np.maximum(LD(1), np.abs(LD(v)))
    out["dr2"] = 1 / (sc * sc)
    return out
