"""The reference of the interior-point pass tests (tests/_ipm_pass_reference.py) checked without the kernels, on the CPU oracle's
g, J, grad f and H: the direction of its reduced system (13), completed by (12), must satisfy the UNREDUCED primal-dual system
(9), assembled here independently (dense loops over the triplets, general bounds); and its E_0 must equal a direct evaluation of
(5) and (6) with dense matrix-vector products.  Everything in long double; the bound on the relative residual is 1e-10."""
import numpy as np
import pytest

import _ipm_pass_reference as ref
from lpopc_amd import problems
from lpopc_amd.problem import Options
from oracle import oracle as orc

LD = ref.LD
CASES = {"quadrotor": lambda: problems.quadrotor(2, 4), "bryson_denham": lambda: problems.bryson_denham(2, 8)}


def _cpu_state(name, seed):
    """An interior primal-dual point of the problem as the solver holds it, from the oracle alone"""
    opts = Options()
    opts.SetStringValue("hessian-approximation", "exact")
    o = orc.Oracle(CASES[name](), opts)
    xl, xu, gl, gu = o.bounds()
    jr, jc = ref.zero_based(*o.jac_structure(), o.m, o.n)
    hr, hc = ref.zero_based(*o.hess_structure(), o.n, o.n)
    lay = ref.Layout(o.n, o.m, gl, gu, jr, jc, hr, hc)
    rng = np.random.RandomState(seed)
    relax = lambda b: 1e-8 * np.maximum(1.0, np.abs(b))

    def inside(x, l, u):
        lo, up = l > -ref.INF, u < ref.INF
        l, u = np.where(lo, l - relax(l), l), np.where(up, u + relax(u), u)
        w = np.where(lo & up, u - l, 1.0)
        x = np.where(lo, np.maximum(x, l + 1e-2 * np.minimum(1.0, w)), x)
        x = np.where(up, np.minimum(x, u - 1e-2 * np.minimum(1.0, w)), x)
        return x, l, u

    x = problems.seeded_iterate(o.starting_point(), xl, xu, seed)
    fixed = xl == xu
    x, l, u = inside(x, xl, xu)
    x, l, u = np.where(fixed, xl, x), np.where(fixed, xl, l), np.where(fixed, xu, u)
    if name == "quadrotor":                         # as the device tests: measured initial states, one open bound each side
        idx = np.array([i * 9 for i in range(12)])
        x[idx] = l[idx] = u[idx] = rng.uniform(-0.2, 0.2, 12)
    free = np.nonzero(l != u)[0]
    l[free[-2]], u[free[-3]] = -2e19, 2e19
    g = o.eval_g(x)
    s, sl, su = inside(g[lay.srow], gl[lay.srow], gu[lay.srow])
    v, vl, vu = np.concatenate([x, s]), np.concatenate([l, sl]), np.concatenate([u, su])
    _, lo, up = ref.bound_kinds(vl, vu)
    lam = rng.standard_normal(o.m) * 3.0
    zL = np.where(lo, np.abs(rng.standard_normal(lay.nv)) * 0.5 + 1e-3, 0.0)
    zU = np.where(up, np.abs(rng.standard_normal(lay.nv)) * 0.5 + 1e-3, 0.0)
    ev = {"obj": o.eval_f(x), "grad": o.eval_grad_f(x), "g": g, "jac": o.eval_jac_g(x), "hess": o.eval_h(x, 1.0, lam)}
    return lay, dict(v=v, vl=vl, vu=vu, zL=zL, zU=zU, lam=lam, gl=gl), ev


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("mu_strategy", [0, 1])
def test_reduced_step_solves_the_unreduced_system(built, name, mu_strategy):
    lay, st, ev = _cpu_state(name, 5)
    o = dict(ref.OPTS, mu_strategy=mu_strategy)
    v, vl, vu, zL, zU, lam = (st[k] for k in ("v", "vl", "vu", "zL", "zU", "lam"))
    n, nv, m = lay.n, lay.nv, lay.m
    free, lo, up = ref.bound_kinds(vl, vu)
    assert lay.ns >= 1 and (~free).any() and (free & ~lo).any() and (free & ~up).any()
    c, _ = ref.constraints(lay, v, ev["g"], st["gl"])
    glag, _, _ = ref.grad_lagrangian(lay, ev["grad"], ev["jac"], lam)
    sca, _, _ = ref.residual_scalars(lay, v, vl, vu, zL, zU, lam, c, glag)
    dec, margins = ref.decide(o, sca, LD(ev["obj"]), LD(o["mu_init"]), m)
    assert dec["status"] == 0 and min(mg for _, mg in margins) > 1e-9
    mu, delta_w = dec["mu"], LD(1e-4)
    K, _, _ = ref.kkt_13(lay, v, vl, vu, zL, zU, ev["jac"], ev["hess"], delta_w, o["delta_c"])
    assert np.array_equal(K, K.T)
    rhs, _ = ref.rhs_13(lay, v, vl, vu, glag, c, mu)
    sol = ref.solve_ld(K, rhs)
    assert ref.relative_residual(K, sol, rhs) <= 1e-15
    dv, dlam = sol[:nv], sol[nv:]
    assert (dv[~free] == 0).all()
    stp = ref.step_quantities(lay, o, v, vl, vu, zL, zU, ev["grad"], dv, mu, dec["tau"], sca["theta"], dec["theta_min"])

    # ---- the unreduced system (9), dense, over (dv, dlambda, dzL at the lower bounds, dzU at the upper bounds)
    W, A = np.zeros((nv, nv), dtype=LD), np.zeros((m, nv), dtype=LD)
    for k in range(lay.hr.size):
        i, j = int(lay.hr[k]), int(lay.hc[k])
        W[i, j] += LD(ev["hess"][k])
        if i != j:
            W[j, i] += LD(ev["hess"][k])
    for k in range(lay.jr.size):
        A[int(lay.jr[k]), int(lay.jc[k])] += LD(ev["jac"][k])
    for s_, r in enumerate(lay.srow):
        A[int(r), n + s_] = LD(-1)
    il, iu = np.nonzero(lo)[0], np.nonzero(up)[0]
    N = nv + m + il.size + iu.size
    S, r9 = np.zeros((N, N), dtype=LD), np.zeros(N, dtype=LD)
    oL, oU = nv + m, nv + m + il.size
    grad_full = np.concatenate([LD(ev["grad"]), np.zeros(lay.ns, dtype=LD)])
    stat = grad_full + A.T @ LD(lam) - LD(zL) + LD(zU)              # grad_x L with the bound multipliers
    for i in range(nv):
        if not free[i]:
            S[i, i] = 1
            continue
        S[i, :nv] = np.where(free, W[i], LD(0))
        S[i, i] += delta_w
        S[i, nv:nv + m] = A[:, i]
        r9[i] = -stat[i]
    for q, i in enumerate(il):
        S[i, oL + q] = -1
        S[oL + q, i], S[oL + q, oL + q] = LD(zL[i]), LD(v[i]) - LD(vl[i])
        r9[oL + q] = mu - (LD(v[i]) - LD(vl[i])) * LD(zL[i])
    for q, i in enumerate(iu):
        S[i, oU + q] = 1
        S[oU + q, i], S[oU + q, oU + q] = -LD(zU[i]), LD(vu[i]) - LD(v[i])
        r9[oU + q] = mu - (LD(vu[i]) - LD(v[i])) * LD(zU[i])
    S[nv:nv + m, :nv] = np.where(free[None, :], A, LD(0))
    S[nv:nv + m, nv:nv + m] = -LD(o["delta_c"]) * np.eye(m, dtype=LD)
    c_direct = LD(ev["g"]) - LD(st["gl"])                           # an equality row: g - g_l; an inequality row: g - s
    c_direct[lay.srow] = LD(ev["g"])[lay.srow] - LD(v[n:])
    r9[nv:nv + m] = -c_direct
    full = np.concatenate([dv, dlam, stp["dzL"][il], stp["dzU"][iu]])
    rel = ref.relative_residual(S, full, r9)
    print("%s mu_strategy %d: relative residual of (9) %.3g, mu %.6g" % (name, mu_strategy, rel, float(mu)))
    assert rel <= 1e-10

    # ---- E_0 by a direct evaluation of (5) and (6)
    z_all = np.concatenate([LD(zL)[il], LD(zU)[iu]])
    n_bounds = z_all.size
    s_d = max(LD(100), (np.abs(LD(lam)).sum() + z_all.sum()) / (m + n_bounds)) / 100
    s_c = max(LD(100), z_all.sum() / n_bounds) / 100
    xz =np.concatenate([(LD(v) - LD(vl))[il] * LD(zL)[il], (LD(vu) - LD(v))[iu] * LD(zU)[iu]])
    e0 = max(np.abs(stat[free]).max() / s_d, np.abs(c_direct).max(), np.abs(xz).max() / s_c)
    assert abs(e0 - dec["err0"]) <= 1e-17 * abs(e0)
    assert np.abs(c_direct - c).max() == 0 and sca["nzb"] == n_bounds
