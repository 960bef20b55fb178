"""Warm start of the device solver in the primal and the dual (rpm_ipm_solve_warm*, rpm_ipm_get_bound_multipliers*,
rpm_ipm_debug_start) and the refined-mesh route that feeds it (rpm_carry_multipliers_batch).

The start state is compared bit for bit with a numpy restatement of the rules in include/rpm_hip.h, written below with the
device's operation order: relaxed bounds, push_inside with the warm_start_* pushes, lambda clipped, z floored (or mu_init over
the distance to the bound), slack multipliers from the slack's stationarity, and with nlp_scaling lambda~ = (lambda sf) / sc,
z~ = z sf.  g, grad f and the Jacobian the rules need come from the engine's own host-pointer callbacks, whose bits are those of
the device-resident evaluations (smoke() pins that).  The solves are compared with a cold solve and with the primal-only restart
of test_ipm.py (mu_init 1e-6, bound_push / bound_frac 1e-9) under the bounds the issue states: status 0, the cold objective
within 1e-7, fewer iterations than cold and no more than primal-only.

Measured on the MI355X (iterations per instance, cold / primal-only / primal + dual; the tests print them, pytest -s):
  restart at the solution, quadrotor 2 x 4, B = 3, exact Hessian:     11 11 11 / 6 6 7 / 0 0 0
  the same, param_sled 2 x 12, limited-memory, B = 2:                  20 20 / - / 0 0
  the same, bryson_denham 8 x 6, nlp_scaling = 1, B = 2:               29 29 / - / 3 3
  one MPC step (initial states moved by +-0.02):                       11 11 11 / 6 7 6 / 3 3 3
  refined mesh 2 x 4 -> 3 x 6, pref (0.4, 0.8, -0.6) and the default:  11 13 / 13 12 / 4 9
"""
import ctypes as C
import os

import numpy as np
import pytest

from lpopc_amd import problems
from lpopc_amd.engine import ABI_SYMBOLS, BatchedIPM, NLPEngine, RpmError, lib
from lpopc_amd.group import SweepGroup
from lpopc_amd.problem import Options

INF = 1e19
NEW_SYMBOLS = ["rpm_ipm_solve_warm", "rpm_ipm_solve_warm_dev", "rpm_ipm_get_bound_multipliers", "rpm_ipm_get_bound_multipliers_dev",
               "rpm_ipm_debug_start", "rpm_sweep_solve_warm", "rpm_sweep_get_bound_multipliers"]
WARM_KEYS = ["warm_start_bound_push", "warm_start_bound_frac", "warm_start_slack_bound_push", "warm_start_slack_bound_frac",
             "warm_start_mult_bound_push", "warm_start_mult_init_max"]
DEFAULTS = {"bound_push": 1e-2, "bound_frac": 1e-2, "mu_init": 0.1, "bound_relax_factor": 1e-8, "warm_start_bound_push": 1e-3,
            "warm_start_bound_frac": 1e-3, "warm_start_slack_bound_push": 1e-3, "warm_start_slack_bound_frac": 1e-3,
            "warm_start_mult_bound_push": 1e-3, "warm_start_mult_init_max": 1e6, "nlp_scaling": 0, "nlp_scaling_max_gradient": 100.0}
SCAL_MIN = 1e-8
PRIMAL_ONLY = {"mu_init": 1e-6, "bound_push": 1e-9, "bound_frac": 1e-9}
WARM = {"mu_init": 1e-6, "warm_start_bound_push": 1e-9, "warm_start_bound_frac": 1e-9, "warm_start_slack_bound_push": 1e-9,
        "warm_start_slack_bound_frac": 1e-9, "warm_start_mult_bound_push": 1e-12}


def _exact():
    o = Options()
    o.SetStringValue("hessian-approximation", "exact")
    return o


# ---- without a device -------------------------------------------------------------------------------------------
def test_symbols_exist_and_are_listed(built):
    L = lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rpm_hip.h")).read()
    flat = " ".join(header.split())
    for sig in ("int rpm_ipm_solve_warm_dev(rpm_ipm* s, double* d_x, double* d_lambda, double* d_z_L, double* d_z_U, double* obj, "
                "int* status, int* iterations, double* kkt_error, void* stream);",
                "int rpm_ipm_solve_warm(rpm_ipm* s, double* x, double* lambda, double* z_L, double* z_U, double* obj, int* status, "
                "int* iterations, double* kkt_error);",
                "int rpm_ipm_get_bound_multipliers_dev(rpm_ipm* s, double* d_z_L, double* d_z_U, void* stream);",
                "int rpm_ipm_get_bound_multipliers(rpm_ipm* s, double* z_L, double* z_U);"):
        assert sig in flat, sig
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    assert L.rpm_ipm_solve_warm.argtypes == [vp, dp, dp, dp, dp, dp, ip, ip, dp]
    assert L.rpm_ipm_solve_warm_dev.argtypes == [vp, vp, vp, vp, vp, dp, ip, ip, dp, vp]
    assert L.rpm_ipm_get_bound_multipliers.argtypes == [vp, dp, dp]
    assert L.rpm_ipm_get_bound_multipliers_dev.argtypes == [vp, vp, vp, vp]
    for k in WARM_KEYS:
        assert '"%s"' % k in header, k
    # what the host decides without a solver (rpm_ipm_create needs a device; the NULL lambda / one NULL z / unknown option
    # refusals of a live solver are checked in test_one_mpc_step)
    x = np.zeros(4)
    px = x.ctypes.data_as(dp)
    assert L.rpm_ipm_solve_warm(None, px, px, px, px, None, None, None, None) == 1
    assert L.rpm_ipm_solve_warm_dev(None, None, None, None, None, None, None, None, None, None) == 1
    assert L.rpm_ipm_get_bound_multipliers(None, px, px) == 1
    assert L.rpm_sweep_solve_warm(None, px, px, None, None, None, None, None, None) == 1
    assert L.rpm_sweep_get_bound_multipliers(None, px, px) == 1


# ---- the numpy restatement of the start state ---------------------------------------------------------------------
def _push(x, l, u, lo, up, push, frac):
    with np.errstate(invalid="ignore", over="ignore"):
        pl = np.where(up, np.minimum(push * np.maximum(1.0, np.abs(l)), frac * (u - l)), push * np.maximum(1.0, np.abs(l)))
        x = np.where(lo, np.maximum(x, l + pl), x)
        pu = np.where(lo, np.minimum(push * np.maximum(1.0, np.abs(u)), frac * (u - l)), push * np.maximum(1.0, np.abs(u)))
        x = np.where(up, np.minimum(x, u - pu), x)
    return x


def _relaxed(l, u, lo, up, f):
    with np.errstate(invalid="ignore"):
        return np.where(lo, l - f * np.maximum(1.0, np.abs(l)), l), np.where(up, u + f * np.maximum(1.0, np.abs(u)), u)


def _reference_start(one, XL, XU, x0, lam, z, o, warm):
    """-> dict(v, zL, zU, lambda, mu), B rows each; `one`: a one-instance engine of the problem for g, grad f and the Jacobian.
    For the tests of the pass that follows (test_ipm_pass.py) also the relaxed bounds vl, vu (x, then the slacks) and the scaling
    factors sc, sf."""
    _, _, gl, gu = one.get_bounds_info()
    B, n, m = len(x0), one.n, one.m
    srow = np.nonzero(gl != gu)[0]
    rows, cols = one.eval_jac_g_structure()
    if rows.max() == m or cols.max() == n:          # 1-based triplets
        rows, cols = rows - 1, cols - 1
    out = {k: [] for k in ("v", "zL", "zU", "lambda", "vl", "vu", "sc", "sf")}
    floor, big = o["warm_start_mult_bound_push"], o["warm_start_mult_init_max"]
    for b in range(B):
        l, u = XL[b], XU[b]
        fixed = l == u
        lo, up = (l > -INF) & ~fixed, (u < INF) & ~fixed
        lr, ur = _relaxed(l, u, lo, up, o["bound_relax_factor"])
        push, frac = (o["warm_start_bound_push"], o["warm_start_bound_frac"]) if warm else (o["bound_push"], o["bound_frac"])
        x = np.where(fixed, l, _push(x0[b], lr, ur, lo, up, push, frac))
        sc, sf = np.ones(m), 1.0
        if o["nlp_scaling"]:
            gmax = o["nlp_scaling_max_gradient"]
            vals, grad = one.eval_jac_g(x0[b]), one.eval_grad_f(x0[b])
            keep = ~fixed[cols]
            rmax = np.zeros(m)
            np.maximum.at(rmax, rows[keep], np.abs(vals[keep]))
            with np.errstate(divide="ignore"):
                sc = np.where(rmax > gmax, np.maximum(gmax / rmax, SCAL_MIN), 1.0)
            gm = np.abs(grad[~fixed]).max()
            sf = max(gmax / gm, SCAL_MIN) if gm > gmax else 1.0
        g = one.eval_g(x)
        if o["nlp_scaling"]:
            g = g * sc
        sl, su = gl[srow], gu[srow]
        slo, sup = sl > -INF, su < INF
        with np.errstate(invalid="ignore"):
            sl, su = np.where(slo, sl * sc[srow], sl), np.where(sup, su * sc[srow], su)
        slr, sur = _relaxed(sl, su, slo, sup, o["bound_relax_factor"])
        spush, sfrac = (o["warm_start_slack_bound_push"], o["warm_start_slack_bound_frac"]) if warm else (o["bound_push"], o["bound_frac"])
        s = _push(g[srow], slr, sur, slo, sup, spush, sfrac)
        if not warm:
            lt = np.zeros(m)
            zl, zu = np.where(lo, 1.0, 0.0), np.where(up, 1.0, 0.0)
            szl, szu = np.where(slo, 1.0, 0.0), np.where(sup, 1.0, 0.0)
        else:
            lt = np.maximum(np.minimum(lam[b], big), -big)
            if o["nlp_scaling"]:
                lt = (lt * sf) / sc
            if z is not None:
                zl, zu = np.maximum(z[0][b], floor), np.maximum(z[1][b], floor)
                if o["nlp_scaling"]:
                    zl, zu = zl * sf, zu * sf
            else:
                with np.errstate(divide="ignore", invalid="ignore"):
                    zl, zu = o["mu_init"] / (x - lr), o["mu_init"] / (ur - x)
            zl, zu = np.where(lo, zl, 0.0), np.where(up, zu, 0.0)
            szl, szu = np.where(slo, np.maximum(-lt[srow], floor), 0.0), np.where(sup, np.maximum(lt[srow], floor), 0.0)
        out["v"].append(np.concatenate([x, s]))
        out["zL"].append(np.concatenate([zl, szl]))
        out["zU"].append(np.concatenate([zu, szu]))
        out["lambda"].append(lt)
        out["vl"].append(np.concatenate([np.where(fixed, l, lr), slr]))
        out["vu"].append(np.concatenate([np.where(fixed, u, ur), sur]))
        out["sc"].append(sc)
        out["sf"].append(sf)
    res = {k: np.stack(v) for k, v in out.items()}
    res["mu"] = np.full(B, o["mu_init"])
    return res


def _quadrotor_bounds(eng, B, seed=8, scale=0.2, base=None):
    """Per-instance fixed initial states as in test_ipm.py: -> (XL, XU, idx)"""
    xl, xu, _, _ = eng.get_bounds_info()
    N1 = 2 * 4 + 1
    idx = [i * N1 for i in range(12)]
    XL, XU = np.tile(xl, (B, 1)), np.tile(xu, (B, 1))
    v = np.random.RandomState(seed).uniform(-scale, scale, size=(B, 12))
    XL[:, idx] = XU[:, idx] = v if base is None else base[:, idx] + v
    return XL, XU, idx


OPEN = {}           # per problem: (variable of instance 0 without a lower bound, variable of instance 0 without an upper bound)


def _start_case(name, open_bounds=True, B=None, options=None, nested=None):
    """B, options (default: the exact Hessian), nested (engine option ipm_nested) and the launch problems: for test_ipm_pass.py"""
    if name == "quadrotor":
        prob, B0 = problems.quadrotor(2, 4), 3
    elif name == "bryson_denham":
        prob, B0 = problems.bryson_denham(2, 8), 2
    else:
        prob, B0 = {"launch_2x5": problems.launch(2, 5), "launch_16x8": problems.launch(16, 8)}[name], 2
    B = B or B0
    options = options or _exact()
    eng = NLPEngine(prob, options, n_instances=B, device=0)
    if nested is not None:
        eng.set_option("ipm_nested", nested)
    one = NLPEngine(prob, options, device=0)
    xl, xu, gl, gu = eng.get_bounds_info()
    if name == "quadrotor":
        XL, XU, _ = _quadrotor_bounds(eng, B)
    else:
        XL, XU = np.tile(xl, (B, 1)), np.tile(xu, (B, 1))
    # instance 0: one free variable without a lower bound, another without an upper bound (neither problem has one of its own)
    free = np.nonzero(xl != xu)[0]
    OPEN[name] = (int(free[-2]), int(free[-3]))
    if open_bounds:
        XL[0, OPEN[name][0]], XU[0, OPEN[name][1]] = -2e19, 2e19
    x0 = eng.get_starting_point()[:eng.n]
    X0 = np.stack([problems.seeded_iterate(x0, xl, xu, 40 + b) for b in range(B)])
    rng = np.random.RandomState(21)
    lam = rng.standard_normal((B, eng.m)) * 3.0
    z = (np.abs(rng.standard_normal((B, eng.n))) * 0.5, np.abs(rng.standard_normal((B, eng.n))) * 0.5)
    return eng, one, XL, XU, X0, lam, z


def _same_bits(got, want, rows, what):
    for k in ("v", "zL", "zU", "lambda", "mu"):
        assert np.array_equal(got[k][rows], want[k][rows]), (what, k, np.abs(got[k][rows] - want[k][rows]).max())


# ---- on the device ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["quadrotor", "bryson_denham"])
@pytest.mark.parametrize("opts", [{}, {"warm_start_bound_push": 3e-2, "warm_start_bound_frac": 2e-3, "warm_start_slack_bound_push": 0.25,
                                       "warm_start_slack_bound_frac": 5e-2, "warm_start_mult_bound_push": 0.3,
                                       "warm_start_mult_init_max": 2.5, "mu_init": 1e-3},
                                  {"nlp_scaling": 1, "nlp_scaling_max_gradient": 0.5},
                                  {"nlp_scaling": 1, "nlp_scaling_max_gradient": 0.5, "warm_start_mult_bound_push": 0.3,
                                   "warm_start_mult_init_max": 2.5, "warm_start_slack_bound_push": 0.25}],
                         ids=["defaults", "own_values", "scaled", "scaled_own_values"])
def test_start_state_bit_for_bit(built, name, opts):
    eng, one, XL, XU, X0, lam, z = _start_case(name)
    B = len(X0)
    o = dict(DEFAULTS, **opts)
    ipm = BatchedIPM(eng, **opts)
    ipm.set_all_bounds(XL, XU)
    ns = ipm.info()["n_slacks"]
    assert ns >= 1                                              # the slack rules are exercised
    every = np.arange(B)
    # the cold start through the hook is the cold start's rule
    i_lo, i_up = OPEN[name]
    assert XL[0, i_lo] < -INF and XU[0, i_up] > INF and XU[0, i_lo] < INF and XL[0, i_up] > -INF
    cold = ipm.debug_start(X0, warm=False)
    want = _reference_start(one, XL, XU, X0, None, None, o, warm=False)
    _same_bits(cold, want, every, "cold")
    assert not cold["status"].any()
    assert cold["zL"][0, i_lo] == 0.0 and cold["zU"][0, i_up] == 0.0 and cold["zU"][0, i_lo] == 1.0 and cold["zL"][0, i_up] == 1.0
    # z given / z NULL
    for zz in (z, None):
        got = ipm.debug_start(X0, lam, zz)
        want = _reference_start(one, XL, XU, X0, lam, zz, o, warm=True)
        _same_bits(got, want, every, "warm, z %s" % ("given" if zz else "NULL"))
        if o["nlp_scaling"]:                                    # the scaling is not vacuous here
            big = o["warm_start_mult_init_max"]
            assert not np.array_equal(want["lambda"], np.clip(lam, -big, big))
        assert not got["status"].any()
        assert (got["zL"][:, eng.n:] + got["zU"][:, eng.n:] > 0).all()
        assert got["zL"][0, i_lo] == 0.0 and got["zU"][0, i_up] == 0.0          # no bound, no multiplier: z given and z NULL
        assert got["zU"][0, i_lo] > 0.0 and got["zL"][0, i_up] > 0.0            # ... the other side has one
        assert (got["zL"][1:, i_lo] > 0.0).all() and (got["zU"][1:, i_up] > 0.0).all()   # ... and so have the other instances
    # injected inputs: a negative z, a z at a bound that does not exist, lambda = +-2e6, a NaN in one instance
    free = np.nonzero(XL[0] != XU[0])[0]
    with_lo = free[XL[0][free] > -INF]
    fixed = np.nonzero(XL[0] == XU[0])[0]
    lam2, zl2, zu2 = lam.copy(), z[0].copy(), z[1].copy()
    zl2[0, with_lo[0]] = -4.0
    zl2[0, i_lo] = zu2[0, i_up] = 7.0               # at bounds that do not exist
    zu2[0, fixed[0]] = 7.0                          # at a fixed variable
    lam2[0, 0], lam2[0, 1] = 2e6, -2e6
    srow = np.nonzero(one.get_bounds_info()[2] != one.get_bounds_info()[3])[0]
    lam2[0, srow[0]] = -2e6
    bad = B - 1
    lam2[bad, 3] = np.nan
    got = ipm.debug_start(X0, lam2, (zl2, zu2))
    want = _reference_start(one, XL, XU, X0, lam2, (zl2, zu2), o, warm=True)
    others = every[every != bad]
    _same_bits(got, want, others, "injected")
    assert got["status"][bad] == 5 and not got["status"][others].any()
    if not o["nlp_scaling"]:
        assert got["zL"][0, with_lo[0]] == o["warm_start_mult_bound_push"]
        assert got["lambda"][0, 0] == o["warm_start_mult_init_max"] and got["lambda"][0, 1] == -o["warm_start_mult_init_max"]
    assert got["zL"][0, i_lo] == 0.0 and got["zU"][0, i_up] == 0.0
    assert got["zU"][0, fixed[0]] == 0.0 and got["zL"][0, fixed[0]] == 0.0
    # ... and the NaN instance ends with status 5 in a solve, alone; a NaN in x or z does the same
    for where in ("lambda", "x", "z"):
        x3, lam3, zl3 = X0.copy(), lam.copy(), z[0].copy()
        {"lambda": lam3, "x": x3, "z": zl3}[where][bad, 2] = np.inf if where == "z" else np.nan
        st = ipm.debug_start(x3, lam3, (zl3, z[1]))["status"]
        assert st[bad] == 5 and not st[others].any(), where
    ipm.close()
    one.close()
    eng.close()


@pytest.mark.gpu
def test_a_nan_instance_stops_alone_in_a_warm_solve(built):
    eng, one, XL, XU, X0, lam, z = _start_case("quadrotor", open_bounds=False)
    ipm = BatchedIPM(eng)
    ipm.set_all_bounds(XL, XU)
    x0 = np.tile(eng.get_starting_point()[:eng.n], (3, 1))
    clean = ipm.solve(x0, np.zeros((3, eng.m)))
    lam0 = np.zeros((3, eng.m))
    lam0[1, 5] = np.nan
    r = ipm.solve(x0, lam0)
    assert list(r["status"]) == [0, 5, 0] and r["iterations"][1] == 0
    for b in (0, 2):
        assert np.array_equal(r["x"][b], clean["x"][b]) and r["iterations"][b] == clean["iterations"][b]
    ipm.close()
    one.close()
    eng.close()


@pytest.mark.gpu
def test_no_multiplier_where_there_is_no_bound(built):
    """rpm_ipm_get_bound_multipliers and the z a warm solve returns are 0 at an infinite bound, whatever z went in; the hook
    invalidates them."""
    import torch
    eng, one, XL, XU, X0, lam, z = _start_case("quadrotor")
    i_lo, i_up = OPEN["quadrotor"]
    ipm = BatchedIPM(eng)
    ipm.set_all_bounds(XL, XU)
    x0 = np.tile(eng.get_starting_point()[:eng.n], (3, 1))
    cold = ipm.solve(x0)
    assert (cold["status"][1:] == 0).all() and cold["status"][0] != 5

    def check(zl, zu):
        assert zl[0, i_lo] == 0.0 and zu[0, i_up] == 0.0
        assert zu[0, i_lo] > 0.0 and zl[0, i_up] > 0.0 and (zl[1:, i_lo] > 0.0).all() and (zu[1:, i_up] > 0.0).all()

    zl, zu = ipm.bound_multipliers()
    check(zl, zu)
    d_zl, d_zu = (torch.full((3, eng.n), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
    ipm.bound_multipliers_dev(d_zl, d_zu)
    torch.cuda.synchronize()
    assert np.array_equal(d_zl.cpu().numpy(), zl) and np.array_equal(d_zu.cpu().numpy(), zu)
    zl_in, zu_in = zl.copy(), zu.copy()
    zl_in[0, i_lo] = zu_in[0, i_up] = 7.0
    warm = ipm.solve(cold["x"], cold["lambda"], (zl_in, zu_in))
    check(warm["z_L"], warm["z_U"])
    check(*ipm.bound_multipliers())
    ipm.debug_start(x0, warm=False)
    with pytest.raises(RpmError):
        ipm.bound_multipliers()                                 # the hook overwrote the solve's state
    ipm.close()
    one.close()
    eng.close()


def _report(tag, cold, primal, warm):
    print("%s: iterations cold %s, primal-only %s, primal + dual %s" % ((tag,) + tuple(list(map(int, v)) for v in (cold, primal, warm))))


def _check_warm(tag, cold, primal, warm, scale):
    _report(tag, cold["iterations"], primal["iterations"], warm["iterations"])
    assert (warm["status"] == 0).all(), warm["status"]
    assert np.max(np.abs(warm["obj"] - cold["obj"])) <= 1e-7 * scale
    assert (warm["iterations"] < cold["iterations"]).all()
    assert (warm["iterations"] <= primal["iterations"]).all()


def _quadrotor_sweep():
    B = 3
    eng = NLPEngine(problems.quadrotor(2, 4), _exact(), n_instances=B, device=0)
    XL, XU, idx = _quadrotor_bounds(eng, B)
    x0 = np.tile(eng.get_starting_point()[:eng.n], (B, 1))
    return eng, XL, XU, idx, x0


@pytest.mark.gpu
def test_restart_at_the_solution(built):
    eng, XL, XU, idx, x0 = _quadrotor_sweep()
    cold_s, prim_s, warm_s = BatchedIPM(eng), BatchedIPM(eng, **PRIMAL_ONLY), BatchedIPM(eng, **WARM)
    for s in (cold_s, prim_s, warm_s):
        s.set_all_bounds(XL, XU)
    with pytest.raises(RpmError):
        cold_s.bound_multipliers()                              # nothing solved yet
    cold = cold_s.solve(x0)
    assert (cold["status"] == 0).all()
    zl, zu = cold_s.bound_multipliers()
    assert (zl >= 0).all() and (zu >= 0).all()
    assert not zl[:, idx].any() and not zu[:, idx].any()        # fixed variables
    assert (zl[:, XL[0] != XU[0]] > 0).all()                    # (every free variable here has both bounds; the ones without:
                                                                #  test_no_multiplier_where_there_is_no_bound)
    primal = prim_s.solve(cold["x"])
    warm = warm_s.solve(cold["x"], cold["lambda"], (zl, zu))
    _check_warm("restart, quadrotor 2x4 exact", cold, primal, warm, np.max(np.abs(cold["obj"])))
    for s in (cold_s, prim_s, warm_s):
        s.close()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["limited_memory", "nlp_scaling"])
def test_restart_at_the_solution_other_modes(built, which):
    if which == "limited_memory":
        eng = NLPEngine(problems.param_sled(2, 12), Options(), n_instances=2, device=0)
        extra = {}
    else:
        eng = NLPEngine(problems.bryson_denham(8, 6), _exact(), n_instances=2, device=0)
        extra = {"nlp_scaling": 1}
    x0 = np.tile(eng.get_starting_point()[:eng.n], (2, 1))
    cold_s, warm_s = BatchedIPM(eng, **extra), BatchedIPM(eng, **dict(WARM, **extra))
    cold = cold_s.solve(x0)
    assert (cold["status"] == 0).all()
    warm = warm_s.solve(cold["x"], cold["lambda"], cold_s.bound_multipliers())
    print("%s: iterations cold %s, primal + dual %s" % (which, cold["iterations"], warm["iterations"]))
    assert (warm["status"] == 0).all()
    assert (warm["iterations"] < cold["iterations"]).all()
    cold_s.close()
    warm_s.close()
    eng.close()


@pytest.mark.gpu
def test_one_mpc_step(built):
    import torch
    eng, XL, XU, idx, x0 = _quadrotor_sweep()
    B = len(x0)
    first = BatchedIPM(eng)
    first.set_all_bounds(XL, XU)
    prev = first.solve(x0)
    assert (prev["status"] == 0).all()
    z_prev = first.bound_multipliers()
    XL2, XU2, _ = _quadrotor_bounds(eng, B, seed=9, scale=0.02, base=XL)
    assert np.abs(XL2[:, idx] - XL[:, idx]).max() <= 0.02 and not np.array_equal(XL2, XL)
    cold_s, prim_s, warm_s = first, BatchedIPM(eng, **PRIMAL_ONLY), BatchedIPM(eng, **WARM)
    for s in (cold_s, prim_s, warm_s):
        s.set_all_bounds(XL2, XU2)
    cold = cold_s.solve(x0)
    assert (cold["status"] == 0).all()
    primal = prim_s.solve(prev["x"])
    warm = warm_s.solve(prev["x"], prev["lambda"], z_prev)
    _check_warm("one MPC step, quadrotor 2x4 exact", cold, primal, warm, np.max(np.abs(cold["obj"])))
    zl, zu = warm_s.bound_multipliers()
    assert np.array_equal(warm["z_L"], zl) and np.array_equal(warm["z_U"], zu)
    # the device-resident form: the same bits, and rpm_ipm_get_bound_multipliers_dev hands out what it returned
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (prev["x"], prev["lambda"], z_prev[0], z_prev[1])]
    torch.cuda.synchronize()
    rd = warm_s.solve_dev(d[0], d[1], d_z_L=d[2], d_z_U=d[3], warm=True)
    for k, t in zip(("x", "lambda", "z_L", "z_U"), d):
        assert np.array_equal(t.cpu().numpy(), warm[k]), k
    for k in ("obj", "status", "iterations", "kkt_error"):
        assert np.array_equal(rd[k], warm[k]), k
    d_zl, d_zu = torch.full_like(d[2], float("nan")), torch.full_like(d[3], float("nan"))
    warm_s.bound_multipliers_dev(d_zl, d_zu)
    torch.cuda.synchronize()
    assert np.array_equal(d_zl.cpu().numpy(), zl) and np.array_equal(d_zu.cpu().numpy(), zu)
    # host-decided argument errors of the warm entry points (the solver exists only with a device)
    L = lib()
    dp = C.POINTER(C.c_double)
    xa, la, za = (np.zeros(B * eng.n), np.zeros(B * eng.m), np.zeros(B * eng.n))
    px, pl, pz = (a.ctypes.data_as(dp) for a in (xa, la, za))
    assert L.rpm_ipm_solve_warm(warm_s._h, px, None, pz, pz, None, None, None, None) == 1
    assert b"lambda" in L.rpm_ipm_last_error(warm_s._h)
    assert L.rpm_ipm_solve_warm(warm_s._h, px, pl, pz, None, None, None, None, None) == 1
    assert b"z_L and z_U" in L.rpm_ipm_last_error(warm_s._h)
    assert L.rpm_ipm_solve_warm_dev(warm_s._h, C.c_void_p(8), None, None, None, None, None, None, None, None) == 1
    assert L.rpm_ipm_solve_warm_dev(warm_s._h, C.c_void_p(8), C.c_void_p(8), None, C.c_void_p(8), None, None, None, None, None) == 1
    assert L.rpm_ipm_get_bound_multipliers(warm_s._h, pz, None) == 1
    with pytest.raises(RpmError) as ei:
        warm_s.set_option("warm_start_target_mu", 1.0)
    assert "unknown option" in str(ei.value)
    for s in (cold_s, prim_s, warm_s):
        s.close()
    eng.close()


PREFS = [(0.4, 0.8, -0.6), (1.0, -0.5, 1.5)]                   # the second is quadrotor()'s default


def _refined_pair():
    src_p, to_p = [problems.quadrotor(2, 4, pref=p) for p in PREFS], [problems.quadrotor(3, 6, pref=p) for p in PREFS]
    src, to = (NLPEngine(ps[0], _exact(), n_instances=2, device=0) for ps in (src_p, to_p))
    for e, ps in ((src, src_p), (to, to_p)):
        e.set_instance_constants(1, ps[1].GetOpimalProblemFuns().consts)
    return src_p, to_p, src, to


@pytest.mark.gpu
def test_refined_mesh_end_to_end(built):
    src_p, to_p, src, to = _refined_pair()
    s0 = BatchedIPM(src)
    coarse = s0.solve(np.tile(src.get_starting_point()[:src.n], (2, 1)))
    assert (coarse["status"] == 0).all()
    x_c, fx = src.carry_solution_batch(to, coarse["x"])
    lam_c, fl = src.carry_multipliers_batch(to, coarse["x"], coarse["lambda"])
    assert not fx.any() and not fl.any()
    cold_s, prim_s = BatchedIPM(to), BatchedIPM(to, **PRIMAL_ONLY)
    warm_opts = {k: v for k, v in WARM.items() if k != "warm_start_mult_bound_push"}
    warm_s = BatchedIPM(to, **warm_opts)
    cold = cold_s.solve(np.tile(to.get_starting_point()[:to.n], (2, 1)))
    assert (cold["status"] == 0).all()
    primal = prim_s.solve(x_c)
    warm = warm_s.solve(x_c, lam_c)
    assert "z_L" not in warm
    _report("refined mesh 2x4 -> 3x6, quadrotor exact", cold["iterations"], primal["iterations"], warm["iterations"])
    assert (warm["status"] == 0).all()
    assert (np.abs(warm["obj"] - cold["obj"]) <= 1e-7 * np.maximum(1.0, np.abs(cold["obj"]))).all()
    assert (warm["iterations"] < cold["iterations"]).all()
    assert (warm["iterations"] <= primal["iterations"]).all()
    # the same through SweepGroup on one device: bit for bit the engine route
    L = lib()
    g_src, g_to = SweepGroup(src_p[0], [0], 2, _exact()), SweepGroup(to_p[0], [0], 2, _exact(), **warm_opts)
    for g, ps in ((g_src, src_p), (g_to, to_p)):
        c = np.ascontiguousarray(ps[1].GetOpimalProblemFuns().consts, dtype=np.float64)
        assert L.rpm_set_instance_constants(L.rpm_sweep_engine(g._h, 0), 1, c.ctypes.data_as(C.POINTER(C.c_double)), c.size) == 0
    gc = g_src.solve(np.tile(src.get_starting_point()[:src.n], (2, 1)))
    assert np.array_equal(gc["x"], coarse["x"]) and np.array_equal(gc["lambda"], coarse["lambda"])
    gx, _ = g_src.carry_solution(g_to, gc["x"])
    gl, gf = g_src.carry_multipliers(g_to, gc["x"], gc["lambda"])
    assert np.array_equal(gx, x_c) and np.array_equal(gl, lam_c) and not gf.any()
    gw = g_to.solve_warm(gx, gl)
    for k in ("x", "lambda", "obj", "status", "iterations", "kkt_error"):
        assert np.array_equal(gw[k], warm[k]), k
    gz, wz = g_to.bound_multipliers(), warm_s.bound_multipliers()
    assert np.array_equal(gz[0], wz[0]) and np.array_equal(gz[1], wz[1])
    for o in (s0, cold_s, prim_s, warm_s, g_src, g_to, src, to):
        o.close()
