"""One pass of the interior-point iteration on injected states (rpm_ipm_debug_start + rpm_ipm_debug_pass: the solve loop's own
steps) against the long-double reference of tests/_ipm_pass_reference.py: the residual pass (ipm_jt_lambda_kernel,
ipm_residual_kernel), the KKT assembly (rpm_kkt_assemble.hip: ipm_fill_kernel by destination through SlotValue of
rpm_kkt_slots.hpp, ipm_zero_kernel + ipm_assemble_kernel by source with the rule restated, and the two against each other bit for bit) and the direction kernel.

The comparison rule, the same everywhere:
  a single expression or a maximum     |dev - ref| <= 8 * 2^-52 * M,               M = sum of the magnitudes of its operands
  a sum of k terms                     |dev - ref| <= (k + 8) * 2^-52 * sum |term|
k is the standard bound of a sum in any order; the 8 covers one libm call (log, pow) per term and the roundings of the operands.
These are not measured figures: the smallest structural error, one missing term, is four orders of magnitude above them.  Where
the code is a copy or one IEEE operation the test asserts bit equality.  The operands of a stage are the DEVICE's results of the
stage before (its evaluations, its c and grad_x L, its mu, its dv), each checked where it is made, so no comparison depends on the
condition number of the KKT matrix.

Cases (tests/test_ipm_warm_start.py::_start_case): quadrotor(2, 4) B = 3 and bryson_denham(2, 8) B = 2 (slacks, fixed variables,
one variable without a lower and one without an upper bound), launch(2, 5) B = 2 (libm-heavy dynamics, phase links), for stage 1
launch(16, 8) B = 2 (several workgroups per instance, long Jacobian columns) and the quadrotor at B = 40 with nlp_scaling.
States: (a) interior with random lambda and z, (b) 1e-10 from the bounds with z over 1e-12 .. 1e6, (c) a converged point
re-injected, (d) a NaN in one instance's lambda.

The stage-3 solve of (13) by the unpivoted LDL^T is judged by the growth-aware rule of tests/_kkt_reference.py: with K_ref(delta_w)
of ref.kkt_13 in the order the sub-problems eliminate, its long-double factors L, D, E = |L||D||L'| and G the largest
|| |L_w^-1||L_w| ||_inf over the windows of 16 positions,  rho_E = max |K x - rhs| / (E |x| + |rhs|) <= 8 (3 Nt + 1) G 2^-53  for
every instance with G <= 1e4 (the others are printed as left out); in the band layout the factors themselves reproduce K_ref within
the same constant.  The old figure  max |K x - rhs| / (|K||x| + |rhs|)  and both figures of the float64 twin are printed
beside it (pytest -s); the figures measured on the MI355X are in DESIGN.md f-2.  The inertia ladder has a test of its own below.
"""
import numpy as np
import pytest

import _ipm_pass_reference as ref
import _kkt_reference as kr
import test_ipm_warm_start as ws
from lpopc_amd.engine import BatchedIPM, RpmError
from lpopc_amd.problem import Options

LD = ref.LD
TIGHT = {"warm_start_bound_push": 1e-10, "warm_start_bound_frac": 1e-10, "warm_start_slack_bound_push": 1e-10,
         "warm_start_slack_bound_frac": 1e-10, "warm_start_mult_bound_push": 1e-12}
SCALED = {"nlp_scaling": 1, "nlp_scaling_max_gradient": 0.5}
# option names of rpm_ipm_set_option that the reference reads under a name of its own
REF_KEYS = ("tol", "mu_init", "mu_strategy", "delta_c", "acceptable_tol", "acceptable_iter", "max_iter")


def _options(hessian):
    o = Options()
    o.SetStringValue("hessian-approximation", hessian)
    return o


class Case:
    """Engines, bounds, inputs and the solver of one case; start(): the injected state and what the reference needs beside it"""

    def __init__(self, name, opts=None, B=None, hessian="exact", nested=None):
        self.name, self.opts = name, dict(opts or {})
        self.eng, self.one, self.XL, self.XU, self.X0, self.lam, self.z = ws._start_case(name.split("@")[0], B=B, options=_options(hessian),
                                                                                          nested=nested)
        self.B, self.hessian = len(self.X0), hessian
        self.ipm = BatchedIPM(self.eng, **self.opts)
        self.ipm.set_all_bounds(self.XL, self.XU)
        e = self.one
        _, _, gl, gu = e.get_bounds_info()
        jr, jc = ref.zero_based(*e.eval_jac_g_structure(), e.m, e.n)
        hr = hc = None
        if hessian == "exact":
            hr, hc = ref.zero_based(*e.eval_h_structure(), e.n, e.n)
        self.lay = ref.Layout(e.n, e.m, gl, gu, jr, jc, hr, hc)
        self.gl = gl
        self.o = dict(ref.OPTS)
        for k in REF_KEYS:
            if k in self.opts:
                self.o[k] = self.opts[k]
        self._slots = None

    def order(self):
        """the unknowns in the order the sub-problems eliminate them (rpm_ipm_get_permutation)"""
        return np.argsort(self.ipm.permutation(), kind="stable")

    def set(self, **opts):
        for k, v in opts.items():
            self.ipm.set_option(k, v)
            self.opts[k] = v
            if k in REF_KEYS:
                self.o[k] = v

    def close(self):
        self.ipm.close()
        self.eng.close()
        self.one.close()

    def tight_inputs(self):
        """state (b): x on its bounds where they exist (the 1e-10 pushes then decide), z over 1e-14 .. 1e6 (floor 1e-12)"""
        rng = np.random.RandomState(77)
        X = self.X0.copy()
        pick = rng.randint(0, 3, size=X.shape)
        X = np.where((pick == 0) & (self.XL > -ref.INF), self.XL - 1.0, X)      # (beyond the bound: the push starts from the relaxed one)
        X = np.where((pick == 1) & (self.XU < ref.INF), self.XU + 1.0, X)
        z = tuple(10.0 ** rng.uniform(-14.0, 6.0, size=X.shape) for _ in range(2))
        return X, self.lam, z

    def start(self, X0=None, lam=None, z=None):
        X0, lam, z = (self.X0 if X0 is None else X0), (self.lam if lam is None else lam), (self.z if z is None else z)
        st = self.ipm.debug_start(X0, lam, z)
        want = ws._reference_start(self.one, self.XL, self.XU, X0, np.nan_to_num(lam), z, dict(ws.DEFAULTS, **self.opts), warm=True)
        st["vl"], st["vu"], st["sc"], st["sf"] = want["vl"], want["vu"], want["sc"], want["sf"]
        ok = st["status"] == 0
        assert ((st["vl"] <= st["v"]) & (st["v"] <= st["vu"]))[ok].all()
        return st

    def slots(self):
        """slot of every lower-triangle pair of unknowns (-1: none), once per case"""
        if self._slots is None:
            nt = self.lay.nt
            assert self.ipm.info()["kkt_order"] == nt and self.ipm.info()["n_slacks"] == self.lay.ns
            s = np.full((nt, nt), -1, dtype=np.int64)
            for a in range(nt):
                for c in range(a + 1):
                    s[a, c] = self.ipm.slot(a, c)
            self._slots = s
        return self._slots

    def rows(self, st, b):
        """instance b of a start state as the reference takes it"""
        sc = st["sc"][b]
        return dict(v=st["v"][b], vl=st["vl"][b], vu=st["vu"][b], zL=st["zL"][b], zU=st["zU"][b], lam=st["lambda"][b],
                    gl_rows=self.gl * sc if self.opts.get("nlp_scaling") else self.gl, sc=sc, sf=float(st["sf"][b]))


def _close(dev, want, tol, what):
    dev, want, tol = np.asarray(dev, dtype=np.float64), np.asarray(want), np.asarray(tol, dtype=np.float64)
    err = np.abs(LD(dev) - LD(want)).astype(np.float64)
    bad = ~(err <= tol)
    assert not bad.any(), (what, int(bad.sum()), "worst error / bound", float(np.max(err[bad] / np.maximum(tol[bad], 1e-300))),
                           "first at", np.argwhere(bad)[0].tolist())


# ---------------------------------------------------------------------------------------------------------------- stage 1
def _check_stage1(case, st, out, b, expect_status=None):
    lay, o, r = case.lay, case.o, case.rows(st, b)
    n, m = lay.n, lay.m
    I = {k: a[b] for k, a in out["inst"].items()}
    g, jac, grad, f = out["g"][b], out["jac"][b], out["grad"][b], out["obj"][b]
    tag = "%s instance %d" % (case.name, b)
    # c = g - g_l resp. g - s: entrywise, bit for bit where no scaling factor multiplies g_l
    c_ref, c_mag = ref.constraints(lay, r["v"], g, r["gl_rows"])
    _close(out["c"][b], c_ref, ref.single_tol(c_mag), tag + " c")
    if not case.opts.get("nlp_scaling"):
        want = g - case.gl
        want[lay.srow] = g[lay.srow] - r["v"][n:]
        assert np.array_equal(out["c"][b], want), tag + " c bits"
    # grad_x L: per column a sum of (entries + 1) terms; the slack columns are -lambda, a copy
    gl_ref, gl_mag, gl_cnt = ref.grad_lagrangian(lay, grad, jac, r["lam"])
    _close(out["glag"][b], gl_ref, ref.sum_tol(gl_cnt, gl_mag), tag + " glag")
    assert np.array_equal(out["glag"][b][n:], -r["lam"][lay.srow]), tag + " glag of the slacks"
    # the reduced scalars, from the device's own c and grad_x L
    args = (lay, r["v"], r["vl"], r["vu"], r["zL"], r["zU"], r["lam"])
    row_scale = r["sc"] if case.opts.get("nlp_scaling") else None
    val, mag, cnt = ref.residual_scalars(*args, out["c"][b], out["glag"][b], row_scale)
    assert I["nzb"] == val["nzb"], tag
    for k in ("theta", "dinf", "cinf", "comp_max", "comp_min", "sum_lam", "sum_z", "lnsum"):
        tol = ref.sum_tol(cnt[k], mag[k]) if k in cnt else ref.single_tol(mag[k])
        _close(I[k], val[k], tol, tag + " " + k)
    assert I["f"] == f, tag
    # the decisions: on the reference alone none is closer than 1e-9 ...
    pure, _, _ = ref.residual_scalars(*args, c_ref, gl_ref, row_scale)
    want, margins = ref.decide(o, pure, LD(f), LD(st["mu"][b]), m, r["sf"])
    tight = [mg for mg in margins if mg[1] <= 1e-9]
    assert not tight, (tag, tight)
    # ... and replayed in double from the device's own reduced scalars they give what the device left (what the record does not
    # hold — the 2-norms of the adaptive rule, the unscaled violation — from the reference)
    dev = {k: float(val[k]) for k in ("psum", "psq", "dsq", "csq", "cinf_u")}
    dev.update({k: float(I[k]) for k in ("theta", "dinf", "cinf", "comp_max", "comp_min", "sum_lam", "sum_z", "lnsum")})
    dev["nzb"], dev["nfree"] = int(I["nzb"]), val["nfree"]
    got, _ = ref.decide(o, dev, float(f), float(st["mu"][b]), m, r["sf"])
    _close(I["err0"], got["err0"], ref.single_tol(abs(got["err0"])), tag + " E_0")
    assert I["status"] == got["status"] == want["status"], (tag, I["status"], got["status"], want["status"])
    if expect_status is not None:
        assert I["status"] == expect_status, (tag, I["status"])
    assert I["n_acc"] == got["n_acc"] and I["iter"] == 0 and I["mode"] == 0, tag
    if got["status"] != 0:
        return I, got
    assert I["theta_max"] == got["theta_max"] and I["theta_min"] == got["theta_min"], tag
    assert (I["nfilt"], I["fixed_mode"], I["nrefs"]) == (0, got["fixed_mode"], got["nrefs"]), tag
    assert I["delta_w"] == 0.0 and I["refactor"] == 1, tag
    nzb = val["nzb"]
    if o["mu_strategy"] == 1 and nzb > 0:
        # avg = psum / nzb is a sum of nzb products the record does not hold: mu is checked against the rule's image of the
        # interval the sum rule leaves for avg (the rule is monotone in avg on either side of its clamps), widened by 8 ulp
        rel = float(ref.sum_tol(nzb, 1.0))
        ends = []
        for fct in (1.0 - rel, 1.0 + rel):
            d2 = dict(dev, psum=dev["psum"] * fct)
            ends.append(ref.decide(o, d2, float(f), float(st["mu"][b]), m, r["sf"])[0]["mu"])
        lo_, hi_ = min(ends) * (1.0 - 8 * ref.EPS), max(ends) * (1.0 + 8 * ref.EPS)
        assert lo_ <= I["mu"] <= hi_, (tag, "mu", I["mu"], lo_, hi_)
        _close(I["mu_max"], got["mu_max"], ref.sum_tol(nzb, got["mu_max"]), tag + " mu_max")
        _close(I["refs0"], got["refs0"], ref.sum_tol(max(nzb, m, val["nfree"]), got["refs0"]), tag + " refs[0]")
    else:
        assert ref.ulps(I["mu"], got["mu"]) <= 8, (tag, "mu", I["mu"], got["mu"], ref.ulps(I["mu"], got["mu"]))
    assert I["tau"] == max(o["tau_min"], 1.0 - I["mu"]), tag
    _close(I["phi"], LD(f) - LD(I["mu"]) * LD(I["lnsum"]), ref.single_tol(abs(f) + abs(I["mu"] * I["lnsum"])), tag + " phi")
    return I, got


def _check_scaled_evaluations(case, st, out, b):
    """nlp_scaling: what the solver holds is the engine's evaluation times sc resp. sf, one IEEE product each"""
    x, sc, sf = st["v"][b][:case.lay.n], st["sc"][b], st["sf"][b]
    one = case.one
    assert (sc < 1.0).any() and (sc == 1.0).any(), "the scaling is not vacuous"
    assert np.array_equal(out["g"][b], one.eval_g(x) * sc)
    assert np.array_equal(out["jac"][b], one.eval_jac_g(x) * sc[case.lay.jr])
    assert np.array_equal(out["grad"][b], one.eval_grad_f(x) * sf) and out["obj"][b] == one.eval_f(x) * sf


STAGE1 = [("quadrotor", {}, None), ("bryson_denham", {}, None), ("launch_2x5", {}, None), ("launch_16x8", {}, None),
          ("quadrotor@40", SCALED, 40)]


@pytest.mark.gpu
@pytest.mark.parametrize("mu_strategy", [0, 1], ids=["monotone", "adaptive"])
@pytest.mark.parametrize("state", ["interior", "at_bounds"])
@pytest.mark.parametrize("name,opts,B", STAGE1, ids=[c[0] for c in STAGE1])
def test_stage_1_residual_pass(built, name, opts, B, state, mu_strategy):
    opts = dict(opts, mu_strategy=mu_strategy, **(TIGHT if state == "at_bounds" else {}))
    case = Case(name, opts, B=B)
    lay = case.lay
    if name == "launch_16x8":
        # several workgroups per instance in the vector kernels, and columns that ipm_jt_lambda_kernel gives a workgroup each
        per_column = np.bincount(lay.jc, minlength=lay.n)
        assert lay.nv >= 4096 and case.B <= 32 and (per_column > 256).sum() >= 2 * case.eng.n_phases, (lay.nv, np.sort(per_column)[-12:])
    st = case.start(*(case.tight_inputs() if state == "at_bounds" else ()))
    assert not st["status"].any()
    if state == "at_bounds":
        free, lo, up = ref.bound_kinds(st["vl"], st["vu"])
        with np.errstate(invalid="ignore"):             # (a bound that does not exist may be infinite)
            d = np.concatenate([((st["v"] - st["vl"]) / np.maximum(1.0, np.abs(st["vl"])))[lo],
                                ((st["vu"] - st["v"]) / np.maximum(1.0, np.abs(st["vu"])))[up]])
        zz = np.concatenate([st["zL"][lo], st["zU"][up]])
        assert (d <= 2e-10).sum() >= 10 and zz.min() <= 1e-11 and zz.max() >= 1e5
    out = case.ipm.debug_pass(1)
    for b in range(case.B):
        _check_stage1(case, st, out, b)
        if opts.get("nlp_scaling") and b in (0, case.B - 1):
            _check_scaled_evaluations(case, st, out, b)
    with pytest.raises(RpmError):          # valid only directly after debug_start
        case.ipm.debug_pass(1)
    case.close()


# ---------------------------------------------------------------------------------------------------------------- stage 2
def _dense_from_storage(case, K_row):
    s = case.slots()
    used = s >= 0
    dense = np.zeros(s.shape)
    dense[used] = K_row[s[used]]
    unmapped = np.ones(K_row.size, dtype=bool)
    unmapped[s[used]] = False
    assert np.unique(s[used]).size == used.sum()           # no slot serves two entries
    return dense, used, unmapped


def _check_stage2(case, st, out, b, sigma):
    lay, o, r = case.lay, case.o, case.rows(st, b)
    nv = lay.nv
    I = {k: a[b] for k, a in out["inst"].items()}
    tag = "%s instance %d" % (case.name, b)
    hess = out["hess"][b] if case.hessian == "exact" else None
    K, M, N = ref.kkt_13(lay, r["v"], r["vl"], r["vu"], r["zL"], r["zU"], out["jac"][b], hess, I["delta_w"], o["delta_c"], sigma)
    dense, used, unmapped = _dense_from_storage(case, out["K"][b])
    low = np.tril(np.ones(K.shape, dtype=bool))
    assert not ((N > 0) & low & ~used).any(), tag + ": an entry of (13) without a slot"
    tol = np.where(N > 1, ref.sum_tol(N, M), ref.single_tol(M))
    _close(dense[used], K[used], tol[used], tag + " KKT entries")
    assert (dense[used & (N == 0)] == 0.0).all(), tag + " structural zeros"
    assert (out["K"][b][unmapped] == 0.0).all(), tag + " storage outside every slot"
    copies = used & (N == 1) & (np.arange(lay.nt)[:, None] >= nv)      # Jacobian entries, -1 of the slacks, -delta_c
    assert np.array_equal(dense[copies], K[copies].astype(np.float64)), tag + " copied slots"
    assert (I["delta_w"], I["refactor"]) == (0.0, 1), tag
    rhs, rmag = ref.rhs_13(lay, r["v"], r["vl"], r["vu"], out["glag"][b], out["c"][b], I["mu"])
    _close(out["rhs"][b], rhs, ref.single_tol(rmag), tag + " right-hand side")
    assert np.array_equal(out["rhs"][b][nv:], -out["c"][b]), tag
    return int((N > 1).sum())


def _run_stage2(name, B, nested, hessian, scaled):
    opts = dict(SCALED if scaled else {})
    case = Case(name, opts, B=B, hessian=hessian, nested=nested)
    summed = 0
    for state in ("interior", "at_bounds"):
        if state == "at_bounds":
            case.set(**TIGHT)
        inputs = case.tight_inputs() if state == "at_bounds" else ()
        st = case.start(*inputs)
        out = case.ipm.debug_pass(2)
        assert (out["inst"]["status"] == 0).all()
        sigma = None
        if hessian != "exact":
            sigma = case.ipm.debug_lbfgs_state()["record"][:, 0]
            assert (sigma > 0).all()
        for b in range(case.B):
            summed += _check_stage2(case, st, out, b, None if sigma is None else sigma[b])
        # the same state through the factorisation: level 1 assembled by the factor kernel or by the fill kernel, one direction
        fused = []
        for on in (1, 0):
            try:
                case.ipm.set_option("fused_fill", on)
            except RpmError:
                assert on == 1
                continue
            case.start(*inputs)
            fused.append((on, case.ipm.debug_pass(3)))
        case.ipm.set_option("fused_fill", 1 if len(fused) == 2 else 0)
        print("%s %s nested %d: fused level-1 assembly %s" % (name, state, nested, "compared" if len(fused) == 2 else "not available"))
        if len(fused) == 2:
            for k in ("dv", "dlam", "dzL", "dzU", "rhs", "record"):
                assert np.array_equal(fused[0][1][k], fused[1][1][k]), (name, state, k)
    if hessian == "exact":
        assert summed > 0, "no Hessian slot sums duplicates: the sum rule went unused"
    case.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scaled", [0, 1], ids=["unscaled", "nlp_scaling"])
@pytest.mark.parametrize("hessian", ["exact", "limited-memory"])
@pytest.mark.parametrize("nested", [0, 1], ids=["band", "nested"])
@pytest.mark.parametrize("name", ["quadrotor", "bryson_denham", "launch_2x5"])
def test_stage_2_kkt_assembly(built, name, nested, hessian, scaled):
    _run_stage2(name, None, nested, hessian, scaled)


@pytest.mark.gpu
@pytest.mark.parametrize("nested", [0, 1], ids=["band", "nested"])
def test_stage_2_two_kernel_assembly(built, monkeypatch, nested):
    """the other assembly path: ipm_zero_kernel + ipm_assemble_kernel, which rpm_ipm_create chooses when the one-pass fill list
    cannot be used (or RPM_IPM_TWO_PASS_FILL is set)"""
    monkeypatch.setenv("RPM_IPM_TWO_PASS_FILL", "1")
    _run_stage2("quadrotor", None, nested, "exact", 0)
    _run_stage2("bryson_denham", None, nested, "limited-memory", 1)


@pytest.mark.gpu
@pytest.mark.parametrize("hessian", ["exact", "limited-memory"])
@pytest.mark.parametrize("nested", [0, 1], ids=["band", "nested"])
@pytest.mark.parametrize("name", ["quadrotor", "bryson_denham"])
def test_stage_2_both_assembly_routes_write_the_same_bits(built, monkeypatch, name, nested, hessian):
    """the one-pass fill (by destination, SlotValue of rpm_kkt_slots.hpp) and ipm_zero_kernel + ipm_assemble_kernel (by source,
    atomic adds onto zero) state the slot rule separately: the same state leaves the same storage and right-hand side, bit for bit —
    duplicate sums and lone Hessian slots (exact), sigma on the diagonal (limited-memory), the sigma_cap branch (at_bounds)"""
    one_pass = Case(name, hessian=hessian, nested=nested)
    try:
        monkeypatch.setenv("RPM_IPM_TWO_PASS_FILL", "1")          # read when the solver is created
        two_pass = Case(name, hessian=hessian, nested=nested)
        try:
            for state in ("interior", "at_bounds"):
                outs = []
                for case in (one_pass, two_pass):
                    if state == "at_bounds":
                        case.set(**TIGHT)
                    st = case.start(*(case.tight_inputs() if state == "at_bounds" else ()))
                    assert not st["status"].any()
                    outs.append(case.ipm.debug_pass(2))
                    assert (outs[-1]["inst"]["status"] == 0).all()
                for b in range(one_pass.B):
                    assert np.array_equal(outs[0]["K"][b], outs[1]["K"][b]), (name, state, b, "K")
                    assert np.array_equal(outs[0]["rhs"][b], outs[1]["rhs"][b]), (name, state, b, "rhs")
                assert outs[0]["K"].any() and outs[0]["rhs"].any()
        finally:
            two_pass.close()
    finally:
        one_pass.close()


@pytest.mark.gpu
def test_stage_2_kkt_assembly_batch_of_40(built):
    """the quadrotor case once at B = 40, where the scaling kernels' grid switches to 16 workgroups per instance, with nlp_scaling"""
    _run_stage2("quadrotor@40", 40, 1, "exact", 1)


# ---------------------------------------------------------------------------------------------------------------- stage 3
def _check_stage3(case, st, out, b, sigma, must_run=True):
    lay, o, r = case.lay, case.o, case.rows(st, b)
    nv = lay.nv
    I = {k: a[b] for k, a in out["inst"].items()}
    tag = "%s instance %d" % (case.name, b)
    free, lo, up = ref.bound_kinds(r["vl"], r["vu"])
    dv, dlam = out["dv"][b], out["dlam"][b]
    if I["status"] != 0:                 # (the factorisation gave up on this matrix: nothing of the direction kernel to check)
        assert must_run is False, (tag, I["status"])
        return None
    assert (dv[~free] == 0.0).all(), tag + " dv at fixed unknowns"
    assert np.array_equal(dv[free], out["rhs"][b][:nv][free]) and np.array_equal(dlam, out["rhs"][b][nv:]), tag + " dv, dlam: copies"
    q = ref.step_quantities(lay, o, r["v"], r["vl"], r["vu"], r["zL"], r["zU"], out["grad"][b], dv, I["mu"], I["tau"], I["theta"],
                            I["theta_min"], dz_for_alpha=(out["dzL"][b], out["dzU"][b]))
    _close(out["dzL"][b], q["dzL"], ref.single_tol(q["dzL_mag"]), tag + " dzL")
    _close(out["dzU"][b], q["dzU"], ref.single_tol(q["dzU_mag"]), tag + " dzU")
    assert (out["dzL"][b][~lo] == 0.0).all() and (out["dzU"][b][~up] == 0.0).all(), tag
    _close(I["alpha_max"], q["alpha_max"], ref.single_tol(abs(q["alpha_max"])), tag + " alpha_max")
    _close(I["alpha_z"], q["alpha_z"], ref.single_tol(abs(q["alpha_z"])), tag + " alpha_z")
    _close(I["dphi"], q["dphi"], ref.sum_tol(q["dphi_cnt"], q["dphi_mag"]), tag + " dphi")
    amin = ref.alpha_min_23(o, LD(I["theta"]), LD(I["theta_min"]), LD(I["dphi"]))
    _close(I["alpha_min"], amin, ref.single_tol(abs(amin)), tag + " alpha_min")
    assert I["alpha"] == I["alpha_max"], tag
    assert all(I[k] == 0 for k in ("ls", "accepted", "armijo", "soc_on", "soc_req", "use_soc", "soc_p")), tag
    # how well the unpivoted LDL^T solved (13): the old figure is printed, the growth-aware rule asserted where G <= 1e4
    hess = out["hess"][b] if case.hessian == "exact" else None
    K, _, _ = ref.kkt_13(lay, r["v"], r["vl"], r["vu"], r["zL"], r["zU"], out["jac"][b], hess, I["delta_w"], o["delta_c"], sigma)
    rhs, _ = ref.rhs_13(lay, r["v"], r["vl"], r["vu"], out["glag"][b], out["c"][b], I["mu"])
    x = np.concatenate([dv, dlam])
    G = _factor_rule(case, K, rhs, x, tag)
    return ref.relative_residual(K, x, rhs), I["delta_w"], G


def _factor_rule(case, K, rhs, x, tag):
    """The rule of tests/_kkt_reference.py on one instance's solve of (13) -> G.  Asserted when G <= 1e4; an instance above it is
    printed as left out, never dropped silently.  The float64 twin's two figures are printed beside the device's."""
    order = case.order()
    Kp, bp, xp = kr.permuted(K, order), rhs[order], x[order]
    L, D = kr.ldlt(Kp)
    G = kr.block_gain(L)
    limit = kr.bound(Kp.shape[0], G)
    r, old = kr.both_measures(Kp, bp, xp, L, D)
    xt, _, _ = kr.twin_solve(Kp, bp)
    tr, told = kr.both_measures(Kp, bp, xt, L, D)
    print("%s: G %.2e bound %.2e | device rho_E %.2e old %.2e | float64 twin rho_E %.2e old %.2e%s"
          % (tag, G, limit, r, old, tr, told, "" if G <= kr.G_MAX else " | LEFT OUT of the assertion: G > 1e4"))
    if G <= kr.G_MAX:
        assert r <= limit, (tag, "rho_E", r, "bound", limit, "G", G)
    return G


STAGE3 = ["quadrotor", "bryson_denham", "launch_2x5"]
# The injected state that brings an interior instance of a (case, Hessian) inside the rule's reach, G <= 1e4, where the case's own
# state has none (DESIGN.md f-2 has the figures): the launch problem's first nodes leave multipliers whose pivot is -delta_c itself
# (Jacobian entries down to 6e-11), so it is run with the option delta_c = 1e-2 instead of 1e-9; bryson_denham with the exact Hessian
# accepts delta_w = 100 beside Jacobian entries of 1e-2, and comes into reach in the band layout with z scaled by 3e-2.
REACH_STATE = {("bryson_denham", "exact"): dict(nested=0, z_scale=3e-2), ("bryson_denham", "limited-memory"): dict(nested=0),
               ("launch_2x5", "exact"): dict(nested=1, delta_c=1e-2), ("launch_2x5", "limited-memory"): dict(nested=1, delta_c=1e-2)}


def _adjusted_case(name, hessian, nested, z_scale=1.0, delta_c=None):
    """a case with the adjusted injected state -> (case, start state)"""
    case = Case(name, {} if delta_c is None else {"delta_c": delta_c}, hessian=hessian, nested=nested)
    st = case.start(z=(case.z[0] * z_scale, case.z[1] * z_scale))
    assert not st["status"].any()
    return case, st


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["interior", "at_bounds"])
@pytest.mark.parametrize("hessian", ["exact", "limited-memory"])
@pytest.mark.parametrize("name", STAGE3)
def test_stage_3_direction(built, name, hessian, state):
    opts = dict(TIGHT if state == "at_bounds" else {})
    case = Case(name, opts, hessian=hessian)
    st = case.start(*(case.tight_inputs() if state == "at_bounds" else ()))
    out = case.ipm.debug_pass(3)
    sigma = case.ipm.debug_lbfgs_state()["record"][:, 0] if hessian != "exact" else None
    worst = []
    for b in range(case.B):
        worst.append(_check_stage3(case, st, out, b, None if sigma is None else sigma[b], must_run=state == "interior"))
    assert any(w is not None for w in worst)
    print("stage-3 residual %s %s %s: %s" % (name, hessian, state,
                                             ", ".join("gave up" if w is None else "%.2e (delta_w %.1e, G %.1e)" % w for w in worst)))
    case.close()
    if state == "interior":
        # the precondition: an interior instance of every (case, Hessian) inside the rule's reach — the case's own state or, where
        # that has none, the adjusted one of REACH_STATE, judged the same way
        reach = [w[2] for w in worst if w is not None]
        if min(reach) > kr.G_MAX and (name, hessian) in REACH_STATE:
            other, st = _adjusted_case(name, hessian, **REACH_STATE[(name, hessian)])
            out = other.ipm.debug_pass(3)
            sigma = other.ipm.debug_lbfgs_state()["record"][:, 0] if hessian != "exact" else None
            reach += [_check_stage3(other, st, out, b, None if sigma is None else sigma[b])[2] for b in range(other.B)]
            other.close()
        assert min(reach) <= kr.G_MAX, (name, hessian, reach)


# the band layout's states with an instance whose own factors have G <= 1e4 (the input condition, here on the device's factors)
BAND_STATE = {("quadrotor", "exact"): dict(delta_c=1e-2), ("quadrotor", "limited-memory"): dict(delta_c=1e-2),
              ("bryson_denham", "exact"): dict(z_scale=3e-2), ("bryson_denham", "limited-memory"): dict(),
              ("launch_2x5", "exact"): dict(delta_c=1e-2), ("launch_2x5", "limited-memory"): dict(delta_c=1e-2)}


@pytest.mark.gpu
@pytest.mark.parametrize("hessian", ["exact", "limited-memory"])
@pytest.mark.parametrize("name", STAGE3)
def test_stage_3_band_factors_reproduce_the_matrix(built, name, hessian):
    """Band + border layout, interior state (BAND_STATE): the factors a stage-3 pass leaves in the storage (L11^-1 of every 16 x 16
    diagonal block inverted back in long double) reproduce K_ref at the accepted delta_w,  |L D L' - K_ref| <= 8 (3 Nt + 1) G 2^-53
    |L||D||L'|  entrywise, G and E of the device's own factors, for every instance with G <= 1e4 — at least one per case; an
    instance above it is printed as left out."""
    case, st = _adjusted_case(name, hessian, 0, **BAND_STATE[(name, hessian)])
    out = case.ipm.debug_pass(3)
    assert (out["inst"]["status"] == 0).all()
    assert np.array_equal(case.ipm.debug_storage().view(np.uint64), out["K"].view(np.uint64))     # the read-only hook: the same storage
    sigma = case.ipm.debug_lbfgs_state()["record"][:, 0] if hessian != "exact" else None
    info, order = case.ipm.info(), case.order()
    lay, o = case.lay, case.o
    asserted = 0
    for b in range(case.B):
        r = case.rows(st, b)
        hess = out["hess"][b] if hessian == "exact" else None
        K, _, _ = ref.kkt_13(lay, r["v"], r["vl"], r["vu"], r["zL"], r["zU"], out["jac"][b], hess, out["inst"]["delta_w"][b], o["delta_c"],
                             None if sigma is None else sigma[b])
        Ld, Dd = kr.band_border_factors(out["K"][b], lay.nt, info["band_order"], info["half_bandwidth"])
        Gd = kr.block_gain(Ld)
        err = kr.reconstruction_error(Ld, Dd, kr.permuted(K, order))
        print("%s %s instance %d: delta_w %.1e, G of the device's factors %.2e, |L D L' - K| / E %.2e (bound %.2e)%s"
              % (name, hessian, b, out["inst"]["delta_w"][b], Gd, err, kr.bound(lay.nt, Gd),
                 "" if Gd <= kr.G_MAX else " | LEFT OUT of the assertion: G > 1e4"))
        if Gd <= kr.G_MAX:
            assert err <= kr.bound(lay.nt, Gd), (name, hessian, b, err, Gd)
            asserted += 1
    assert asserted >= 1, (name, hessian)
    case.close()


def _rungs(o, count=12):
    """delta_w of Algorithm IC after debug_start (delta_w_last = 0): 0, delta_w_first, then times kw_inc_first (the defaults of
    IpmOpts, carried by the reference's option table), the device's own products"""
    out = [0.0, o["delta_w_first"]]
    while len(out) < count:
        out.append(out[-1] * o["kw_inc_first"])
    return out


# (case, layout, delta_c).  At the production delta_c = 1e-9 the quadrotor in the nested layout has every rung decided.  In the band
# layout, and for the launch problem in both, multipliers whose pivot is -delta_c itself put G at 2e5 .. 1e11 and every margin below
# 2e-3: those three run with the option delta_c = 1, where every rung of every instance has a margin above 1e3.
LADDER = [("quadrotor", 1, 1e-9), ("quadrotor", 0, 1.0), ("launch_2x5", 0, 1.0), ("launch_2x5", 1, 1.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,nested,delta_c", LADDER, ids=["%s-%s-delta_c_%g" % (n, "nested" if k else "band", d) for n, k, d in LADDER])
def test_stage_3_inertia_ladder_stops_at_the_first_right_rung(built, name, nested, delta_c):
    """Exact Hessian, interior states, the random lambda of the cases (W indefinite): the accepted delta_w is a rung of the ladder;
    by the long-double factors of K_ref(rung) the inertia is wrong at every rung before it and (nv, m, 0) at it; the record says
    so.  A rung whose smallest pivot margin |D_k| / (bound E_kk) is below 100 is undecided — the device may go either way there:
    at most one in ten of the rungs checked, and at least one instance of the case has none."""
    case, st = _adjusted_case(name, "exact", nested, delta_c=delta_c)
    out = case.ipm.debug_pass(3)
    lay, o, order, rungs = case.lay, case.o, case.order(), _rungs(case.o)
    assert o["delta_c"] == delta_c
    checked = undecided = clean = 0
    for b in range(case.B):
        I = {k: a[b] for k, a in out["inst"].items()}
        r = case.rows(st, b)
        tag = "%s nested %d instance %d" % (name, nested, b)
        assert I["status"] == 0, tag
        assert I["delta_w"] in rungs, (tag, I["delta_w"])
        last = rungs.index(I["delta_w"])
        assert last >= 1, tag + ": W is not indefinite, the ladder was not climbed"
        here = 0
        for k in range(last + 1):
            K, _, _ = ref.kkt_13(lay, r["v"], r["vl"], r["vu"], r["zL"], r["zU"], out["jac"][b], out["hess"][b], rungs[k], o["delta_c"])
            L, D = kr.ldlt(kr.permuted(K, order))
            G = kr.block_gain(L)
            counts, margin = kr.inertia(D, kr.growth_diagonal(L, D), kr.bound(lay.nt, G))
            checked += 1
            print("%s rung %d delta_w %.1e: reference inertia %s, G %.2e, margin %.2e%s" % (tag, k, rungs[k], counts, G, margin,
                                                                                        "" if margin >= kr.MARGIN_MIN else " UNDECIDED"))
            if margin < kr.MARGIN_MIN:
                here += 1
                continue
            assert (counts == (lay.nv, lay.m, 0)) == (k == last), (tag, k, counts)
        undecided += here
        clean += here == 0
        assert (I["npos"], I["nneg"], I["nbad"], I["refactor"]) == (lay.nv, lay.m, 0, 0), tag
        assert I["delta_w_last"] == I["delta_w"], tag
    print("%s nested %d: %d of %d rungs undecided, %d of %d instances with none" % (name, nested, undecided, checked, clean, case.B))
    assert 10 * undecided <= checked and clean >= 1, (name, nested, undecided, checked, clean)
    case.close()


# ---------------------------------------------------------------------------------------------------------------- states (c), (d)
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["quadrotor", "bryson_denham"])
def test_converged_point_reinjected(built, name):
    """(c): the (x, lambda, z) of a real solve, pushed by 1e-12 only.  With mu_init = 1e-9 the pass ends it: status 1, E_0 <= tol.
    The termination test precedes the barrier update, so the monotone rule is seen on the same point with tol = 1e-12, which
    no longer ends it: from mu_init = 0.1 it must fall more than once in the single pass."""
    case = Case(name)
    case.start()                                   # (an injected state that the solve below replaces)
    sol = case.ipm.solve(case.X0)
    assert (sol["status"] == 0).all()
    with pytest.raises(RpmError, match="directly after rpm_ipm_debug_start"):      # a solve's state is no injected state
        case.ipm.debug_pass(1)
    with pytest.raises(RpmError, match="stage 1, 2 or 3"):
        case.ipm.debug_pass(4)
    z = case.ipm.bound_multipliers()
    case.set(**dict({k: 1e-12 for k in TIGHT}, mu_init=1e-9))
    st = case.start(sol["x"], sol["lambda"], z)
    out = case.ipm.debug_pass(1)
    for b in range(case.B):
        I, _ = _check_stage1(case, st, out, b, expect_status=1)
        assert I["err0"] <= case.o["tol"]
    case.set(mu_strategy=0, mu_init=0.1, tol=1e-12)
    st = case.start(sol["x"], sol["lambda"], z)
    out = case.ipm.debug_pass(1)
    for b in range(case.B):
        I, got = _check_stage1(case, st, out, b, expect_status=0)
        assert got["falls"] > 1 and I["mu"] < 0.02, (b, got["falls"], I["mu"])
        print("%s instance %d: mu fell %d times to %.3e" % (name, b, got["falls"], I["mu"]))
    case.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["quadrotor", "launch_2x5"])
def test_nan_instance_touches_no_other(built, name):
    """(d): a NaN in one instance's lambda ends that instance with status 5; every other instance is bit-identical, through the
    direction kernel, to the batch without it"""
    case = Case(name)
    bad = case.B - 1
    keys = ("obj", "grad", "g", "jac", "c", "glag", "hess", "K", "rhs", "dv", "dlam", "dzL", "dzU", "record")
    lam = case.lam.copy()
    lam[bad, 3] = np.nan
    for stage in (1, 3):
        case.start()
        clean = case.ipm.debug_pass(stage)
        st = case.start(lam=lam)
        assert st["status"][bad] == 5 and not st["status"][:bad].any()
        out = case.ipm.debug_pass(stage)
        assert out["inst"]["status"][bad] == 5 and not out["inst"]["status"][:bad].any()
        for k in keys:          # (bit patterns: what a stage leaves untouched is NaN on both sides)
            assert np.array_equal(out[k][:bad].view(np.uint64), clean[k][:bad].view(np.uint64)), (stage, k)
        if stage == 1:
            for b in range(bad):
                _check_stage1(case, st, out, b, expect_status=0)
    case.close()
