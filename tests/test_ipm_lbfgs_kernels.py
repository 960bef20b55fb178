"""The eleven kernels of csrc/rpm_ipm_lbfgs.hip (hessian-approximation = limited-memory, lpopc's default) one by one against a
long-double reference of the same operation (tests/_lbfgs_cases.py; oracle.ipm_oracle.LimitedMemory in numpy.longdouble),
through the three test hooks rpm_ipm_debug_lbfgs_step / _state / _solve, which run the production launchers on given data:

  * the update: pair statistics, the skip / store / shift decision, the columns S, Y (bitwise), sigma and every entry of M within
    the rounding bound of their sums, at every fill level from empty to full-and-shifting, with 4 and with 16 waves per sum;
  * the skipping rule, the clamp of sigma, the gating by mode and status inside a batch;
  * the Woodbury solve (Z = K0^-1 E, C = M - E'Z, its LU with partial pivoting and the replay, the correction) against a direct
    long-double solve of K0 - E M^-1 E', on the band and the nested layout, at every fill level, and with n < 4096 <= Nt where
    the two summation layouts alternate within one solve.

All bounds come from tests/_lbfgs_cases.py (TOL is measured on the CPU: tests/test_lbfgs_reference.py, profiles/lbfgs_noise.json)."""
import numpy as np
import pytest

import _lbfgs_cases as lc

LD, H = lc.LD, lc.H
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not np.finfo(np.longdouble).eps < 2e-19, reason="numpy.longdouble is not the 80-bit type here")]


class _Solver:
    def __init__(self, name, B, nested=None):
        from lpopc_amd.engine import BatchedIPM, NLPEngine
        self.inf = lc.info(name)
        self.eng = NLPEngine(lc.PROBLEMS[name](), n_instances=B, device=0)      # default options: limited-memory
        if nested is not None:
            self.eng.set_option("ipm_nested", nested)
        self.ipm = BatchedIPM(self.eng)
        xl, xu = self.eng.get_bounds_info()[:2]
        assert (self.eng.n, self.ipm.info()["kkt_order"]) == (self.inf["n"], self.inf["nt"])
        assert np.array_equal(np.asarray(xl), self.inf["xl"]) and np.array_equal(np.asarray(xu), self.inf["xu"])
        if nested is not None:
            assert (self.ipm.subproblems().shape[0] > 1) == bool(nested)
        self.B, self.prev = B, None

    def call(self, steps, t, gates=None):
        """call t of every instance's sequence -> state after it (and the one before it in self.prev)"""
        mode = status = None
        if gates is not None:
            mode, status = (np.array([gates(bi, t)[q] for bi in range(self.B)], dtype=np.int32) for q in (0, 1))
        self.ipm.debug_lbfgs_step(*[np.stack([steps[bi][t][q] for bi in range(self.B)]) for q in range(3)], reset=t == 0, mode=mode, status=status)
        self.prev, self.state = getattr(self, "state", None), self.ipm.debug_lbfgs_state()
        return self.state

    def close(self):
        self.ipm.close()
        self.eng.close()


def _same(a, b, bi, keys=("S", "Y", "M")):
    """bit for bit (the columns beyond the pairs held are whatever the allocation held: possibly NaN patterns)"""
    return all(np.array_equal(np.ascontiguousarray(a[k][bi]).view(np.uint64), np.ascontiguousarray(b[k][bi]).view(np.uint64)) for k in keys)


def _compare(sol, bi, ref, act, what):
    """instance bi of the device state against the reference after the same call"""
    state, prev = sol.state, sol.prev
    rec, want, n = state["record"][bi], ref.record(), ref.inf["n"]
    c = want["pairs"]
    print(what, "record", rec[:6], "reference sigma %.17g" % float(want["sigma"]))
    assert [int(v) for v in rec[1:6]] == [c, want["skipped"], want["prev_valid"], want["updates"], want["skips"]], what
    assert rec[1:6].tolist() == [float(int(v)) for v in rec[1:6]]
    d_sigma = abs(LD(rec[0]) - want["sigma"])
    assert d_sigma <= ref.sigma_bound, (what, float(d_sigma), ref.sigma_bound)
    for a in range(c):                       # the reference's column order: oldest first
        assert np.array_equal(state["S"][bi, a], ref.lm.S[a].astype(np.float64)), (what, "S", a)
        assert np.array_equal(state["Y"][bi, a], ref.lm.Y[a].astype(np.float64)), (what, "Y", a)
    if c:
        assert not np.any(state["Y"][bi, :c][:, ~ref.inf["free"]])
    if ref.m_valid:
        M, bound = ref.m_and_bound()
        d = np.abs(state["M"][bi].astype(LD) - M)
        worst = float(np.max(np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), 0.0)))
        print(what, "M: largest error / bound %.3g" % worst)
        assert np.all(d <= bound), (what, worst, np.argwhere(~(d <= bound))[:4].tolist())
        dead = [q for q in range(2 * H) if q % H >= c]
        eye = np.eye(2 * H)
        assert np.array_equal(state["M"][bi][dead], eye[dead]) and np.array_equal(state["M"][bi][:, dead], eye[:, dead]), what
    if act in ("skip", "none", "frozen"):    # nothing but the counters moves
        assert _same(state, prev, bi), what
        assert rec[0] == prev["record"][bi][0] and rec[1] == prev["record"][bi][1]
    if act == "none":
        assert np.array_equal(rec[:6], prev["record"][bi][:6]), what
    if act == "frozen":
        assert _same(state, prev, bi, ("record",)), what


def _run(sol, steps, refs, upto, gates=None, what=""):
    for t in range(upto + 1):
        sol.call(steps, t, gates)
        for bi, ref in enumerate(refs):
            act = ref.step(*steps[bi][t], *(gates(bi, t) if gates else (0, 0)))
            _compare(sol, bi, ref, act, "%s call %d instance %d (%s)" % (what, t, bi, act))
    for ref in refs:
        ref.check_margins()


@pytest.mark.parametrize("name", list(lc.PROBLEMS))
def test_fill_full_shift(built, name):
    """9 good steps, B = 2 with different draws: the memory fills (call 6), is full, shifts (calls 7 to 9)."""
    sol = _Solver(name, 2)
    steps = [lc.small_steps(name, bi) for bi in range(2)]
    refs = [lc.RefInstance(sol.inf) for _ in range(2)]
    _run(sol, steps, refs, 9, what=name)
    assert [int(sol.state["record"][bi][1]) for bi in range(2)] == [6, 6] and [int(sol.state["record"][bi][4]) for bi in range(2)] == [9, 9]
    assert sol.state["record"][0][7] == H - 1 + 16           # the last store went through the shift
    sol.close()


@pytest.mark.parametrize("name", ["quadrotor_3x4", "quadrotor_32x8"])
def test_skipping_rule(built, name):
    """good, good, y = -H s (one skip: nothing else changes), good (the skip counter back to 0), skip, skip (memory emptied,
    sigma = 1, no pairs), s = 0 (nothing changes at all), y = 0 with s != 0 (a skip), three good steps."""
    sol = _Solver(name, 2)
    steps = [lc.skipping_steps(name, bi) for bi in range(2)]
    refs = [lc.RefInstance(sol.inf) for _ in range(2)]
    seen = []
    for t in range(len(lc.SKIPPING) + 1):
        sol.call(steps, t)
        for bi, ref in enumerate(refs):
            act = ref.step(*steps[bi][t])
            _compare(sol, bi, ref, act, "%s call %d instance %d (%s)" % (name, t, bi, act))
        seen.append((act, sol.state["record"][0][:6].tolist()))
    assert [a for a, _ in seen] == ["first", "store", "store", "skip", "store", "skip", "skip-empty", "none", "skip", "store", "store", "store"]
    assert seen[3][1][1:] == [2.0, 1.0, 1.0, 2.0, 1.0] and seen[4][1][1:] == [3.0, 0.0, 1.0, 3.0, 1.0]
    assert seen[6][1] == [1.0, 0.0, 0.0, 1.0, 3.0, 3.0] and seen[7][1] == seen[6][1] and seen[8][1] == [1.0, 0.0, 1.0, 1.0, 3.0, 4.0]
    assert seen[11][1][1:] == [3.0, 0.0, 1.0, 6.0, 4.0]
    for ref in refs:
        ref.check_margins()
    sol.close()


def test_sigma_clamp(built):
    name = "quadrotor_3x4"
    sol = _Solver(name, 1)
    steps = [lc.clamp_steps(name)]
    ref = lc.RefInstance(sol.inf)
    got = []
    for t in range(3):
        sol.call(steps, t)
        _compare(sol, 0, ref, ref.step(*steps[0][t]), "clamp call %d" % t)
        got.append(float(sol.state["record"][0][0]))
    assert got == [1.0, 1e8, 1e-8]
    ref.check_margins()
    sol.close()


def test_gating_in_a_batch(built):
    """B = 4: instance 1 gets mode = 2 at call 3 (memory emptied, previous iterate invalid, call 4 stores nothing, call 5 stores a
    pair from the iterate of call 4), instance 2 has status = 1 from call 4 on (frozen bitwise), instances 0 and 3 run as they run
    alone."""
    name, B, sched = lc.MIXED_PROBLEM, lc.MIXED_B, lc.GATING
    sol = _Solver(name, B)
    steps = [lc.batch_steps(bi) for bi in range(B)]
    refs = [lc.RefInstance(sol.inf) for _ in range(B)]
    states = []
    for t in range(sched["steps"] + 1):
        sol.call(steps, t, lambda bi, t_: lc.gates(sched, bi, t_))
        states.append(sol.state)
        for bi, ref in enumerate(refs):
            act = ref.step(*steps[bi][t], *lc.gates(sched, bi, t))
            _compare(sol, bi, ref, act, "gating call %d instance %d (%s)" % (t, bi, act))
    r1 = [s["record"][1][:6].tolist() for s in states]
    assert r1[2][1:4] == [2.0, 0.0, 1.0] and r1[3][:4] == [1.0, 0.0, 0.0, 0.0] and r1[4][:4] == [1.0, 0.0, 0.0, 1.0] and r1[5][1:4] == [1.0, 0.0, 1.0]
    assert np.array_equal(states[5]["S"][1, 0], steps[1][5][0] - steps[1][4][0])
    for t in range(4, sched["steps"] + 1):
        assert _same(states[t], states[3], 2) and _same(states[t], states[3], 2, ("record",))
    assert [int(states[-1]["record"][bi][1]) for bi in range(B)] == [6, 5, 3, 6]
    for ref in refs:
        ref.check_margins()
    sol.close()
    for bi in (0, 3):
        one = _Solver(name, 1)
        for t in range(sched["steps"] + 1):
            st = one.call([steps[bi]], t)
            assert np.array_equal(st["record"][0][:6], states[t]["record"][bi][:6]), (bi, t)
            c = int(st["record"][0][1])
            assert all(np.array_equal(st[k][0][:c], states[t][k][bi][:c]) for k in ("S", "Y")), (bi, t)
            if t > 0:
                assert np.array_equal(st["M"][0], states[t]["M"][bi]), (bi, t)
        one.close()


def _check_solution(d, case, what):
    d_ref = case["d_ref"]
    err = float(np.max(np.abs(d.astype(LD) - d_ref)) / np.max(np.abs(d_ref)))
    print(what, "max|d - d_ref| / max|d_ref| = %.3g (TOL %.3g)" % (err, lc.TOL))
    assert np.all(np.isfinite(d)) and err <= lc.TOL, (what, err)


@pytest.mark.parametrize("fill", lc.SMALL_FILLS)
@pytest.mark.parametrize("nested", [0, 1], ids=["band", "nested"])
@pytest.mark.parametrize("name", lc.SMALL)
def test_woodbury_solve_small(built, name, nested, fill):
    """After 1, 3, 6 and 9 steps: (K0 - E M^-1 E') d = r on the device against the long-double direct solve of the formed matrix."""
    sol = _Solver(name, 2, nested)
    inf = sol.inf
    steps = [lc.small_steps(name, bi) for bi in range(2)]
    for t in range(fill + 1):
        sol.call(steps, t)
    cases = [lc.woodbury_case("%s@%d#%d" % (name, fill, bi)) for bi in range(2)]
    for bi, case in enumerate(cases):
        assert int(sol.state["record"][bi][1]) == len(case["ref"].lm.S) == min(fill, H)
    d = sol.ipm.debug_lbfgs_solve(inf["rows"], inf["cols"], np.stack([c["vals"] for c in cases]), np.stack([c["rhs"] for c in cases]))
    for bi, case in enumerate(cases):
        _check_solution(d[bi], case, "%s %s fill %d instance %d" % (name, "nested" if nested else "band", fill, bi))
    sol.close()


@pytest.mark.parametrize("nested", [0, 1], ids=["band", "nested"])
def test_woodbury_solve_mixed_fill_levels(built, nested):
    """One batch whose instances hold 6 pairs (after two shifts), 2, 6 (never shifted) and none (the plain K0 solve)."""
    name, B, sched = lc.MIXED_PROBLEM, lc.MIXED_B, lc.MIXED
    sol = _Solver(name, B, nested)
    inf = sol.inf
    steps = [lc.batch_steps(bi) for bi in range(B)]
    for t in range(sched["steps"] + 1):
        sol.call(steps, t, lambda bi, t_: lc.gates(sched, bi, t_))
    assert tuple(int(sol.state["record"][bi][1]) for bi in range(B)) == lc.MIXED_COUNTS
    cases = [lc.woodbury_case("%s@mixed#%d" % (name, bi)) for bi in range(B)]
    d = sol.ipm.debug_lbfgs_solve(inf["rows"], inf["cols"], np.stack([c["vals"] for c in cases]), np.stack([c["rhs"] for c in cases]))
    for bi, case in enumerate(cases):
        _check_solution(d[bi], case, "mixed %s instance %d (%d pairs)" % ("nested" if nested else "band", bi, lc.MIXED_COUNTS[bi]))
    sol.close()


@pytest.mark.parametrize("name", lc.LARGE)
def test_woodbury_solve_large(built, name):
    """n >= 4096 (16 waves per sum throughout) and n < 4096 <= Nt (4-wave sums over n for M and C, 16-wave sums for E'd, sharing
    lb_part within the solve), after 7 steps, K0 diagonal with distinct values: against the closed form in long double, and the
    residual of the un-split system."""
    sol = _Solver(name, 1)
    inf = sol.inf
    assert (inf["n"] >= 4096) == (name == "quadrotor_32x8") and inf["nt"] >= 4096
    steps = [lc.large_steps(name)]
    for t in range(lc.LARGE_STEPS + 1):
        sol.call(steps, t)
    case = lc.woodbury_case("%s@%d#0" % (name, lc.LARGE_STEPS))
    assert int(sol.state["record"][0][1]) == len(case["ref"].lm.S) == H
    assert np.unique(case["vals"]).size == inf["nt"]
    idx = np.arange(inf["nt"], dtype=np.int32)
    d = sol.ipm.debug_lbfgs_solve(idx, idx, case["vals"][None, :], case["rhs"][None, :])[0]
    _check_solution(d, case, name)
    E, M, k0, r, dl = case["E"], case["M"], case["vals"].astype(LD), case["rhs"].astype(LD), d.astype(LD)
    Minv = lc.ld_solve(M, np.eye(2 * H, dtype=LD))
    res = r - k0 * dl + E @ (Minv @ (E.T @ dl))
    size = np.abs(k0) * np.abs(dl) + np.abs(E) @ (np.abs(Minv) @ (np.abs(E.T) @ np.abs(dl))) + np.abs(r)
    print(name, "residual %.3g, TOL * size %.3g" % (float(np.max(np.abs(res))), lc.TOL * float(np.max(size))))
    assert np.max(np.abs(res)) <= lc.TOL * np.max(size)
    sol.close()


def test_hooks_refuse_the_exact_hessian(built):
    from lpopc_amd.engine import RPM_E_UNSUPPORTED, BatchedIPM, NLPEngine, RpmError
    from lpopc_amd.problem import Options
    o = Options()
    o.SetStringValue("hessian-approximation", "exact")
    eng = NLPEngine(lc.PROBLEMS["brachistochrone_1x4"](), o, device=0)
    ipm = BatchedIPM(eng)
    z, nt = np.zeros((1, eng.n)), ipm.info()["kkt_order"]
    for fn in (lambda: ipm.debug_lbfgs_step(z, z, z, reset=True), ipm.debug_lbfgs_state,
               lambda: ipm.debug_lbfgs_solve(np.arange(nt), np.arange(nt), np.ones((1, nt)), np.ones((1, nt)))):
        with pytest.raises(RpmError) as ex:
            fn()
        assert ex.value.code == RPM_E_UNSUPPORTED
    ipm.close()
    eng.close()
