"""The CPU side of the limited-memory BFGS kernel tests (tests/_lbfgs_cases.py; the device side is test_ipm_lbfgs_kernels.py):

  * oracle.ipm_oracle.LimitedMemory in long double: B from the compact representation equals the explicit BFGS recursion,
    the history shifts oldest-first, two skips in a row empty it;
  * every decision of the skipping rule in every sequence the device tests run is at least 1e-3 (as a cosine) away from the
    threshold, so rounding cannot flip one;
  * TOL of the Woodbury tests is what the perturbation model gives (re-measured here) and what profiles/lbfgs_noise.json says;
    plain float64 Woodbury stays below TOL / 16 against long double; cond(K), cond(C) <= 1e3 in every case.
"""
import json
import os

import numpy as np
import pytest

import _lbfgs_cases as lc
from oracle.ipm_oracle import LimitedMemory

HERE = os.path.dirname(os.path.abspath(__file__))
LD = lc.LD

pytestmark = pytest.mark.skipif(not np.finfo(np.longdouble).eps < 2e-19, reason="numpy.longdouble is not the 80-bit type here")


def test_long_double_elimination():
    rng = np.random.RandomState(0)
    A, X = rng.uniform(-1, 1, (40, 40)), rng.uniform(-1, 1, (40, 3))
    A[0, 0] = 0.0                                        # needs the row interchange
    got = lc.ld_solve(A, A.astype(LD) @ X.astype(LD))
    assert got.dtype == LD and np.max(np.abs(got - X)) <= 1e-15
    assert np.max(np.abs(lc.ld_solve(A, (A.astype(LD) @ X.astype(LD))[:, 1]) - X[:, 1])) <= 1e-15


@pytest.mark.parametrize("pairs", [1, 4, 6, 9])
def test_compact_form_equals_the_bfgs_recursion(pairs):
    """B = sigma I - Q M^-1 Q' over the pairs held against  B <- B - B s s'B / s'B s + y y' / y's  from B = sigma I, in long double."""
    n = 30
    rng = np.random.RandomState(pairs)
    hd = rng.uniform(1, 30, n)
    lm = LimitedMemory(n, dtype=LD)
    given = []
    for _ in range(pairs):
        s = rng.uniform(-1, 1, n)
        given.append((s.astype(LD), (hd * s + 3.0 * s.sum() / n).astype(LD)))
        assert lm.update(*given[-1]) == "store"
    held = given[-6:]
    assert len(lm.S) == len(held) == min(pairs, 6) and lm.updates == pairs
    for (s, y), s_held, y_held in zip(held, lm.S, lm.Y):             # oldest first
        assert np.array_equal(s, s_held) and np.array_equal(y, y_held)
    s, y = held[-1]
    assert lm.sigma == (s @ y) / (s @ s)
    B = lm.sigma * np.eye(n, dtype=LD)
    for s, y in held:
        Bs = B @ s
        B = B - np.outer(Bs, Bs) / (s @ Bs) + np.outer(y, y) / (y @ s)
    got = lm.matrix(lc.ld_solve)
    assert got.dtype == LD
    assert np.max(np.abs(got - B)) <= 1e-16 * np.max(np.abs(B))
    # and in float64 the class is what solve() runs: same numbers to float64 rounding
    lm64 = LimitedMemory(n)
    for s, y in given:
        lm64.update(s.astype(np.float64), y.astype(np.float64))
    assert np.max(np.abs(lm64.matrix() - B.astype(np.float64))) <= 1e-12 * float(np.max(np.abs(B)))


def test_skipping_rule_of_the_class():
    n = 12
    rng = np.random.RandomState(3)
    lm = LimitedMemory(n, dtype=LD)
    s = rng.uniform(-1, 1, n).astype(LD)
    assert lm.update(s, 2 * s) == "store" and lm.update(s, 3 * s) == "store" and abs(lm.sigma - 3) <= 1e-18
    assert lm.update(s, -s) == "skip" and (len(lm.S), lm.skipped) == (2, 1) and abs(lm.sigma - 3) <= 1e-18
    assert lm.update(0 * s, s) == "none" and (len(lm.S), lm.skipped) == (2, 1)
    assert lm.update(s, s) == "store" and lm.skipped == 0
    assert lm.update(s, 0 * s) == "skip" and lm.update(s, -s) == "skip-empty"
    assert (len(lm.S), lm.skipped, lm.sigma, lm.updates, lm.skips) == (0, 0, 1, 3, 3)
    assert lm.update(s, 1e9 * s) == "store" and lm.sigma == LD(1e8)
    assert lm.update(s, 1e-9 * s) == "store" and lm.sigma == LD(1e-8)
    lm.prev = s
    lm.empty()
    assert lm.prev is None and not lm.S and lm.sigma == 1 and lm.updates == 5


def _actions(ref):
    return [a for a, _ in ref.log]


def test_decisions_keep_their_margin(built):
    """Every sequence of the device tests, on the reference alone."""
    for name in lc.PROBLEMS:
        for bi in range(2):
            ref = lc.run_reference(lc.info(name), lc.small_steps(name, bi))
            ref.check_margins()
            assert _actions(ref) == ["first"] + ["store"] * 9
            assert min(c for a, c in ref.log if a == "store") > 0.5           # the SPD model: 0.76 to 0.82
    for name in ("quadrotor_3x4", "quadrotor_32x8"):
        for bi in range(2):
            ref = lc.run_reference(lc.info(name), lc.skipping_steps(name, bi))
            ref.check_margins()
            assert _actions(ref) == ["first", "store", "store", "skip", "store", "skip", "skip-empty", "none", "skip", "store", "store", "store"]
    ref = lc.run_reference(lc.info("quadrotor_3x4"), lc.clamp_steps("quadrotor_3x4"))
    ref.check_margins()
    assert _actions(ref) == ["first", "store", "store"] and ref.lm.sigma == LD(1e-8)
    for schedule, counts in ((lc.GATING, (6, 5, 3, 6)), (lc.MIXED, lc.MIXED_COUNTS)):
        for bi in range(lc.MIXED_B):
            ref = lc.run_batch_reference(schedule, bi)
            ref.check_margins()
            assert len(ref.lm.S) == counts[bi]
    acts = _actions(lc.run_batch_reference(lc.GATING, 1))
    assert acts[3:6] == ["emptied", "first", "store"]
    assert _actions(lc.run_batch_reference(lc.GATING, 2))[4:] == ["frozen"] * 6


def test_fixed_variables_are_masked(built):
    """The inputs do exercise the mask: glag_new - glag_old is far from 0 at the fixed variables, y is 0 there."""
    inf = lc.info("quadrotor_3x4")
    assert int((~inf["free"]).sum()) == 14
    ref = lc.run_reference(inf, lc.small_steps("quadrotor_3x4", 0))
    for x, g1, g0 in lc.small_steps("quadrotor_3x4", 0):
        assert np.all(np.abs(g1 - g0)[~inf["free"]] >= 0.4) and np.array_equal(x[~inf["free"]], inf["xl"][~inf["free"]])
    assert all(not np.any(y[~inf["free"]]) and not np.any(s[~inf["free"]]) for s, y in zip(ref.lm.S, ref.lm.Y))


@pytest.fixture(scope="module")
def measured(built):
    return lc.measure_all()


def test_tolerance_is_the_measured_one(measured):
    figures = {k: v["figure"] for k, v in measured.items()}
    print("figure per case:", {k: "%.3g" % v for k, v in figures.items()})
    assert lc.TOL == lc.tol_from(figures.values()), (lc.TOL, max(figures.values()))
    with open(os.path.join(HERE, "..", "profiles", "lbfgs_noise.json")) as f:
        prof = json.load(f)
    assert prof["TOL"] == lc.TOL and prof["K0_solve_bound"] == lc.K0_SOLVE_BOUND and prof["draws"] == lc.NOISE_DRAWS
    assert sorted(prof["cases"]) == sorted(k[0] for k in lc.case_keys())
    assert prof["TOL"] == lc.tol_from(v["figure"] for v in prof["cases"].values())
    for key, got in measured.items():                    # the file says what this machine measures (it keeps 4 digits)
        for q in ("figure", "cond_K", "cond_C"):
            assert abs(prof["cases"][key][q] - got[q]) <= 1e-2 * got[q], (key, q, got[q])


def test_float64_woodbury_and_conditioning(measured):
    """The identity itself loses nothing (float64 numpy against the long-double direct solve: far below TOL), and no case can
    hide a failure behind ill-conditioning."""
    for key, got in measured.items():
        assert got["woodbury_f64"] <= lc.TOL / 16, (key, got)
        assert got["cond_K"] <= lc.COND_CAP and got["cond_C"] <= lc.COND_CAP, (key, got)
