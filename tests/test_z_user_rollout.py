"""The roll-out in a user-problem library: examples/user_problem_vanderpol.hpp, built through lpopc_amd.userproblem.build as
test_z_user_problem.py builds it, carries rpm_rollout_kernel for its own functor.  3 instances on a 2 x 4 mesh against the
restatement of test_sweep_rollout.py with the Van der Pol right-hand side; the bound is the project's,
1e-12 * max(1, max|reference column|), its worst figure printed first.  The right-hand side calls no libm, and on the MI355X every
figure came out 0.00e+00: equal bits are asserted, as in test_sweep_rollout.py."""
import numpy as np
import pytest

import test_sweep_carry as sc
import test_sweep_rollout as sr
import test_sweep_shift as ss
import test_z_user_problem as zu
from lpopc_amd.engine import NLPEngine


def f_vanderpol(t, y, u, par, c):
    return np.array([(1.0 - y[1] * y[1]) * y[0] - y[1] + u[0],
                     y[0]])


@pytest.mark.gpu
def test_a_user_library_rolls_out_its_own_dynamics(built):
    B = 3
    probs = [zu._vanderpol(2, 4) for _ in range(B)]
    xs = sc._iterates(probs)
    eng = NLPEngine(probs[0], n_instances=B, device=0)
    for s in sr.NEW_SYMBOLS:
        assert hasattr(eng._L, s), s
    ph = ss._phases(eng)[0][0]
    t0, tf = sr._t0tf(ph, xs)
    dt = np.array([0.05, 1.0, -0.1]) * (tf - t0)                         # inside the horizon, all of it, backwards
    worst, equal = 0.0, True
    for n_steps in sr.STEPS:
        for hold in (0, 1):
            for kind in (0, 3):
                s0, ts = sr._starts_of(kind, ph, xs)
                ref = sr._rollout_ref(f_vanderpol, ph, xs, dt, n_steps, hold, s0, ts, [np.array([1.0])] * B)
                got = eng.rollout_batch(0, xs, dt, n_steps, hold, s0, ts, traj=True)
                what = ("vanderpol", n_steps, hold, kind)
                worst = max(worst, sr._close(got["state"][:, :, None], ref["state"][:, :, None], what),
                            sr._close(got["traj"].swapaxes(1, 2), ref["traj"].swapaxes(1, 2), what))
                assert np.array_equal(got["nonfinite"], ref["nonfinite"]), what
                equal = equal and all(np.array_equal(got[k], ref[k], equal_nan=True) for k in sr.KEYS)
    print("vanderpol: worst |roll-out - restatement| / max(1, max|column|): %.2e (bound 1e-12); equal to the bit: %s" % (worst, equal))
    assert equal
    times = sr._sample_times(ph, xs)
    got, flags = eng.sample_plan_batch(0, xs, times)
    assert np.array_equal(got, sr._sample_ref(ph, xs, times)[0]) and not flags.any()
    eng.close()
