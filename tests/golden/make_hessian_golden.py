"""Records tests/golden/hessian/eval_h.npz: Oracle.eval_h on the HESS_CASES of tests/test_gpu_parity.py at the inputs of
test_exact_hessian (seed 5, lambda ~ U(-1,1) seed 1), sigma = 0.7 and 0, at the default step and at 1e-3, with finite-difference
and analytic first derivatives.  The committed file was recorded BEFORE orpm_eval_h and orpm_eval_h_mag were folded into one walk
(oracle/orpm_hess.c); tests/test_oracle_hessian.py::test_eval_h_is_bit_identical_to_the_recording holds the signed walk to it.

    python tests/golden/make_hessian_golden.py        (only after a deliberate change of the oracle's Hessian)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from lpopc_amd import problems  # noqa: E402
from lpopc_amd.problem import Options  # noqa: E402

CASES = {
    "bryson_denham": lambda: problems.bryson_denham(3, 5),
    "hypersensitive": lambda: problems.hypersensitive([-1, -0.5, 0.4, 1], [4, 6, 3], tf=50.0),
    "brachistochrone": lambda: problems.brachistochrone(2, 6),
    "quadrotor": lambda: problems.quadrotor(2, 4),
    "climb": lambda: problems.min_time_climb(2, 6),
    "launch": lambda: problems.launch(2, 5),
}
VARIANTS = [(step, an) for step in (None, 1e-3) for an in (False, True)]


def options(step, analytic):
    o = Options()
    o.SetStringValue("hessian-approximation", "exact")
    if step is not None:
        o.SetNumericValue("finite-difference-tol", step)
    if analytic:
        o.SetStringValue("first-derive", "analytic")
    return o


def inputs(orc):
    xl, xu, _, _ = orc.bounds()
    return problems.seeded_iterate(orc.starting_point(), xl, xu, 5), np.random.RandomState(1).uniform(-1, 1, orc.m)


def key(name, step, analytic, sigma):
    return "%s_step%s_%s_sigma%g" % (name, "default" if step is None else "%g" % step, "an" if analytic else "fd", sigma)


def record(oracle_cls):
    out = {}
    for name, make in CASES.items():
        for step, an in VARIANTS:
            orc = oracle_cls(make(), options(step, an))
            x, lam = inputs(orc)
            for sigma in (0.7, 0.0):
                out[key(name, step, an, sigma)] = orc.eval_h(x, sigma, lam)
    return out


if __name__ == "__main__":
    from oracle.oracle import Oracle
    np.savez_compressed(os.path.join(HERE, "hessian", "eval_h.npz"), **record(Oracle))
