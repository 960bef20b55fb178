"""Shared by test_ipm_batch_sizes.py: the sweeps whose instances differ (constants, bounds, starts, a few special instances), the
positions at which an instance of a batch is compared with a one-instance solve, and bit-for-bit comparison of whole results.

Everything here is a function of the instance index alone, so the first B instances of a sweep are the same whatever B is."""
import functools

import numpy as np

from lpopc_amd import problems
from lpopc_amd.problem import Options
from oracle import ipm_oracle
from oracle import oracle as orc

FLOATS = ("x", "lambda", "obj", "kkt_error", "z_L", "z_U")
INTS = ("status", "iterations", "restorations")

# the quadrotor sweep's special instances: starts at its own solution / NaN in x0 / NaN bound (32 is the last of B = 33)
EARLY, NAN_X0, NAN_BOUND = 5, 17, 32
SPECIAL = (EARLY, NAN_X0, NAN_BOUND)


def exact():
    o = Options()
    o.SetStringValue("hessian-approximation", "exact")
    return o


def picks(B, special=()):
    """At most 12 positions: both sides of every block edge of the table in DESIGN.md (32, 64, 256), the ends, the special ones."""
    edge = [p for p in (0, 1, 31, 32, 63, 64, 255, 256, B - 2, B - 1) if 0 <= p < B]
    out = sorted(set(edge) | set(p for p in special if p < B))
    if len(out) > 12:                      # the specials stay; of the edges, the far side of each goes first
        for drop in (63, 255, 1):
            if len(out) > 12 and drop in out and drop not in special:
                out.remove(drop)
    assert len(out) <= 12
    return out


def same_bits(a, b):
    """Bit for bit (a NaN equals the same NaN, -0.0 does not equal 0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    return bool(np.array_equal(a, b))


def run(ipm, x0, lam0=None, z0=None):
    """One solve and everything the solver reports about it, per instance."""
    r = ipm.solve(x0, lam0, z0)
    zl, zu = ipm.bound_multipliers()
    B = r["x"].shape[0]
    out = {k: r[k] for k in ("x", "lambda", "obj", "status", "iterations", "kkt_error")}
    out["z_L"], out["z_U"] = (r["z_L"], r["z_U"]) if "z_L" in r else (zl, zu)
    if "z_L" in r:                          # a warm solve hands back what rpm_ipm_get_bound_multipliers reports
        assert same_bits(r["z_L"], zl) and same_bits(r["z_U"], zu)
    out["restorations"] = ipm.restorations().copy()
    out["trace"] = [ipm.trace(bi, capacity=512) for bi in range(B)]
    out["stats"] = ipm.stats()
    return out


def differences(a, ia, b, ib):
    """Names of the result fields in which instance ia of a and instance ib of b differ."""
    bad = [k for k in FLOATS + INTS if not same_bits(a[k][ia], b[k][ib])]
    if not same_bits(a["trace"][ia], b["trace"][ib]):
        ta, tb = a["trace"][ia], b["trace"][ib]
        rows = min(len(ta), len(tb))
        first = next((k for k in range(rows) if not same_bits(ta[k], tb[k])), rows)
        bad.append("trace (first differing row %d of %d / %d)" % (first, len(ta), len(tb)))
    return bad


def assert_same(a, ia, b, ib, what):
    bad = differences(a, ia, b, ib)
    assert not bad, (what, ia, ib, bad, int(a["status"][ia]), int(b["status"][ib]), int(a["iterations"][ia]), int(b["iterations"][ib]))


def assert_permuted(first, second, perm, what):
    """second solved the instances of first in the order perm: second[k] is first[perm[k]]."""
    for k, bi in enumerate(perm):
        assert_same(first, int(bi), second, k, what)


def permuted(perm, *arrays):
    return [None if a is None else np.ascontiguousarray(a[perm]) for a in arrays]


# ---------------------------------------------------------------------------------------------- the quadrotor sweep
N1 = 2 * 4 + 1
STATE0 = [i * N1 for i in range(12)]          # X(0, state) of the 12 states of quadrotor(2, 4)


def quadrotor_prefs(B):
    rng = np.random.RandomState(3)            # drawn as in test_ipm.py::test_sweep_with_per_instance_targets
    return [tuple(rng.uniform(-1.0, 1.0, size=3)) for _ in range(B)]


def quadrotor_problem(pref=None):
    return problems.quadrotor(2, 4) if pref is None else problems.quadrotor(2, 4, pref=pref)


@functools.lru_cache(maxsize=None)
def _quadrotor_base():
    o = orc.Oracle(quadrotor_problem(), exact())
    xl, xu, _, _ = o.bounds()
    return o.starting_point(), xl, xu


@functools.lru_cache(maxsize=None)
def _early_start(seed):
    """The converged solution of instance EARLY's own problem (the restatement's, so that it is there without a GPU)."""
    s = _quadrotor_plain(EARLY + 1, seed)
    o = orc.Oracle(quadrotor_problem(s["prefs"][EARLY]), exact())
    r = ipm_oracle.solve(o, s["X0"][EARLY], x_l=s["XL"][EARLY], x_u=s["XU"][EARLY], max_iter=200)
    assert r["status"] == 0
    return r["x"]


def _quadrotor_plain(B, seed):
    guess, xl, xu = _quadrotor_base()
    prefs = quadrotor_prefs(B)
    XL, XU = np.tile(xl, (B, 1)), np.tile(xu, (B, 1))
    # measured initial states, drawn as in test_ipm_warm_start.py::_quadrotor_bounds
    XL[:, STATE0] = XU[:, STATE0] = np.random.RandomState(seed).uniform(-0.2, 0.2, size=(B, 12))
    X0 = np.stack([guess * (1 + 1e-2 * np.random.RandomState(1000 + bi).uniform(-1, 1, guess.size)) for bi in range(B)])
    # the problem constants of an instance: quadrotor()'s, with the tracking target at 7 .. 9
    base = np.array(quadrotor_problem().GetOpimalProblemFuns().consts, dtype=np.float64)
    consts = [np.concatenate([base[:7], p, base[10:]]) for p in prefs]
    assert same_bits(consts[B - 1], np.array(quadrotor_problem(prefs[B - 1]).GetOpimalProblemFuns().consts, dtype=np.float64))
    return {"prefs": prefs, "consts": consts, "XL": XL, "XU": XU, "X0": X0}


def quadrotor_sweep(B, seed=8, special=True):
    """-> dict(prefs, consts, XL, XU, X0, free): B instances of quadrotor(2, 4) that differ in the tracking target, the measured
    initial state and the start; with `special`, instance EARLY starts at its own solution, NAN_X0 has a NaN in its start and
    NAN_BOUND a NaN lower bound on a free variable."""
    s = _quadrotor_plain(B, seed)
    _, xl, xu = _quadrotor_base()
    s["free"] = np.nonzero(xl != xu)[0]
    if special:
        assert B > NAN_BOUND
        s["X0"][EARLY] = _early_start(seed)
        s["X0"][NAN_X0, s["free"][7]] = np.nan
        s["XL"][NAN_BOUND, s["free"][11]] = np.nan
    return s


def finite(B):
    return [bi for bi in range(B) if bi not in (NAN_X0, NAN_BOUND)]


def restatement(s, bi, **options):
    o = orc.Oracle(quadrotor_problem(s["prefs"][bi]), exact())
    return ipm_oracle.solve(o, s["X0"][bi], x_l=s["XL"][bi], x_u=s["XU"][bi], **options)


class Solo:
    """The one-instance reference: one engine and one solver, given an instance's constants, bounds and start per pick."""

    def __init__(self, problem, options, nested=None, upper_dense=None, **solver_options):
        from lpopc_amd.engine import BatchedIPM, NLPEngine
        self.eng = NLPEngine(problem, options, n_instances=1, device=0)
        if nested is not None:
            self.eng.set_option("ipm_nested", nested)
        self.ipm = BatchedIPM(self.eng, **solver_options)
        if upper_dense is not None:
            self.ipm.set_option("upper_dense", upper_dense)

    def solve(self, x0, consts=None, xl=None, xu=None, lam0=None, z0=None):
        if consts is not None:
            self.eng.set_instance_constants(0, consts)
        if xl is not None:
            self.ipm.set_all_bounds(xl[None, :], xu[None, :])
        one = lambda a: None if a is None else a[None, :]
        return run(self.ipm, x0[None, :], one(lam0), None if z0 is None else (z0[0][None, :], z0[1][None, :]))

    def close(self):
        self.ipm.close()
        self.eng.close()


def batch(problem, options, B, nested=None, consts=None, **solver_options):
    from lpopc_amd.engine import BatchedIPM, NLPEngine
    eng = engine_with_constants(problem, options, B, consts)
    if nested is not None:
        eng.set_option("ipm_nested", nested)
    return eng, BatchedIPM(eng, **solver_options)


def engine_with_constants(problem, options, B, consts, **engine_options):
    """A B-instance engine on device 0.  Every rpm_set_instance_constants call on an initialised engine uploads all instances'
    constants again, so all but the last are set before the device is initialised."""
    from lpopc_amd.engine import NLPEngine
    eng = NLPEngine(problem, options, n_instances=B, **engine_options)
    if consts is not None:
        for bi in range(B - 1):
            eng.set_instance_constants(bi, consts[bi])
    eng.device_init(0)
    if consts is not None:
        eng.set_instance_constants(B - 1, consts[B - 1])
    return eng
