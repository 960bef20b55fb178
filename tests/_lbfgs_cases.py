"""Cases, inputs, the long-double reference and the tolerance of the limited-memory BFGS kernel tests
(tests/test_lbfgs_reference.py on the CPU, tests/test_ipm_lbfgs_kernels.py on the device).  Not a test module.

Everything here runs on the CPU from the oracle alone: the device tests feed the same float64 inputs to the kernels
(rpm_ipm_debug_lbfgs_step / _state / _solve) and compare with what this module computes in numpy.longdouble.

Pairs.  s is uniform in [-1, 1] on the free variables and 0 on the fixed ones, y = H s with a fixed SPD model H (a diagonal in
[1, 30] plus a rank-8 term), handed over as glag_new = y + g0, glag_old = g0 with random g0 and random NON-ZERO differences at
the fixed variables (so the mask vl != vu matters).  The pair the kernels store is the float64 x - x_prev and the masked
float64 glag_new - glag_old; exactly those go into the reference.

K0 of the small Woodbury cases: random values on the structural pattern of the diagonal-Hessian KKT matrix (the diagonal, the
Jacobian entries outside the columns of fixed variables, the slack couplings) — the pattern every layout of the solver holds and the only one known without a
device, so that TOL below is measured on the CPU on the very matrices the device tests use and one reference serves the band
and the nested layout.  Positive diagonal in [0.5, 2] (+ sigma on x) on variables and slacks, negative on the multipliers:
quasi-definite.  K0 of the large cases is such a diagonal alone, every value distinct.

TOL (profiles/lbfgs_noise.json, re-measured by test_lbfgs_reference.py).  The project's bound for the device K0 solve on this
family is 1e-11 of the solution's largest entry (tests/test_ipm.py).  The correction d = z0 + Z (M - E'Z)^-1 E'z0 combines
2c + 1 such solves; `noise_figure` moves every entry of z0 and of every column of Z by 1e-11 of that column's largest entry
with independent random signs (20 draws) and measures how far d moves, relative to max|d_ref|.  TOL = 4 x the largest figure
over all cases, rounded up to a power of two; the 4 covers the model being entrywise independent where real errors are
correlated."""
import functools

import numpy as np

from lpopc_amd import problems
from oracle import oracle as orc
from oracle.ipm_oracle import LimitedMemory

LD = np.longdouble
H = 6                       # IPM_LB_H
U = 2.0 ** -53              # unit roundoff of float64
K0_SOLVE_BOUND = 1e-11      # tests/test_ipm.py: device K0 solve against numpy, relative to the largest entry
NOISE_DRAWS = 20
TOL = 2.0 ** -32            # measured: see the module docstring and profiles/lbfgs_noise.json
COND_CAP = 1e3
MARGIN = 1e-3               # every decision of the skipping rule is at least this far (as a cosine) from sqrt(eps)

PROBLEMS = {
    "brachistochrone_1x4": lambda: problems.brachistochrone(1, 4),      # n < 64
    "brachistochrone_2x6": lambda: problems.brachistochrone(2, 6),
    "quadrotor_3x4": lambda: problems.quadrotor(3, 4),                   # 14 fixed variables
    "launch_2x5": lambda: problems.launch(2, 5),
    "param_sled_2x12": lambda: problems.param_sled(2, 12),               # static parameter
    "quadrotor_51x5": lambda: problems.quadrotor(51, 5),                 # n < 4096 <= Nt: 4-wave sums over n, 16-wave correction
    "quadrotor_32x8": lambda: problems.quadrotor(32, 8),                 # 16 waves throughout
    # the quadrotor's last two variables (t0, tf) are fixed: s and y are 0 there, the tail of its sums carries no weight.  The
    # brachistochrone's last variable (tf) is free: 16-wave sums whose last element counts (update test only)
    "brachistochrone_32x32": lambda: problems.brachistochrone(32, 32),
}
SIZES = {"brachistochrone_1x4": (21, 40), "brachistochrone_2x6": (53, 96), "quadrotor_3x4": (206, 352), "launch_2x5": (436, 793),
         "param_sled_2x12": (77, 131), "quadrotor_51x5": (4094, 7156), "quadrotor_32x8": (4110, 7184),
         "brachistochrone_32x32": (4101, 7180)}      # n, Nt
SMALL = ["brachistochrone_2x6", "quadrotor_3x4", "launch_2x5", "param_sled_2x12"]
LARGE = ["quadrotor_51x5", "quadrotor_32x8"]
SMALL_FILLS = (1, 3, 6, 9)
LARGE_STEPS = 7
GOOD9 = ["good"] * 9
SKIPPING = ["good", "good", "neg", "good", "neg", "neg", "szero", "yzero", "good", "good", "good"]
CLAMP = ["big", "small"]
# batches of B = 4 on brachistochrone_2x6, good steps after the priming call (call 0); mode: {instance: {call: mode}}, status:
# {instance: first call with status 1}
MIXED_PROBLEM, MIXED_B, MIXED_STEPS = "brachistochrone_2x6", 4, 8
GATING = dict(steps=9, mode={1: {3: 2}}, status={2: 4})
MIXED = dict(steps=MIXED_STEPS, mode={3: {8: 2}}, status={1: 3, 2: 7})     # the fill levels the Woodbury test wants:
MIXED_COUNTS = (6, 2, 6, 0)                    # 6 after two shifts, 2 (frozen from call 3), 6 never shifted (frozen from call 7), emptied


@functools.lru_cache(maxsize=None)
def info(name):
    """Sizes, the fixed variables and the structural pattern of K0 (lower triangle, unknown order: variables, slacks, multipliers)."""
    o = orc.Oracle(PROBLEMS[name]())
    xl, xu, gl, gu = o.bounds()
    n, m = o.n, o.m
    ineq = np.nonzero(gl != gu)[0]
    ns = ineq.size
    nv, nt = n + ns, n + ns + m
    assert (n, nt) == SIZES[name], (name, n, nt)
    ji, jj = np.asarray(o.jac_structure())
    ji, jj = ji[xl[jj] != xu[jj]], jj[xl[jj] != xu[jj]]        # fixed variables are identity rows of the solver's matrix: no slots for their columns
    ent = np.unique(np.stack([nv + np.asarray(ji, dtype=np.int64), np.asarray(jj, dtype=np.int64)], axis=1), axis=0)
    rows = np.concatenate([np.arange(nt), ent[:, 0], nv + ineq])
    cols = np.concatenate([np.arange(nt), ent[:, 1], n + np.arange(ns)])
    sign = np.ones(nt)
    sign[nv:] = -1.0
    xl, xu = np.array(xl, dtype=float), np.array(xu, dtype=float)
    return dict(name=name, n=n, m=m, ns=ns, nv=nv, nt=nt, xl=xl, xu=xu, free=np.asarray(xl != xu),
                rows=rows.astype(np.int32), cols=cols.astype(np.int32), sign=sign)


# ---------------------------------------------------------------------------------------------- inputs of the update
def make_steps(inf, kinds, seed):
    """-> [(x, glag_new, glag_old)]: the priming call (no pair: x only becomes the previous iterate) and one call per kind:
    good (y = H s), neg (y = -H s), szero (x unchanged, y != 0), yzero (y = 0 exactly, s != 0), big (y = 1e9 s), small (y = 1e-9 s)."""
    n, free = inf["n"], inf["free"]
    rng = np.random.RandomState(seed)
    hd, lr = rng.uniform(1, 30, n), rng.randn(n, 8) / np.sqrt(n)

    def model(s):
        return hd * s + 50.0 * (lr @ (lr.T @ s))
    x = np.where(free, rng.uniform(-1, 1, n), inf["xl"])
    out = []
    for kind in ["prime"] + list(kinds):
        move = np.where(free, rng.uniform(-1, 1, n), 0.0)
        x_new = x.copy() if kind in ("prime", "szero") else x + move
        s = x_new - x
        y = {"prime": model(move), "szero": model(move), "good": model(s), "neg": -model(s), "yzero": 0.0 * s, "big": 1e9 * s, "small": 1e-9 * s}[kind]
        g0 = rng.uniform(-1, 1, n)
        at_fixed = g0 + rng.uniform(0.5, 1.5, n) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)
        g1 = np.where(free, g0 if kind == "yzero" else g0 + y, at_fixed)
        out.append((x_new, g1, g0))
        x = x_new
    return out


class RefInstance:
    """One instance of the update in long double, gated as the kernels gate it."""

    def __init__(self, inf):
        self.inf = inf
        self.lm = LimitedMemory(inf["n"], dtype=LD)
        self.sigma_bound = 0.0
        self.m_valid = False               # the kernels write M when a pair is stored or skips empty the memory, not before
        self.log = []                      # (action, cosine) of every call

    def step(self, x, g1, g0, mode=0, status=0):
        lm, free = self.lm, self.inf["free"]
        if status != 0:
            act, cos = "frozen", None
        elif mode != 0:
            lm.empty()
            self.sigma_bound, self.m_valid = 0.0, False      # (M is left as it was: nothing reads it while no pair is held)
            act, cos = "emptied", None
        elif lm.prev is None:
            lm.prev = x.copy()
            act, cos = "first", None
        else:
            s64, y64 = x - lm.prev, np.where(free, g1 - g0, 0.0)           # float64, as the kernels form them
            s, y = s64.astype(LD), y64.astype(LD)
            sn, yn = np.sqrt(s @ s), np.sqrt(y @ y)
            cos = float((s @ y) / (sn * yn)) if sn > 0 and yn > 0 else 0.0
            act = lm.update(s, y)
            lm.prev = x.copy()
            if act == "store":
                clamped = lm.sigma in (LD(lm.init_val_min), LD(lm.init_val_max))
                # sigma = s'y / s's from two sums of n products in any order: (n + 2) u (sum|s y| + |s'y|) / s's to first order
                self.sigma_bound = 0.0 if clamped else float((self.inf["n"] + 2) * U * (np.abs(s * y).sum() + abs(s @ y)) / (s @ s))
            elif act == "skip-empty":
                self.sigma_bound = 0.0
            self.m_valid = self.m_valid or act in ("store", "skip-empty")
        self.log.append((act, cos))
        return act

    def check_margins(self):
        """asserted on the reference alone: rounding cannot flip a decision of the skipping rule"""
        for act, cos in self.log:
            if act == "store":
                assert cos >= MARGIN, (act, cos)
            elif act in ("skip", "skip-empty"):
                assert cos <= -MARGIN or cos == 0.0, (act, cos)

    def record(self):
        lm = self.lm
        return dict(sigma=lm.sigma, pairs=len(lm.S), skipped=lm.skipped, prev_valid=int(lm.prev is not None), updates=lm.updates, skips=lm.skips)

    def m_and_bound(self):
        """M in the kernels' fixed 12 x 12 layout (index a < H: pair a's sigma s column, H + a: its y column; identity on the
        unused indices) and the entrywise bound (n + 2) 2^-53 sum|terms| (times sigma in the S'S block): a sum of n products
        in any order plus two more roundings.  Structural zeros have bound 0."""
        lm, n, c = self.lm, self.inf["n"], len(self.lm.S)
        M, bound = np.eye(2 * H, dtype=LD), np.zeros((2 * H, 2 * H))
        if c:
            S, Y = np.abs(np.array(lm.S, dtype=LD)), np.abs(np.array(lm.Y, dtype=LD))
            ss, sy = S @ S.T, S @ Y.T
            low = np.tril(sy, -1)
            mag = np.block([[lm.sigma * ss, low], [low.T, np.diag(np.diag(sy))]])
            idx = np.array(list(range(c)) + [H + a for a in range(c)])
            M[np.ix_(idx, idx)] = lm.compact()[1]
            bound[np.ix_(idx, idx)] = ((n + 2) * U * mag).astype(np.float64)
        return M, bound


def run_reference(inf, steps, mode=None, status_from=None):
    """One instance through `steps`; mode: {call: mode}, status_from: first call with status 1 (call 0 = priming call) -> RefInstance"""
    ref = RefInstance(inf)
    for t, (x, g1, g0) in enumerate(steps):
        ref.step(x, g1, g0, (mode or {}).get(t, 0), int(status_from is not None and t >= status_from))
    return ref


# ---------------------------------------------------------------------------------------------- long-double linear algebra
def ld_solve(A, b):
    """A x = b by elimination with partial pivoting in long double (numpy has no long-double LAPACK); b a vector or a matrix."""
    A, b = np.array(A, dtype=LD), np.array(b, dtype=LD)
    vec = b.ndim == 1
    if vec:
        b = b[:, None]
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]], b[[k, p]] = A[[p, k]], b[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k + 1:] -= np.outer(f, A[k, k + 1:])
        b[k + 1:] -= np.outer(f, b[k])
    x = np.zeros_like(b)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x[:, 0] if vec else x


def e_and_m(inf, lm):
    """E (Nt x 2c: Q at the positions of x) and M of the pairs held, long double"""
    Q, M = lm.compact()
    E = np.zeros((inf["nt"], Q.shape[1]), dtype=LD)
    E[:inf["n"]] = Q
    return E, M


# ---------------------------------------------------------------------------------------------- the Woodbury cases
def k0_values(inf, sigma, seed, diagonal_only=False):
    """Values of K0 on inf's pattern (or on the diagonal alone) for one instance, float64; sigma (float64) is added on x."""
    rng = np.random.RandomState(seed)
    nt, n = inf["nt"], inf["n"]
    diag = inf["sign"] * rng.uniform(0.5, 2.0, nt)
    diag[:n] += sigma
    if diagonal_only:
        return diag
    return np.concatenate([diag, rng.uniform(-1, 1, inf["rows"].size - nt)])


def k0_dense(inf, vals):
    A = np.zeros((inf["nt"], inf["nt"]))
    A[inf["rows"], inf["cols"]] = vals
    A[inf["cols"], inf["rows"]] = vals
    return A


def seed_of(name, bi):
    return 1000 * (sorted(PROBLEMS).index(name) + 1) + bi


@functools.lru_cache(maxsize=None)
def small_steps(name, bi):
    return make_steps(info(name), GOOD9, seed_of(name, bi))


@functools.lru_cache(maxsize=None)
def skipping_steps(name, bi):
    return make_steps(info(name), SKIPPING, seed_of(name, 50 + bi))


@functools.lru_cache(maxsize=None)
def clamp_steps(name):
    return make_steps(info(name), CLAMP, seed_of(name, 90))


@functools.lru_cache(maxsize=None)
def batch_steps(bi):
    """instance bi of the B = 4 batches: GATING runs all of it, MIXED its first MIXED_STEPS + 1 calls"""
    return make_steps(info(MIXED_PROBLEM), ["good"] * GATING["steps"], seed_of(MIXED_PROBLEM, 10 + bi))


def gates(schedule, bi, t):
    """(mode, status) of instance bi at call t"""
    return schedule["mode"].get(bi, {}).get(t, 0), int(bi in schedule["status"] and t >= schedule["status"][bi])


def run_batch_reference(schedule, bi):
    ref = RefInstance(info(MIXED_PROBLEM))
    for t, (x, g1, g0) in enumerate(batch_steps(bi)[:schedule["steps"] + 1]):
        ref.step(x, g1, g0, *gates(schedule, bi, t))
    return ref


@functools.lru_cache(maxsize=None)
def large_steps(name):
    return make_steps(info(name), ["good"] * LARGE_STEPS, seed_of(name, 0))


def case_keys():
    """(key, kind, name, fill, instance) of every Woodbury case of the device tests"""
    out = [("%s@%d#%d" % (name, fill, bi), "small", name, fill, bi) for name in SMALL for fill in SMALL_FILLS for bi in range(2)]
    out += [("%s@mixed#%d" % (MIXED_PROBLEM, bi), "mixed", MIXED_PROBLEM, MIXED_STEPS, bi) for bi in range(MIXED_B)]
    out += [("%s@%d#0" % (name, LARGE_STEPS), "large", name, LARGE_STEPS, 0) for name in LARGE]
    return out


@functools.lru_cache(maxsize=None)
def woodbury_case(key):
    """Inputs and the long-double reference of one case: dict(inf, ref (RefInstance), vals (K0 values, float64), rhs, d_ref (LD),
    E, M (LD), diagonal (bool))."""
    kind, name, fill, bi = {k[0]: k[1:] for k in case_keys()}[key]
    inf = info(name)
    if kind == "small":
        ref = run_reference(inf, small_steps(name, bi)[:fill + 1])
    elif kind == "mixed":
        ref = run_batch_reference(MIXED, bi)
        assert len(ref.lm.S) == MIXED_COUNTS[bi]
    else:
        ref = run_reference(inf, large_steps(name))
    ref.check_margins()
    diagonal = kind == "large"
    seed = seed_of(name, bi) + 7 * fill + (500 if kind == "mixed" else 0)
    vals = k0_values(inf, float(ref.lm.sigma), seed, diagonal)
    rhs = np.random.RandomState(seed + 1).uniform(-1, 1, inf["nt"])
    E, M = e_and_m(inf, ref.lm)
    c2 = E.shape[1]
    if diagonal:                       # closed form: elementwise K0^-1 and a 2c x 2c solve
        k0 = vals.astype(LD)
        z0, Z = rhs.astype(LD) / k0, E / k0[:, None]
        d_ref = z0 + Z @ ld_solve(M - E.T @ Z, E.T @ z0)
    else:                              # K = K0 - E M^-1 E' formed and solved directly: no Woodbury in the reference
        K = k0_dense(inf, vals).astype(LD)
        if c2:
            K = K - E @ ld_solve(M, E.T)
        d_ref = ld_solve(K, rhs.astype(LD))
    return dict(inf=inf, ref=ref, vals=vals, rhs=rhs, d_ref=d_ref, E=E, M=M, diagonal=diagonal)


def woodbury_f64(case, rng=None):
    """The identity in float64 (numpy): d = z0 + Z (M - E'Z)^-1 E'z0.  With rng: z0 and every column of Z moved entrywise by
    K0_SOLVE_BOUND of the column's largest entry, random signs.  -> d, C"""
    inf, vals = case["inf"], case["vals"]
    E, M, r = case["E"].astype(np.float64), case["M"].astype(np.float64), case["rhs"]
    if "z" not in case:
        if case["diagonal"]:
            case["z"] = (r / vals, E / vals[:, None])
        else:
            A = k0_dense(inf, vals)
            case["z"] = (np.linalg.solve(A, r), np.linalg.solve(A, E) if E.shape[1] else E.copy())
    z0, Z = case["z"]
    if rng is not None:
        z0 = z0 + K0_SOLVE_BOUND * np.max(np.abs(z0)) * np.where(rng.rand(*z0.shape) < 0.5, -1.0, 1.0)
        if Z.shape[1]:
            Z = Z + K0_SOLVE_BOUND * np.max(np.abs(Z), axis=0) * np.where(rng.rand(*Z.shape) < 0.5, -1.0, 1.0)
    if not Z.shape[1]:
        return z0, np.eye(1)
    C = M - E.T @ Z
    return z0 + Z @ np.linalg.solve(C, E.T @ z0), C


def cond_k_bound(case):
    """cond_2(K), K = K0 - E M^-1 E': by SVD for the dense cases; for a diagonal K0 (order 7000) an upper bound instead — K is
    then diag(K0) + (B - sigma I) on x and diagonal elsewhere, B - sigma I = -Q M^-1 Q' has its non-zero eigenvalues on
    span(Q), and Weyl's inequalities bound the spectrum of the x block by [min k0_x + min(0, l_min), max k0_x + max(0, l_max)]."""
    inf, vals = case["inf"], case["vals"]
    E, M = case["E"].astype(np.float64), case["M"].astype(np.float64)
    if not case["diagonal"]:
        K = k0_dense(inf, vals)
        if E.shape[1]:
            K = K - E @ np.linalg.solve(M, E.T)
        return float(np.linalg.cond(K))
    n = inf["n"]
    q, r = np.linalg.qr(E[:n])
    low = np.linalg.eigvalsh(-(r @ np.linalg.solve(M, r.T) + (r @ np.linalg.solve(M, r.T)).T) / 2)
    lo = min(vals[:n].min() + min(0.0, low.min()), np.abs(vals[n:]).min())
    hi = max(vals[:n].max() + max(0.0, low.max()), np.abs(vals[n:]).max())
    assert lo > 0
    return float(hi / lo)


def noise_figure(case, key):
    """-> dict(figure, woodbury_f64, cond_K, cond_C) of one case (see the module docstring)"""
    d_ref = case["d_ref"]
    scale = float(np.max(np.abs(d_ref)))
    d0, C = woodbury_f64(case)
    rng = np.random.RandomState(sum(map(ord, key)))
    fig = 0.0
    for _ in range(NOISE_DRAWS):
        d, _ = woodbury_f64(case, rng)
        fig = max(fig, float(np.max(np.abs(d - d0))) / scale)
    return dict(figure=fig, woodbury_f64=float(np.max(np.abs(d0.astype(LD) - d_ref))) / scale, cond_K=cond_k_bound(case), cond_C=float(np.linalg.cond(C)))


def tol_from(figures):
    return float(2.0 ** np.ceil(np.log2(4.0 * max(figures))))


def measure_all():
    return {k[0]: noise_figure(woodbury_case(k[0]), k[0]) for k in case_keys()}


if __name__ == "__main__":          # PYTHONPATH=. python tests/_lbfgs_cases.py profiles/lbfgs_noise.json: measure and write the profile
    import json
    import sys
    res = measure_all()
    prof = {"K0_solve_bound": K0_SOLVE_BOUND, "draws": NOISE_DRAWS, "TOL": tol_from([v["figure"] for v in res.values()]),
            "cases": {k: {q: float("%.4g" % w) for q, w in v.items()} for k, v in res.items()}}
    with open(sys.argv[1], "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    print("TOL = 2^%d" % int(np.log2(prof["TOL"])), "largest figure %.3g" % max(v["figure"] for v in res.values()))
