"""Cases, inputs and the entrywise tolerance rule of the exact-Hessian tests (tests/test_oracle_hessian.py on the CPU,
tests/test_gpu_hessian.py on the device).  Not a test module.

The rule:  |H - H_ref|_i <= C_NOISE * 2^-52 * mag_i  entry by entry, mag = Oracle.eval_h_mag (the sum of the magnitudes of
the terms the entry is made of, 1/den included); where mag_i == 0 the two values must be equal.  C_NOISE is derived from
the oracle alone (test_oracle_hessian.py::test_noise_constant_covers_two_builds_of_the_oracle, profiles/hessian_noise.json).
"""
import numpy as np

from lpopc_amd import problems
from lpopc_amd.problem import Options

EPS = 2.0 ** -52
C_NOISE = 16.0            # 8 * max(c_ref, 1) rounded up to a power of two; c_ref per case in profiles/hessian_noise.json
STEPS = (1e-3, 1e-6)
RESOLVED_RTOL, RESOLVED_SHARE = 1e-6, 0.70     # at step 1e-3: C*2^-52*mag_i <= 1e-6 |H_ref,i| on >= 70 % of the nonzeros

# nodes per workgroup of rpm_hess_kernel (ensure_hessian: the largest power of two <= 64 with TH * NR <= 1024 threads);
# the device tests assert that the engine says the same (get_option("hess_tile_nodes"))
TH = {"hypersensitive": 64, "bryson_denham": 32, "brachistochrone": 32, "climb": 32, "launch": 8, "quadrotor": 4}


def ragged_mesh(nodes):
    """Mesh points of unequal interval widths for the given nodes per interval."""
    w = np.array([1.0 + 0.25 * ((3 * i) % 5) for i in range(len(nodes))])
    pts = -1.0 + 2.0 * np.concatenate([[0.0], np.cumsum(w)]) / w.sum()
    pts[0], pts[-1] = -1.0, 1.0
    return [float(p) for p in pts], [int(n) for n in nodes]


def _one_phase(make):
    def build(nodes):
        p = make()
        problems.set_mesh(p.GetPhase(0), *ragged_mesh(nodes))
        return p
    return build


_BUILD = {
    "hypersensitive": lambda nodes: problems.hypersensitive(*ragged_mesh(nodes), tf=50.0),
    "bryson_denham": _one_phase(lambda: problems.bryson_denham()),
    "brachistochrone": _one_phase(lambda: problems.brachistochrone(None, None)),
    "climb": _one_phase(lambda: problems.min_time_climb(None, None)),
    "quadrotor": _one_phase(lambda: problems.quadrotor(None, None)),
}


def launch_with(per_phase_nodes):
    """Delta-III, all four phases and three linkages, phase i on ragged_mesh(per_phase_nodes[i])."""
    p = problems.launch()
    for i, nodes in enumerate(per_phase_nodes):
        problems.set_mesh(p.GetPhase(i), *ragged_mesh(nodes))
    return p


def _split(n, th):
    """n nodes in ragged intervals none of which ends on a multiple of the tile."""
    if n <= 3:
        return [n]
    if n <= 9:
        return [n - 2, 2] if n >= 5 else [2, n - 2]
    parts, left, i = [], n, 0
    while left > 0:
        k = min(left, max(2, (th // 2 + 3 + 5 * (i % 3)) if th >= 8 else 3 + i % 2))
        if 0 < left - k < 2:
            k = left
        parts.append(k)
        left -= k
        i += 1
    return parts


def _cases():
    out = []
    for name in ("hypersensitive", "bryson_denham", "brachistochrone", "climb", "quadrotor"):
        th = TH[name]
        for n in (th - 1, th, th + 1, 2 * th + 3):          # one partial tile, one full, k0 > 0 with cnt = 1, and cnt = 3 < TH
            out.append(("%s_N%d" % (name, n), name, lambda name=name, n=n, th=th: _BUILD[name](_split(n, th))))
    # N > 256: five tiles of 64 with a partial last one.  NOT a test of rpm_hess_tt_kernel's strided loop: the functors are
    # autonomous, the per-node tt terms are exactly 0 (tests/test_gpu_hessian.py::test_t0_tf_reduction_on_given_terms is)
    out.append(("hypersensitive_N300", "hypersensitive", lambda: _BUILD["hypersensitive"]([15] * 20)))
    # the smallest mesh the set-up accepts: one interval of two nodes
    out.append(("hypersensitive_N2", "hypersensitive", lambda: _BUILD["hypersensitive"]([2])))
    out.append(("brachistochrone_N2", "brachistochrone", lambda: _BUILD["brachistochrone"]([2])))
    # Delta-III: TH = 8; the four phases carry N = TH-1, TH, TH+1, 2 TH+3 at once, in two orders (the link entries of a
    # pair use the LEFT phase's node count for the right phase's columns, so the order matters)
    out.append(("launch_N7_8_9_19", "launch", lambda: launch_with([[5, 2], [8], [4, 5], [6, 7, 6]])))
    out.append(("launch_N19_9_8_7", "launch", lambda: launch_with([[9, 10], [2, 7], [3, 5], [7]])))
    return out


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]

ANALYTIC_CASES = [
    # first-derive = analytic (rpm_hess_kernel<P, true>), multi-tile
    ("hypersensitive_N131_analytic", "hypersensitive", lambda: _BUILD["hypersensitive"](_split(131, 64))),
    ("brachistochrone_N67_analytic", "brachistochrone", lambda: _BUILD["brachistochrone"](_split(67, 32))),
]


def exact_options(step=None, analytic=False):
    o = Options()
    o.SetStringValue("hessian-approximation", "exact")
    if step is not None:
        o.SetNumericValue("finite-difference-tol", step)
    if analytic:
        o.SetStringValue("first-derive", "analytic")
    return o


def iterates(x_guess):
    """Two seeded iterates: every component of the guess moved away from zero by 15 % to 30 % of itself (an exact zero
    becomes 0.15 to 0.3).  One-sided on purpose: the Hessian has to have curvature to resolve, and the guesses sit where
    the functions cancel internally (hover thrust against gravity, u against x^3 on the turnpike, the launcher at rest
    in the rotating frame with the density's exp at ground level), which is rounding noise no magnitude of F bounds."""
    x_guess = np.asarray(x_guess, dtype=np.float64)
    out = []
    for seed in (5, 17):
        u = np.random.RandomState(seed).uniform(0.5, 1.0, size=x_guess.shape)
        out.append(np.where(x_guess == 0.0, 0.3 * u, x_guess * (1.0 + 0.3 * u)))
    return out


def draws(m):
    """Two (sigma, lambda) draws, lambda ~ U(-1, 1); the second has sigma = 0 (what a feasibility step evaluates)."""
    return [(0.7, np.random.RandomState(1).uniform(-1, 1, m)), (0.0, np.random.RandomState(2).uniform(-1, 1, m))]


def noise_ratio(h, h_ref, mag):
    """max_i |h - h_ref|_i / (2^-52 mag_i); inf if the two differ where mag_i == 0."""
    d = np.abs(h - h_ref)
    z = mag == 0
    if np.any(d[z] != 0) or not np.all(np.isfinite(h)):
        return float("inf")
    return float(np.max(d[~z] / (EPS * mag[~z]))) if np.any(~z) else 0.0


def assert_entrywise(h, h_ref, mag, c=C_NOISE, what=""):
    assert h.shape == h_ref.shape == mag.shape
    assert np.all(np.isfinite(h)), what
    d = np.abs(h - h_ref)
    bad = np.flatnonzero(~(d <= c * EPS * mag))          # mag_i == 0: d_i must be 0
    if bad.size:
        i = bad[np.argmax(d[bad] / np.maximum(EPS * mag[bad], 1e-300))]
        raise AssertionError("%s: %d of %d entries off; worst entry %d: got %.17g, reference %.17g, |d| = %.3g = %.3g * 2^-52 mag"
                             % (what, bad.size, h.size, i, h[i], h_ref[i], d[i], d[i] / max(EPS * mag[i], 1e-300)))


def resolved_share(h_ref, mag, c=C_NOISE):
    """Share of the nonzero reference entries that the rule pins to 1e-6 of their own value."""
    nz = h_ref != 0
    return float(np.mean(c * EPS * mag[nz] <= RESOLVED_RTOL * np.abs(h_ref[nz]))) if np.any(nz) else 1.0
