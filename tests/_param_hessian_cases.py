"""Cases of the parameter-Hessian tests (tests/test_param_hessian_reference.py on the CPU, tests/test_gpu_param_hessian.py on
the device): functor, meshes, and the reference values of a case, computed once per process and shared.  Not a test module.

Nodes per workgroup of rpm_hess_kernel: sled NV = 5, NR = 21; oscillator and probe NV = 6, NR = 28 — TH = 32 for all three
(the largest power of two with TH * NR <= 1024), so the meshes sit on both sides of 32 and, with N = 300, past the 256
threads of the reduction."""
import os

import numpy as np

import _hessian_cases as hc
import _param_hessian_reference as R
from lpopc_amd import problems
from lpopc_amd.problem import Options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH = 32
PROBE_HEADER = os.path.join(ROOT, "tests", "user_problems", "param_hessian_probe.hpp")


def _nodes(n):
    return [15] * 20 if n == 300 else hc._split(n, TH)


def _remesh(prob, per_phase):
    for i, n in enumerate(per_phase):
        ph = prob.GetPhase(i)
        ph.GetMeshPoints().clear()
        ph.GetNodesPerInterval().clear()
        problems.set_mesh(ph, *hc.ragged_mesh(_nodes(n)))
    return prob


def probe_library():
    from lpopc_amd import userproblem
    return userproblem.build(PROBE_HEADER)


def make(functor, per_phase):
    if functor == "sled":
        return _remesh(problems.param_sled(), per_phase)
    if functor == "oscillator":
        return _remesh(problems.param_oscillator(), per_phase)
    return R.probe_problem([hc.ragged_mesh(_nodes(n)) for n in per_phase], probe_library())


FUNCTOR = {"sled": R.Sled, "oscillator": R.Oscillator, "probe": R.Probe}

# (id, functor, nodes per phase, analytic first derivatives)
CASES = ([("sled_N%d" % n, "sled", (n,), False) for n in (2, 31, 32, 33, 67, 300)] +
         [("%s_N%d_%d" % (f, a, b), f, (a, b), False) for f in ("oscillator", "probe") for (a, b) in ((31, 33), (67, 32), (2, 300))] +
         [("sled_N67_analytic", "sled", (67,), True)])
CASE_IDS = [c[0] for c in CASES]


def options(step=None, analytic=False):
    o = Options()
    o.SetStringValue("hessian-approximation", "exact-parameters")
    if step is not None:
        o.SetNumericValue("finite-difference-tol", step)
    if analytic:
        o.SetStringValue("first-derive", "analytic")
    return o


def starting_point(prob):
    """(guess, m) on the mesh: the engine's host set-up."""
    from lpopc_amd.engine import NLPEngine
    e = NLPEngine(prob)
    x = e.get_starting_point()
    m = e.m
    e.close()
    return x, m


_REF = {}


def reference(cid, step):
    """{"ref", "dep", "x0", "m", "runs": [(x, sigma, lam, values, mag)]} of a case at a step: hc.iterates x hc.draws."""
    key = (cid, step)
    if key not in _REF:
        _, functor, per_phase, analytic = CASES[CASE_IDS.index(cid)]
        prob = make(functor, per_phase)
        ref = R.Reference(prob, FUNCTOR[functor], analytic)
        x0, m = starting_point(prob)
        dep = ref.dependencies(x0)
        runs = []
        for x in hc.iterates(x0):
            for sigma, lam in hc.draws(m):
                _, _, v, mag = ref.walk(x, sigma, lam, step, dep)
                runs.append((x, sigma, lam, v.astype(np.float64), mag.astype(np.float64)))
        _REF[key] = dict(ref=ref, dep=dep, x0=x0, m=m, runs=runs, structure=ref.structure(dep), reduced=ref.reduced(dep))
    return _REF[key]


def entry_constants(reduced):
    """C per entry: hc.C_NOISE, plus one per addition level of rpm_hess_tt_kernel for the entries it sums —
    ceil(log2(min(N, 256))) levels of the tree and ceil(N / 256) additions of the strided loop."""
    c = np.full(reduced.shape, hc.C_NOISE)
    nz = reduced > 0
    N = reduced[nz].astype(np.float64)
    c[nz] += np.ceil(np.log2(np.minimum(N, 256))) + np.ceil(N / 256)
    return c


def pooled_resolved_share(runs):
    ok = nz = 0
    for (_, _, _, v, mag) in runs:
        z = v != 0
        nz += int(z.sum())
        ok += int(np.sum(hc.C_NOISE * hc.EPS * mag[z] <= hc.RESOLVED_RTOL * np.abs(v[z])))
    return ok / nz if nz else 1.0
