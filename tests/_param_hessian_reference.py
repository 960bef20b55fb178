"""Reference of the exact Hessian with static parameters (hessian-approximation = exact-parameters), in np.longdouble, for
the two shipped parameter functors (sled, oscillator) and the test functor tests/user_problems/param_hessian_probe.hpp.
Not a test module.  The oracle's Hessian is nq = 0 only, so this stands where it stands for tests/test_gpu_hessian.py.

Two layers:

(a) lagrangian_nl(x, sigma, lam): the nonlinear part of the Lagrangian straight from its definition — per phase the sum over
    the nodes of (tf - t0)/2 (sigma w L - lambda . f) + mu . c, plus sigma Mayer + nu . event, plus the linkage terms.  (The
    linear part of the defect rows, D x, has no second derivative.)
(b) walk(x, sigma, lam, step): the second-difference walk of csrc/rpm_hess_kernels.hip, triplet by triplet in the COO order
    of csrc/rpm_hess.cpp.  Perturbed points, steps and denominators are formed in double, as the device forms them; function
    values, differences and sums are long double.  Returns (hi, hj, values, mag); mag as Oracle.eval_h_mag builds it: every
    F, multiplier, sigma, weight and factor by its absolute value, every subtraction an addition, 1/den included.
"""
import numpy as np

from lpopc_amd import problems
from lpopc_amd.engine import NLPEngine

LD = np.longdouble


# ---- the functors, term by term what csrc/problems/problems.hpp and the probe header compute -----------------------------
class Sled:
    nx, nu, nq, nc = 2, 1, 1, 0
    has_analytic = True

    @staticmethod
    def dae(ph, t, x, u, p, c):
        return [x[1], p[0] * u[0]], []

    @staticmethod
    def lagrange(ph, t, x, u, p, c):
        return LD(0)

    @staticmethod
    def mayer(ph, t0, x0, tf, xf, p, c):
        return tf + c[0] * (p[0] * p[0])

    @staticmethod
    def event(ph, t0, x0, tf, xf, p, c):
        return [x0[0], x0[1], xf[0], xf[1]]

    @staticmethod
    def link(xl, xr, pl, pr, c):
        return []

    @staticmethod
    def dae_jac_col(ph, v, t, x, u, p, c):       # columns [x, v, u, t, p]
        return [LD(1) if v == 1 else LD(0), p[0] if v == 2 else (u[0] if v == 4 else LD(0))]

    @staticmethod
    def lagrange_grad_col(ph, v, t, x, u, p, c):
        return LD(0)


class Oscillator:
    nx, nu, nq, nc = 2, 1, 2, 1
    has_analytic = False

    @staticmethod
    def dae(ph, t, x, u, p, c):
        return [x[1], (-(p[0] * x[0]) - c[0] * x[1]) + u[0]], [x[0] + p[1] * u[0]]

    @staticmethod
    def lagrange(ph, t, x, u, p, c):
        return (u[0] * u[0] + p[1] * (x[0] * x[0])) + c[1] * (p[0] * p[0])

    @staticmethod
    def mayer(ph, t0, x0, tf, xf, p, c):
        return xf[0] * xf[0] + p[0] * p[1] if ph == 2 else LD(0)

    @staticmethod
    def event(ph, t0, x0, tf, xf, p, c):
        return [x0[0], x0[1]] if ph == 1 else [xf[0] + p[1]]

    @staticmethod
    def link(xl, xr, pl, pr, c):
        return [xl[0] - xr[0], xl[1] - xr[1], pl[0] - pr[0], pl[1] - pr[1]]


class Probe:
    nx, nu, nq, nc = 2, 1, 2, 1
    has_analytic = False

    @staticmethod
    def dae(ph, t, x, u, p, c):
        return ([x[1] + (p[0] * t) * x[0], ((-(p[0] * x[0]) + (p[1] * u[0]) * x[1]) + (t * t) * u[0]) + x[1] * x[1]],
                [((x[0] * u[0] + x[0] * x[1]) + u[0] * u[0]) + (p[1] * t) * p[0]])

    @staticmethod
    def lagrange(ph, t, x, u, p, c):
        return (u[0] * u[0] + (p[1] * x[0]) * x[0]) + (t * p[0]) * x[1]

    @staticmethod
    def mayer(ph, t0, x0, tf, xf, p, c):
        return ((tf * p[0]) * xf[0] + (p[1] * p[1]) * x0[0]) + t0 * tf

    @staticmethod
    def event(ph, t0, x0, tf, xf, p, c):
        return [x0[0] * p[0] + t0 * p[1], xf[1] * tf + (p[0] * p[1]) * xf[0]]

    @staticmethod
    def link(xl, xr, pl, pr, c):
        return [xl[0] * pl[0] - xr[0] * pr[1], xl[1] * xr[1] + pl[1] * pr[0]]


def probe_problem(meshes, library=None):
    """The probe functor's two phases on the given (mesh points, nodes per interval) pairs, one linkage of two constraints.
    library: what lpopc_amd.userproblem.build made of tests/user_problems/param_hessian_probe.hpp (None: description only)."""
    from lpopc_amd.problem import Linkage, OptimalProblem, Phase, ProblemFunctor
    from lpopc_amd.userproblem import RPM_PROBLEM_USER
    op = OptimalProblem(2, 1, ProblemFunctor(RPM_PROBLEM_USER, [], library=library))
    for ip, (mesh, nodes) in enumerate(meshes):
        P = Phase(ip + 1, 2, 1, 2, 1, 2)
        P.SetTimeMin(0.5 + 2.0 * ip, 1.5 + 2.0 * ip)
        P.SetTimeMax(0.5 + 2.0 * ip, 3.5 + 2.0 * ip)
        for _ in range(2):
            P.SetStateMin(-4, -4, -4)
            P.SetStateMax(4, 4, 4)
        P.SetcontrolMin(-3.0)
        P.SetcontrolMax(3.0)
        for lo, hi in ((0.2, 5.0), (0.1, 2.0)):
            P.SetparameterlMin(lo)
            P.SetparameterMax(hi)
        P.SetpathMin(-9.0)
        P.SetpathMax(9.0)
        for _ in range(2):
            P.SeteventMin(-5.0)
            P.SeteventMax(5.0)
        P.SetTimeGuess(0.5 + 2.0 * ip)
        P.SetTimeGuess(2.5 + 2.0 * ip)
        P.SetStateGuess(1, 1.0 - 0.4 * ip)
        P.SetStateGuess(1, 0.6 - 0.4 * ip)
        P.SetStateGuess(2, -0.3)
        P.SetStateGuess(2, -0.2)
        P.SetControlGuess(1, 0.4)
        P.SetControlGuess(1, -0.3)
        P.SetparameterGuess(1.3)
        P.SetparameterGuess(0.7)
        problems.set_mesh(P, mesh, nodes)
        op.AddPhase(P)
    lk = Linkage(1, 1, 2)
    for _ in range(2):
        lk.SetLinkMin(-1.0)
        lk.SetLinkMax(1.0)
    op.AddLinkage(lk)
    return op


_TABLES = {}


def _tables(mesh, nodes):
    """Collocation points and weights of a mesh: the engine's own host tables (they depend on the mesh alone)."""
    key = (tuple(float(v) for v in mesh), tuple(int(v) for v in nodes))
    if key not in _TABLES:
        e = NLPEngine(problems.hypersensitive(list(key[0]), list(key[1])))
        t = e.phase_tables(0)
        e.close()
        _TABLES[key] = (t["points"].copy(), t["weights"].copy())
    return _TABLES[key]


class _Phase:
    pass


class Reference:
    def __init__(self, prob, functor, analytic=False):
        self.f = functor
        self.c = [LD(v) for v in prob.GetOpimalProblemFuns().consts]
        self.analytic = bool(analytic) and functor.has_analytic
        self.ph, self.links = [], []
        var0 = g0 = 0
        for ip in range(prob.GetPhaseNum()):
            P = prob.GetPhase(ip)
            d = _Phase()
            d.nx, d.nu, d.nq, d.nc, d.ne = P.get_optimal_info()
            d.num = ip + 1
            d.N = int(sum(P.GetNodesPerInterval()))
            d.points, d.weights = _tables(P.GetMeshPoints(), P.GetNodesPerInterval())
            d.var0, d.g0 = var0, g0
            d.u0 = var0 + d.nx * (d.N + 1)
            d.t0 = d.u0 + d.nu * d.N
            d.p0 = d.t0 + 2
            var0 = d.p0 + d.nq
            g0 += (d.nx + d.nc) * d.N + d.ne
            self.ph.append(d)
        for il in range(prob.GetLinkageNum()):
            lk = prob.GetLinkage(il)
            self.links.append((lk.LeftPhase(), lk.RightPhase(), len(lk.GetLinkageMin()), g0))
            g0 += len(lk.GetLinkageMin())
        self.n = var0

    # ---- (a) ------------------------------------------------------------------------------------------------------------
    def lagrangian_nl(self, x, sigma, lam):
        x = np.asarray(x, dtype=LD)
        lam = np.asarray(lam, dtype=LD)
        sigma = LD(sigma)
        f, c, tot = self.f, self.c, LD(0)
        for d in self.ph:
            N, t0, tf = d.N, x[d.t0], x[d.t0 + 1]
            p = [x[d.p0 + j] for j in range(d.nq)]
            half = (tf - t0) / 2
            tk = (d.points.astype(LD) + 1) * half + t0                      # all nodes at once: arrays of N long doubles
            xs = [x[d.var0 + i * (N + 1):d.var0 + i * (N + 1) + N] for i in range(d.nx)]
            us = [x[d.u0 + j * N:d.u0 + (j + 1) * N] for j in range(d.nu)]
            ff, cc = f.dae(d.num, tk, xs, us, p, c)
            acc = sigma * d.weights.astype(LD) * f.lagrange(d.num, tk, xs, us, p, c)
            for o in range(d.nx):
                acc = acc - lam[d.g0 + o * N:d.g0 + (o + 1) * N] * ff[o]
            tot = tot + half * np.sum(acc)
            for o in range(d.nc):
                tot = tot + np.sum(lam[d.g0 + (d.nx + o) * N:d.g0 + (d.nx + o + 1) * N] * cc[o])
            x0 = [x[d.var0 + i * (N + 1)] for i in range(d.nx)]
            xf = [x[d.var0 + i * (N + 1) + N] for i in range(d.nx)]
            tot = tot + sigma * f.mayer(d.num, t0, x0, tf, xf, p, c)
            if d.ne:
                ev = f.event(d.num, t0, x0, tf, xf, p, c)
                for i in range(d.ne):
                    tot = tot + lam[d.g0 + (d.nx + d.nc) * N + i] * ev[i]
        for (il, ir, nl, g0) in self.links:
            a, b = self.ph[il], self.ph[ir]
            xl = [x[a.var0 + i * (a.N + 1) + a.N] for i in range(a.nx)]
            xr = [x[b.var0 + i * (b.N + 1)] for i in range(b.nx)]
            lo = f.link(xl, xr, [x[a.p0 + j] for j in range(a.nq)], [x[b.p0 + j] for j in range(b.nq)], c)
            for i in range(nl):
                tot = tot + lam[g0 + i] * lo[i]
        return tot

    def dense_central(self, x, sigma, lam, rel=LD(1e-5)):
        """Central second differences of (a) in long double: the dense n x n Hessian, O(h^2 + 2^-64 / h^2)."""
        x = np.asarray(x, dtype=LD)
        n = x.size
        h = [rel * (1 + abs(v)) for v in x]
        L = lambda y: self.lagrangian_nl(y, sigma, lam)      # noqa: E731
        H = np.zeros((n, n), dtype=LD)
        L0 = L(x)
        for i in range(n):
            xp, xm = x.copy(), x.copy()
            xp[i] += h[i]
            xm[i] -= h[i]
            H[i, i] = (L(xp) - 2 * L0 + L(xm)) / (h[i] * h[i])
        for (i, j) in self.coupled_pairs():
            v = []
            for si, sj in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                y = x.copy()
                y[i] += si * h[i]
                y[j] += sj * h[j]
                v.append(L(y))
            H[i, j] = H[j, i] = (v[0] - v[1] - v[2] + v[3]) / (4 * h[i] * h[j])
        return H

    def coupled_pairs(self):
        """Pairs i > j of variables that share a term of the Lagrangian (every other mixed derivative is exactly zero)."""
        out = set()
        for d in self.ph:
            N = d.N
            border = [d.t0, d.t0 + 1] + [d.p0 + j for j in range(d.nq)]
            for k in range(N):
                nodev = [d.var0 + i * (N + 1) + k for i in range(d.nx)] + [d.u0 + j * N + k for j in range(d.nu)]
                for a in nodev:
                    for b in nodev + border:
                        if a != b:
                            out.add((max(a, b), min(a, b)))
            ends = [d.var0 + i * (N + 1) for i in range(d.nx)] + [d.var0 + i * (N + 1) + N for i in range(d.nx)] + border
            for a in ends:
                for b in ends:
                    if a != b:
                        out.add((max(a, b), min(a, b)))
        for (il, ir, nl, g0) in self.links:
            a, b = self.ph[il], self.ph[ir]
            vs = ([a.var0 + i * (a.N + 1) + a.N for i in range(a.nx)] + [b.var0 + i * (b.N + 1) for i in range(b.nx)] +
                  [a.p0 + j for j in range(a.nq)] + [b.p0 + j for j in range(b.nq)])
            for u in vs:
                for w in vs:
                    if u != w:
                        out.add((max(u, w), min(u, w)))
        return sorted(out)

    # ---- the dependency probe (rpm_dep_probe_kernel): NaN propagation at node 1 of the guess ---------------------------------
    def dependencies(self, x_guess):
        """Per phase (nx + nc) x (nx + nu) flags, column-major, concatenated: what rpm_debug_hess_structure takes."""
        x = np.asarray(x_guess, dtype=np.float64)
        out = []
        for d in self.ph:
            N, t0, tf = d.N, x[d.t0], x[d.t0 + 1]
            tk = (d.points[1] + 1) * ((tf - t0) / 2.0) + t0
            p = [LD(x[d.p0 + j]) for j in range(d.nq)]
            for v in range(d.nx + d.nu):
                xs = [LD(np.nan) if i == v else LD(x[d.var0 + i * (N + 1) + 1]) for i in range(d.nx)]
                us = [LD(np.nan) if d.nx + j == v else LD(x[d.u0 + j * N + 1]) for j in range(d.nu)]
                ff, cc = self.f.dae(d.num, LD(tk), xs, us, p, self.c)
                out += [0 if np.isfinite(r) else 1 for r in list(ff) + list(cc)]
        return np.array(out, dtype=np.int32)

    # ---- structure: csrc/rpm_hess.cpp, entry by entry with the recipe of its value ---------------------------------------------
    def entries(self, dep):
        """[(row, col, recipe)] in COO order.  Recipes: ("blk", phase, a, b, k)  XI of pair (a, b) at node k;
        ("t0" | "tf", phase, v, k); ("tt", phase, 0 | 1 | 2)  t0t0, tft0, tftf; ("pt0" | "ptf", phase, i); ("pp", phase, i, j);
        ("end", phase, a, b, da, db); ("link", pair, a, b)."""
        dep = np.asarray(dep).ravel()
        out, off = [], 0
        for ip, d in enumerate(self.ph):
            nx, nu, nq, nc, N, sh = d.nx, d.nu, d.nq, d.nc, d.N, d.var0
            nv, nout = nx + nu, nx + nc
            D = dep[off:off + nv * nout].reshape(nv, nout).T          # rows: outputs, columns: variables
            off += nv * nout
            H = (D.T @ D) != 0
            np.fill_diagonal(H, True)
            I, E = [], []
            T0, TF, PE = 2 * nx, 2 * nx + 1, 2 * nx + 2
            for i in range(nx):
                for j in range(i + 1):
                    rs, cs = i * (N + 1), j * (N + 1)
                    if H[i, j]:
                        I += [(sh + rs + k, sh + cs + k, ("blk", ip, i, j, k)) for k in range(N)]
                    E.append((sh + rs, sh + cs, ("end", ip, i, j, i, j)))
                    if i != j:
                        E.append((sh + rs, sh + cs + N, ("end", ip, i, nx + j, i, nx + i)))
                    E.append((sh + rs + N, sh + cs, ("end", ip, nx + i, j, nx + i, j)))
                    E.append((sh + rs + N, sh + cs + N, ("end", ip, nx + i, nx + j, nx + i, nx + i)))
            rowshift = nx * (N + 1)
            for i in range(nu):
                rs = rowshift + i * N
                for j in range(nx):
                    if H[nx + i, j]:
                        I += [(sh + rs + k, sh + j * (N + 1) + k, ("blk", ip, nx + i, j, k)) for k in range(N)]
                for j in range(i + 1):
                    if H[nx + i, nx + j]:
                        I += [(sh + rs + k, sh + rowshift + j * N + k, ("blk", ip, nx + i, nx + j, k)) for k in range(N)]
            trow = nx * (N + 1) + nu * N
            for r in range(2):
                row, tv, nm = trow + r, (T0, TF)[r], ("t0", "tf")[r]
                for i in range(nx):
                    I += [(sh + row, sh + i * (N + 1) + k, (nm, ip, i, k)) for k in range(N)]
                    E.append((sh + row, sh + i * (N + 1), ("end", ip, tv, i, tv, i)))
                    E.append((sh + row, sh + i * (N + 1) + N, ("end", ip, tv, nx + i, tv, nx + i)))
                for i in range(nu):
                    I += [(sh + row, sh + rowshift + i * N + k, (nm, ip, nx + i, k)) for k in range(N)]
                if r == 0:
                    I.append((sh + row, sh + trow, ("tt", ip, 0)))
                    E.append((sh + row, sh + trow, ("end", ip, T0, T0, T0, T0)))
                else:
                    I.append((sh + row, sh + trow, ("tt", ip, 1)))
                    E.append((sh + row, sh + trow, ("end", ip, TF, T0, TF, T0)))
                    I.append((sh + row, sh + trow + 1, ("tt", ip, 2)))
                    E.append((sh + row, sh + trow + 1, ("end", ip, TF, TF, TF, TF)))
            for i in range(nq):
                row, pa = trow + 2 + i, nv + 1 + i
                for j in range(nx):
                    I += [(sh + row, sh + j * (N + 1) + k, ("blk", ip, pa, j, k)) for k in range(N)]
                    E.append((sh + row, sh + j * (N + 1), ("end", ip, PE + i, j, PE + i, j)))
                    E.append((sh + row, sh + j * (N + 1) + N, ("end", ip, PE + i, nx + j, PE + i, nx + j)))
                for j in range(nu):
                    I += [(sh + row, sh + rowshift + j * N + k, ("blk", ip, pa, nx + j, k)) for k in range(N)]
                I.append((sh + row, sh + trow, ("pt0", ip, i)))
                E.append((sh + row, sh + trow, ("end", ip, PE + i, T0, PE + i, T0)))
                I.append((sh + row, sh + trow + 1, ("ptf", ip, i)))
                E.append((sh + row, sh + trow + 1, ("end", ip, PE + i, TF, PE + i, TF)))
                for j in range(i + 1):
                    I.append((sh + row, sh + trow + 2 + j, ("pp", ip, i, j)))
                    E.append((sh + row, sh + trow + 2 + j, ("end", ip, PE + i, PE + j, PE + i, PE + j)))
            out += I + E
        for il, (l, r, nl, g0) in enumerate(self.links):
            a, b = self.ph[l], self.ph[r]
            nxl, nxr, nql, nqr = a.nx, b.nx, a.nq, b.nq
            PL, PR = nxl + nxr, nxl + nxr + nql
            NR = a.N if (nql == 0 and nqr == 0) else b.N
            xf_l = lambda j: a.var0 + (a.N + 1) * (j + 1) - 1      # noqa: E731
            p_l = lambda j: a.p0 + j                                # noqa: E731
            p_r = lambda j: b.p0 + j                                # noqa: E731
            for i in range(nxl):
                for j in range(i + 1):
                    out.append((xf_l(i), xf_l(j), ("link", il, i, j)))
            for i in range(nql):
                out += [(p_l(i), xf_l(j), ("link", il, PL + i, j)) for j in range(nxl)]
                out += [(p_l(i), p_l(j), ("link", il, PL + i, PL + j)) for j in range(i + 1)]
            for i in range(nxr):
                row = b.var0 + (b.N + 1) * i
                out += [(row, xf_l(j), ("link", il, j, nxl + i)) for j in range(nxl)]
                out += [(row, p_l(j), ("link", il, nxl + i, PL + j)) for j in range(nql)]
                out += [(row, b.var0 + (NR + 1) * j, ("link", il, nxl + i, nxl + j)) for j in range(i + 1)]
            for i in range(nqr):
                out += [(p_r(i), xf_l(j), ("link", il, PR + i, j)) for j in range(nxl)]
                out += [(p_r(i), p_l(j), ("link", il, PR + i, PL + j)) for j in range(nql)]
                out += [(p_r(i), b.var0 + (b.N + 1) * j, ("link", il, PR + i, nxl + j)) for j in range(nxr)]
                out += [(p_r(i), p_r(j), ("link", il, PR + i, PR + j)) for j in range(i + 1)]
        return out

    def structure(self, dep):
        e = self.entries(dep)
        return np.array([r for r, _, _ in e], dtype=np.int32), np.array([c for _, c, _ in e], dtype=np.int32)

    def reduced(self, dep):
        """Per entry: the node count N of its phase where the value is a sum over the nodes (the tt and parameter scalars of the
        I-part), else 0."""
        return np.array([self.ph[r[1]].N if r[0] in ("tt", "pt0", "ptf", "pp") else 0 for _, _, r in self.entries(dep)])

    def counts(self, dep):
        """(nI, nE) per phase."""
        out = []
        for ip in range(len(self.ph)):
            rec = [r for _, _, r in self.entries(dep) if r[0] != "link" and r[1] == ip]
            nE = sum(1 for r in rec if r[0] == "end")
            out.append((len(rec) - nE, nE))
        return out

    # ---- (b) ------------------------------------------------------------------------------------------------------------
    def walk(self, x, sigma, lam, step, dep):
        x = np.asarray(x, dtype=np.float64)
        lam = np.asarray(lam, dtype=np.float64)
        node = [_NodeTerms(self, d, x, float(sigma), lam, float(step)) for d in self.ph]
        ent = self.entries(dep)
        val, mag = np.zeros(len(ent), dtype=LD), np.zeros(len(ent), dtype=LD)
        for s, (_, _, r) in enumerate(ent):
            kind = r[0]
            if kind == "link":
                val[s], mag[s] = self._link(x, lam, float(step), r[1], r[2], r[3])
                continue
            T, d = node[r[1]], self.ph[r[1]]
            nv = d.nx + d.nu
            if kind == "blk":
                val[s], mag[s] = T.XI(r[2], r[3], r[4])
            elif kind in ("t0", "tf"):
                val[s], mag[s] = T.t_row(kind, nv, r[2], r[2], r[3])
            elif kind == "tt":
                val[s], mag[s] = _sum([T.tt(r[2], k) for k in range(d.N)])
            elif kind in ("pt0", "ptf"):
                pa = nv + 1 + r[2]
                val[s], mag[s] = _sum([T.t_row(kind[1:], pa, nv, pa, k) for k in range(d.N)])
            elif kind == "pp":
                val[s], mag[s] = _sum([T.XI(nv + 1 + r[2], nv + 1 + r[3], k) for k in range(d.N)])
            else:
                val[s], mag[s] = self._end(d, x, float(sigma), lam, float(step), *r[2:])
        hi, hj = self.structure(dep)
        return hi, hj, val, mag

    def dense(self, x, sigma, lam, step, dep):
        """The walk's triplets summed into a symmetric dense matrix (long double)."""
        hi, hj, v, _ = self.walk(x, sigma, lam, step, dep)
        H = np.zeros((self.n, self.n), dtype=LD)
        for i, j, w in zip(hi, hj, v):
            H[i, j] += w
            if i != j:
                H[j, i] += w
        return H

    def _end(self, d, x, sigma, lam, tol, a, b, da, db):
        nx, N = d.nx, d.N
        base = ([x[d.var0 + j * (N + 1)] for j in range(nx)] + [x[d.var0 + j * (N + 1) + N] for j in range(nx)] +
                [x[d.t0], x[d.t0 + 1]] + [x[d.p0 + j] for j in range(d.nq)])
        h = [tol * (1 + abs(v)) for v in base]
        den = LD(h[da] * h[db])
        M, EV = [], []
        for q in range(4):
            w = list(base)
            if q in (1, 3):
                w[a] = w[a] + h[a]
            if q in (2, 3):
                w[b] = w[b] + h[b]
            w = [LD(v) for v in w]
            args = (d.num, w[2 * nx], w[:nx], w[2 * nx + 1], w[nx:2 * nx], w[2 * nx + 2:], self.c)
            M.append(self.f.mayer(*args))
            EV.append(self.f.event(*args) if d.ne else [])
        sg = LD(sigma)
        val = sg * ((M[3] - M[1] - M[2] + M[0]) / den)
        mg = abs(sg) * ((abs(M[3]) + abs(M[1]) + abs(M[2]) + abs(M[0])) / den)
        for i in range(d.ne):
            le = LD(lam[d.g0 + (nx + d.nc) * N + i])
            val = val + ((EV[3][i] - EV[1][i] - EV[2][i] + EV[0][i]) / den) * le
            mg = mg + ((abs(EV[3][i]) + abs(EV[1][i]) + abs(EV[2][i]) + abs(EV[0][i])) / den) * abs(le)
        return val, mg

    def _link(self, x, lam, tol, il, a, b):
        l, r, nl, _ = self.links[il]
        A, B = self.ph[l], self.ph[r]
        nx, nq = A.nx, A.nq
        base = ([x[A.var0 + j * (A.N + 1) + A.N] for j in range(nx)] + [x[B.var0 + j * (B.N + 1)] for j in range(nx)] +
                [x[A.p0 + j] for j in range(nq)] + [x[B.p0 + j] for j in range(nq)])
        ha, hb = tol * (1 + abs(base[a])), tol * (1 + abs(base[b]))
        den = LD(ha * hb)
        LO = []
        for q in range(4):
            w = list(base)
            if q in (1, 3):
                w[a] = w[a] + ha
            if q in (2, 3):
                w[b] = w[b] + hb
            w = [LD(v) for v in w]
            LO.append(self.f.link(w[:nx], w[nx:2 * nx], w[2 * nx:2 * nx + nq], w[2 * nx + nq:], self.c))
        g0 = self.links[0][3]        # the first pair's multiplier rows for every pair (kept quirk of the reference)
        val = mg = LD(0)
        for i in range(nl):
            ll = LD(lam[g0 + i])
            val = val + ((LO[3][i] - LO[1][i] - LO[2][i] + LO[0][i]) / den) * ll
            mg = mg + ((abs(LO[3][i]) + abs(LO[1][i]) + abs(LO[2][i]) + abs(LO[0][i])) / den) * abs(ll)
        return val, mg


def _sum(pairs):
    v = m = LD(0)
    for a, b in pairs:
        v, m = v + a, m + b
    return v, m


class _NodeTerms:
    """The per-node terms of one phase: XI of a pair, the first-derivative piece D1 of a variable, both with magnitudes.
    Variables in the kernel's order [x.., u.., t, p..]."""

    def __init__(self, ref, d, x, sigma, lam, tol):
        self.ref, self.d, self.x, self.sigma, self.lam, self.tol = ref, d, x, sigma, lam, tol
        self.t0, self.tf = x[d.t0], x[d.t0 + 1]
        self.half = LD((self.tf - self.t0) / 2.0)
        self.F, self.xi, self.b = {}, {}, {}

    def base(self, k):
        if k not in self.b:
            d, x, N = self.d, self.x, self.d.N
            tk0 = (d.points[k] + 1) * ((self.tf - self.t0) / 2.0) + self.t0
            self.b[k] = ([x[d.var0 + i * (N + 1) + k] for i in range(d.nx)] + [x[d.u0 + j * N + k] for j in range(d.nu)] + [tk0] +
                         [x[d.p0 + j] for j in range(d.nq)])
        return list(self.b[k])

    def h(self, k, v):
        return self.tol * (1 + abs(self.base(k)[v]))

    def point(self, k, a, b):
        """[f.., c.., L] at node k with variables a and b stepped (-1: not), the point formed in double."""
        key = (k, a, b)
        if key not in self.F:
            d, f, c = self.d, self.ref.f, self.ref.c
            w = self.base(k)
            for v in (a, b):
                if v >= 0:
                    w[v] = w[v] + self.tol * (1 + abs(self.base(k)[v]))
            w = [LD(v) for v in w]
            xs, us, t, p = w[:d.nx], w[d.nx:d.nx + d.nu], w[d.nx + d.nu], w[d.nx + d.nu + 1:]
            ff, cc = f.dae(d.num, t, xs, us, p, c)
            self.F[key] = list(ff) + list(cc) + [f.lagrange(d.num, t, xs, us, p, c)]
        return self.F[key]

    def XI(self, a, b, k):
        key = (a, b, k)
        if key in self.xi:
            return self.xi[key]
        d, N = self.d, self.d.N
        den = LD(self.h(k, a) * self.h(k, b))
        Fab, Fa, Fb, F0 = self.point(k, a, b), self.point(k, a, -1), self.point(k, b, -1), self.point(k, -1, -1)
        d2 = lambda o: (Fab[o] - Fa[o] - Fb[o] + F0[o]) / den                            # noqa: E731
        m2 = lambda o: (abs(Fab[o]) + abs(Fa[o]) + abs(Fb[o]) + abs(F0[o])) / den        # noqa: E731
        sd = sdm = sp = spm = LD(0)
        for o in range(d.nx):
            lm = LD(self.lam[d.g0 + o * N + k])
            sd, sdm = sd + lm * d2(o), sdm + abs(lm) * m2(o)
        for o in range(d.nc):
            mu = LD(self.lam[d.g0 + (d.nx + o) * N + k])
            sp, spm = sp + mu * d2(d.nx + o), spm + abs(mu) * m2(d.nx + o)
        sw = LD(self.sigma * d.weights[k])
        il = d.nx + d.nc
        out = (self.half * (sw * d2(il) - sd) + sp, abs(self.half) * (abs(sw) * m2(il) + sdm) + spm)
        self.xi[key] = out
        return out

    def D1(self, v, k):
        d, N = self.d, self.d.N
        sw = LD(self.sigma * d.weights[k])
        sdd = sddm = LD(0)
        if self.ref.analytic:
            w = [LD(u) for u in self.base(k)]
            xs, us, t, p = w[:d.nx], w[d.nx:d.nx + d.nu], w[d.nx + d.nu], w[d.nx + d.nu + 1:]
            df = self.ref.f.dae_jac_col(d.num, v, t, xs, us, p, self.ref.c)
            dL = self.ref.f.lagrange_grad_col(d.num, v, t, xs, us, p, self.ref.c)
            for o in range(d.nx):
                lm = LD(self.lam[d.g0 + o * N + k])
                sdd, sddm = sdd + lm * df[o], sddm + abs(lm) * abs(df[o])
            return sdd - sw * dL, sddm + abs(sw) * abs(dL)
        hv = LD(self.h(k, v))
        Fv, F0 = self.point(k, v, -1), self.point(k, -1, -1)
        for o in range(d.nx):
            lm = LD(self.lam[d.g0 + o * N + k])
            sdd, sddm = sdd + lm * ((Fv[o] - F0[o]) / hv), sddm + abs(lm) * ((abs(Fv[o]) + abs(F0[o])) / hv)
        il = d.nx + d.nc
        return sdd - sw * ((Fv[il] - F0[il]) / hv), sddm + abs(sw) * ((abs(Fv[il]) + abs(F0[il])) / hv)

    def t_row(self, which, a, b, dv, k):
        """0.5 D1(dv) + ta XI(a, b) (which = "t0") or -0.5 D1(dv) + tb XI(a, b) ("tf") at node k."""
        tau = self.d.points[k]
        ta, tb = LD((1 - tau) / 2.0), LD((1 + tau) / 2.0)
        (xi, xim), (d1, d1m) = self.XI(a, b, k), self.D1(dv, k)
        if which == "t0":
            return LD(0.5) * d1 + ta * xi, LD(0.5) * d1m + ta * xim
        return LD(-0.5) * d1 + tb * xi, LD(0.5) * d1m + tb * xim

    def tt(self, which, k):
        """Per-node term of t0t0 (0), tft0 (1), tftf (2)."""
        nv = self.d.nx + self.d.nu
        tau = self.d.points[k]
        ta, tb = LD((1 - tau) / 2.0), LD((1 + tau) / 2.0)
        (xi, xim), (d1, d1m) = self.XI(nv, nv, k), self.D1(nv, k)
        if which == 0:
            return ta * (d1 + ta * xi), ta * (d1m + ta * xim)
        if which == 2:
            return tb * (-d1 + tb * xi), tb * (d1m + tb * xim)
        return LD(0.5) * ((tb - ta) * d1) + ta * (tb * xi), LD(0.5) * (abs(tb - ta) * d1m) + ta * (tb * xim)
