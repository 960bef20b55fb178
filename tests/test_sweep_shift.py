"""The receding-horizon shift of a sweep's plan and duals (rpm_shift_plan_batch*, rpm_sweep_shift_plan).

The reference is a numpy restatement written here operation by operation in double: post_time, the knots
2 (time[k] - time[0]) / (time[N] - time[0]) - 1, the forward recurrence and back substitution of the natural cubic spline, the
binary search, A, B, the cubes A * A * A, the clamp of s_q = tp[q] + 2 dt / (time[N] - time[0]) into [-1, 1], the costate and
path-density transforms of lambda before and after, the end-point costate -D(:, N)' lambda_s summed in ascending row order, and
the piecewise-linear rule A y[kl-1] + B y[kr-1] of z_L / z_U.  It is pinned without a device: at dt = 0 it returns its own
knots' values, and columns a + b t come back as a + b clip(t + dt, t0, tf).  The library is built with -ffp-contract=off, and on
the MI355X every one of the four cases came out equal to the restatement to the bit in x, lambda, z_L and z_U (the value of a
control or a path density at tau = 1 passes through pow(A, 3) in post_spline_end, and glibc's and the device's agreed on all of
them), so the comparison with the device asserts equal bits; the project's bound for the carry,
1e-12 * max(1, max|reference column|) per column, is checked and its worst figure printed first, so a failure shows how far off
it is.  Every other comparison is bit for bit too: dt = 0 against the
two carries onto the same engine, host against device form, every carry_tile, a forced column split, shares, an instance alone
against itself inside the batch, a replayed graph.

"dt >= H holds the end value" is checked where the clamp really gives s = 1.0: time[N] - time[0] is ((tf - t0) + t0) - t0, which
can differ from H = tf - t0 by an ulp, so with dt = H the first point alone (tp[0] = -1) may come out one ulp below 1; every
other point of such a row, and every point with dt = 1.5 H, must sit on the end value exactly.

Inputs: the seeded iterates and lambdas of test_sweep_carry*.py, z = RandomState(300 + b).uniform(0, 2) with the entries below
0.3 set to 0 (z >= 0); per instance and phase dt cycles through 0, 1e-9 H, 0.05 H, the advance that lands on the middle LGR
point, H, 1.5 H and -0.1 H (in steps of 3 through that list, so that 3 instances already meet a clamp).  Nothing depends on a
solve.
"""
import ctypes as C

import numpy as np
import pytest

import test_sweep_carry as sc
import test_sweep_carry_multipliers as scm
from lpopc_amd import problems
from lpopc_amd.engine import ABI_SYMBOLS, NLPEngine, RpmError, lib
from lpopc_amd.group import SweepGroup

F = np.float64
NEW_SYMBOLS = ["rpm_shift_plan_batch_dev", "rpm_shift_plan_batch", "rpm_sweep_shift_plan"]
TILES = (0, 1, 2, 4, 8)
CASES = ["hypersensitive", "ragged", "quadrotor", "oscillator"]
N_KINDS = 7


# ---- problems and inputs ------------------------------------------------------------------------------------------
def _makers(case):
    if case == "ragged":         # one interval list [5, 2, 7, 3]: a 2-node interval, unequal widths
        return [lambda p=p: sc._set_meshes(problems.quadrotor(4, 6, pref=p), sc.TARGETS["quadrotor"]["ragged"])
                for p in sc._quadrotor_prefs(5)]
    return sc._makers(case)      # hypersensitive 1x2 (3), quadrotor 4x6 (37), the ragged two-phase oscillator (9)


def _phases(eng):
    """Per phase what the restatement needs, from the problem description and the phase tables (host only); and the first
    row after the phases."""
    rows, tail0 = scm._rows(eng)
    out = []
    for p, ((off, N, nx, nu, nq), (g0, N2, nx2, nc, ne)) in enumerate(zip(sc._layout(eng), rows)):
        assert (N, nx) == (N2, nx2)
        t = eng.phase_tables(p)
        out.append(dict(off=off, N=N, nx=nx, nu=nu, nq=nq, g0=g0, nc=nc, ne=ne, pts=t["points"].astype(F),
                        w=t["weights"].astype(F), dN=scm._d_last_column(t, N).astype(F)))
    return out, tail0


def _duals(B, n):
    out = []
    for k in (0, 1):
        z = np.stack([np.random.RandomState(300 + 50 * k + b).uniform(0.0, 2.0, n) for b in range(B)])
        z[z < 0.3] = 0.0
        z.setflags(write=False)
        out.append(z)
    return out


def _horizons(phases, xs):
    """H = tf - t0 per instance and phase"""
    H = np.zeros((len(xs), len(phases)))
    for p, ph in enumerate(phases):
        it0 = ph["off"] + ph["nx"] * (ph["N"] + 1) + ph["nu"] * ph["N"]
        H[:, p] = xs[:, it0 + 1] - xs[:, it0]
    return H


def _kind(b, p):
    # a stride of 3 so that a batch of 3 already meets 1e-9 H, H and 0; phases of one instance differ, and where one phase has
    # dt = 0 the other has not
    return (3 * b + 3 * p + 1) % N_KINDS


def _dts(phases, xs):
    H = _horizons(phases, xs)
    dt = np.zeros_like(H)
    for b in range(len(xs)):
        for p, ph in enumerate(phases):
            h = H[b, p]
            dt[b, p] = (0.0, 1e-9 * h, 0.05 * h, (ph["pts"][ph["N"] // 2] + 1) * h / 2, h, 1.5 * h, -0.1 * h)[_kind(b, p)]
    return dt


_DATA, _REF = {}, {}


def _data(case):
    """-> dict(makers, phases, tail0, xs, lam, zl, zu, dt): built once per case (no device) and never changed"""
    if case not in _DATA:
        makers = _makers(case)
        xs = sc._source(case)[1] if case != "ragged" else sc._iterates([m() for m in makers])
        xs.setflags(write=False)
        one = NLPEngine(makers[0]())
        phases, tail0 = _phases(one)
        n, m = one.n, one.m
        one.close()
        zl, zu = _duals(len(xs), n)
        dt = _dts(phases, xs)
        dt.setflags(write=False)
        _DATA[case] = dict(makers=makers, phases=phases, tail0=tail0, xs=xs, lam=scm._lambdas(len(xs), m), zl=zl, zu=zu, dt=dt, n=n, m=m)
    return _DATA[case]


# ---- the restatement, operation by operation ------------------------------------------------------------------------
def _post_time(t0, tf, tau):
    return (tf - t0) * (tau + 1) / 2 + t0


def _knots(t0, tf, pts):
    time = _post_time(t0, tf, np.append(pts, F(1.0)))
    time_0, time_N = _post_time(t0, tf, pts[0]), _post_time(t0, tf, F(1.0))
    return 2 * (time - time_0) / (time_N - time_0) - 1, time_0, time_N


def _second(xd, y):
    """mu and z of the forward recurrence, the back substitution, interior c doubled"""
    M = len(xd)
    m, c, z = np.zeros(M), np.zeros(M), F(0.0)
    for i in range(1, M - 1):
        him1, hi = xd[i] - xd[i - 1], xd[i + 1] - xd[i]
        li = 2 * (xd[i + 1] - xd[i - 1]) - him1 * m[i - 1]
        m[i] = hi / li
        alpha = 3.0 / hi * (y[i + 1] - y[i]) - 3.0 / him1 * (y[i] - y[i - 1])
        z = (alpha - him1 * z) / li
        c[i] = z
    nxt = F(0.0)
    for j in range(M - 2, -1, -1):
        nxt = c[j] - m[j] * nxt
        c[j] = 2 * nxt if j >= 1 else nxt
    return c


def _locate(x, xd):
    kl, kr = 1, len(xd)
    for _ in range(32):
        if kr - kl <= 1:
            break
        k = (kr + kl) // 2
        if xd[k - 1] > x:
            kr = k
        else:
            kl = k
    h = xd[kr - 1] - xd[kl - 1]
    return kl, kr, h, (xd[kr - 1] - x) / h, (x - xd[kl - 1]) / h


def _cubic(x, xd, y, c):
    kl, kr, h, A, B = _locate(x, xd)
    Cc, Dd = (A * A * A - A) * (h * h) / 6.0, (B * B * B - B) * (h * h) / 6.0
    return A * y[kl - 1] + B * y[kr - 1] + Cc * c[kl - 1] + Dd * c[kr - 1]


def _linear(x, xd, y):
    """A y[kl-1] + B y[kr-1], held between the two knot values (A and B are rounded separately: next to a knot the sum can come
    out an ulp outside them); the comparisons let a NaN through"""
    kl, kr, h, A, B = _locate(x, xd)
    yl, yr = y[kl - 1], y[kr - 1]
    lo, hi = (yl, yr) if yl < yr else (yr, yl)
    v = A * yl + B * yr
    v = hi if v > hi else v
    return lo if v < lo else v


def _spline_end(pts, y):
    """the value at tau = 1 of the natural spline through the N points (post_spline_end; its cubes are pow(A, 3))"""
    N = len(pts)
    mu = z = F(0.0)
    for i in range(1, N - 1):
        him1, hi = pts[i] - pts[i - 1], pts[i + 1] - pts[i]
        alpha = 3.0 / hi * (y[i + 1] - y[i]) - 3.0 / him1 * (y[i] - y[i - 1])
        li = 2 * (pts[i + 1] - pts[i - 1]) - him1 * mu
        mu = hi / li
        z = (alpha - him1 * z) / li
    d2l = 2 * z if N - 2 >= 1 else F(0.0)
    h = pts[N - 1] - pts[N - 2]
    A, B = (pts[N - 1] - 1.0) / h, (1.0 - pts[N - 2]) / h
    Cc, Dd = (A ** 3.0 - A) * (h * h) / 6.0, (B ** 3.0 - B) * (h * h) / 6.0
    return A * y[N - 2] + B * y[N - 1] + Cc * d2l + Dd * 0.0


def _shifted(tau, dt, time_0, time_N):
    s = tau + 2 * dt / (time_N - time_0)
    s = F(1.0) if s > 1.0 else s
    return F(-1.0) if s < -1.0 else s


def _points(ph, dt, time_0, time_N):
    """the N shifted points and the shifted 1.0"""
    return [_shifted(ph["pts"][q], dt, time_0, time_N) for q in range(ph["N"])], _shifted(F(1.0), dt, time_0, time_N)


def _shift_ref(phases, tail0, dt, xs, lam=None, zl=None, zu=None):
    """-> dict(x, lambda, z_L, z_U) like the library's; arrays not given are left out"""
    B = len(xs)
    dt = np.asarray(dt, dtype=F).reshape(B, len(phases))
    out = {"x": np.full(xs.shape, np.nan)}
    if lam is not None:
        out["lambda"] = np.full(lam.shape, np.nan)
        out["lambda"][:, tail0:] = lam[:, tail0:]
    for key, z in (("z_L", zl), ("z_U", zu)):
        if z is not None:
            out[key] = np.full(z.shape, np.nan)
    with np.errstate(all="ignore"):
        for b in range(B):
            for p, ph in enumerate(phases):
                off, N, nx, nu, nq, g0, nc, ne, pts, w = (ph[k] for k in ("off", "N", "nx", "nu", "nq", "g0", "nc", "ne", "pts", "w"))
                M, u0 = N + 1, off + nx * (N + 1)
                it0 = u0 + nu * N
                xd, time_0, time_N = _knots(xs[b, it0], xs[b, it0 + 1], pts)
                sq, s1 = _points(ph, dt[b, p], time_0, time_N)
                xo = out["x"][b]
                for s in range(nx):
                    y = xs[b, off + s * M:off + (s + 1) * M]
                    c = _second(xd, y)
                    xo[off + s * M:off + (s + 1) * M] = [_cubic(v, xd, y, c) for v in sq + [s1]]
                for j in range(nu):
                    yn = xs[b, u0 + j * N:u0 + (j + 1) * N]
                    y = np.append(yn, _spline_end(pts, yn))
                    c = _second(xd, y)
                    xo[u0 + j * N:u0 + (j + 1) * N] = [_cubic(v, xd, y, c) for v in sq]
                xo[it0], xo[it0 + 1] = time_0, time_N
                xo[it0 + 2:it0 + 2 + nq] = xs[b, it0 + 2:it0 + 2 + nq]
                if lam is not None:
                    lo = out["lambda"][b]
                    for s in range(nx):
                        ls = lam[b, g0 + s * N:g0 + (s + 1) * N]
                        acc = F(0.0)
                        for r in np.flatnonzero(ph["dN"]):
                            acc += ph["dN"][r] * ls[r]
                        y = np.append(-((1 / w) * ls), -acc)
                        c = _second(xd, y)
                        lo[g0 + s * N:g0 + (s + 1) * N] = [-(w[q] * _cubic(sq[q], xd, y, c)) for q in range(N)]
                    p0 = g0 + N * nx
                    for j in range(nc):
                        yn = (1 / w) * lam[b, p0 + j * N:p0 + (j + 1) * N]
                        y = np.append(yn, _spline_end(pts, yn))
                        c = _second(xd, y)
                        lo[p0 + j * N:p0 + (j + 1) * N] = [w[q] * _cubic(sq[q], xd, y, c) for q in range(N)]
                    e0 = p0 + N * nc
                    lo[e0:e0 + ne] = lam[b, e0:e0 + ne]
                for key, z in (("z_L", zl), ("z_U", zu)):
                    if z is None:
                        continue
                    zo = out[key][b]
                    for s in range(nx):
                        y = z[b, off + s * M:off + (s + 1) * M]
                        zo[off + s * M:off + (s + 1) * M] = [_linear(v, xd, y) for v in sq + [s1]]
                    for j in range(nu):
                        yn = z[b, u0 + j * N:u0 + (j + 1) * N]
                        y = np.append(yn, yn[N - 1])                 # the knot at 1 holds the last node's value
                        zo[u0 + j * N:u0 + (j + 1) * N] = [_linear(v, xd, y) for v in sq]
                    zo[it0:it0 + 2 + nq] = z[b, it0:it0 + 2 + nq]
    return out


def _x_columns(phases):
    """-> (slices of the state and control columns, indices of t0 / tf / parameters)"""
    cols, scal = [], []
    for ph in phases:
        off, N, nx, nu, nq = (ph[k] for k in ("off", "N", "nx", "nu", "nq"))
        cols += [slice(off + s * (N + 1), off + (s + 1) * (N + 1)) for s in range(nx)]
        u0 = off + nx * (N + 1)
        cols += [slice(u0 + j * N, u0 + (j + 1) * N) for j in range(nu)]
        scal += list(range(u0 + nu * N, u0 + nu * N + 2 + nq))
    return cols, np.array(scal)


def _lam_columns(phases, tail0, m):
    cols, copied = [], []
    for ph in phases:
        g0, N, nx, nc, ne = (ph[k] for k in ("g0", "N", "nx", "nc", "ne"))
        cols += [slice(g0 + c * N, g0 + (c + 1) * N) for c in range(nx + nc)]
        copied += list(range(g0 + N * (nx + nc), g0 + N * (nx + nc) + ne))
    return cols, np.array(copied + list(range(tail0, m)), dtype=np.int64)


def _close(got, ref, cols, what):
    """the project's bound for the carry, per column; -> worst |got - ref| / max(1, max|ref column|)"""
    worst = 0.0
    for b in range(len(ref)):
        for c in cols:
            scale = max(1.0, np.abs(ref[b, c]).max())
            d = np.abs(got[b, c] - ref[b, c]).max()
            worst = max(worst, d / scale)
            assert d <= 1e-12 * scale, (what, b, c, d, scale)
    return worst


# ---- without a device -------------------------------------------------------------------------------------------
def test_symbols_exist_and_are_listed(built):
    import os
    L = lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rpm_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
    flat = " ".join(header.split())
    assert ("int rpm_shift_plan_batch_dev(rpm_engine* e, const double* d_dt, const double* d_x, double* d_x_out, const double* d_lambda, "
            "double* d_lambda_out, const double* d_z_L, const double* d_z_U, double* d_z_L_out, double* d_z_U_out, int* d_nonfinite, "
            "void* stream);") in flat
    assert ("int rpm_shift_plan_batch(rpm_engine* e, const double* dt, const double* x, double* x_out, const double* lambda, "
            "double* lambda_out, const double* z_L, const double* z_U, double* z_L_out, double* z_U_out, int* nonfinite);") in flat
    assert "int rpm_sweep_shift_plan(rpm_sweep* s, const double* dt, const double* x, double* x_out," in flat


def test_argument_errors_are_decided_on_the_host(built):
    L = lib()
    dp = C.POINTER(C.c_double)
    B = 4
    quad = NLPEngine(problems.quadrotor(3, 5), n_instances=B)
    n, m = quad.n, quad.m
    buf = np.zeros(B * (1 + 6 * n + 2 * m) + 8)
    at = lambda off: C.cast(C.c_void_p(buf.ctypes.data + 8 * off), dp)       # noqa: E731
    o = {"dt": 0, "x": B, "lam": B + B * n, "zl": B + B * (n + m), "zu": B + B * (2 * n + m), "xo": B + B * (3 * n + m),
         "lo": B + B * (4 * n + m), "zlo": B + B * (4 * n + 2 * m), "zuo": B + B * (5 * n + 2 * m)}
    order = ("dt", "x", "xo", "lam", "lo", "zl", "zu", "zlo", "zuo")

    def call(dev=False, **change):
        offs = dict(o, **change)
        args = [None if offs[k] is None else at(offs[k]) for k in order]
        if dev:
            return L.rpm_shift_plan_batch_dev(quad._h, *[None if a is None else C.cast(a, C.c_void_p) for a in args], None, None)
        return L.rpm_shift_plan_batch(quad._h, *args, None)

    def refused(code, text, **kw):
        for dev in (False, True):
            assert call(dev, **kw) == code, (kw, dev)
            assert text in quad.last_error(), quad.last_error()

    refused(1, "dt is NULL", dt=None)
    refused(1, "x is NULL", x=None)
    refused(1, "x_out is NULL", xo=None)
    refused(1, "lambda and lambda_out are given together or both NULL", lo=None)
    refused(1, "lambda and lambda_out are given together or both NULL", lam=None)
    for k in ("zl", "zu", "zlo", "zuo"):
        refused(1, "z_L, z_U, z_L_out and z_U_out are given together or all NULL", **{k: None})
    # an output over an input or another output, by one double
    refused(1, "x_out and x overlap", xo=o["x"] + B * n - 1)
    refused(1, "x_out and dt overlap", xo=0, x=o["xo"])
    refused(1, "lambda_out and lambda overlap", lo=o["lam"])
    refused(1, "x_out and lambda overlap", xo=o["lam"] - n * B + 1, x=o["xo"])
    refused(1, "z_L_out and z_U overlap", zlo=o["zu"], zuo=o["zlo"])
    refused(1, "z_L_out and z_U_out overlap", zlo=o["zuo"] - 1)
    refused(1, "x_out and z_U_out overlap", zuo=o["xo"] + B * n - 1)
    assert L.rpm_shift_plan_batch(None, at(0), at(0), at(0), None, None, None, None, None, None, None) == 1
    assert L.rpm_sweep_shift_plan(None, at(0), at(0), at(0), None, None, None, None, None, None, None) == 1
    # the Python wrapper checks sizes before the library sees a pointer
    with pytest.raises(RpmError) as ei:
        quad.shift_plan_batch(np.zeros(B + 1), np.zeros(B * n))
    assert "dt has 5 entries, expected 4" in str(ei.value)
    # interval sharding
    sh = NLPEngine(problems.launch(8, 8), shard_mode=1, shard_rank=1, shard_world=2)
    with pytest.raises(RpmError) as ei:
        sh.shift_plan_batch(np.zeros(4), np.zeros(sh.n))
    assert ei.value.code == 2 and "shift_plan_batch: not with interval sharding" in str(ei.value)
    # a column that cannot fit one workgroup's LDS
    quad.set_option("carry_lds_bytes", 8 * 16 * 3)
    with pytest.raises(RpmError) as ei:
        quad.shift_plan_batch(np.zeros(B), np.zeros(B * n))
    assert ei.value.code == 2 and "shift_plan_batch: a column of 16 knots does not fit one workgroup's LDS" in str(ei.value)
    quad.set_option("carry_lds_bytes", 0)
    quad.close()
    sh.close()


def test_no_gpu_means_loud_failure_not_fallback(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    a = NLPEngine(problems.quadrotor(3, 5), n_instances=2)
    with pytest.raises(RpmError) as ei:
        a.shift_plan_batch(np.zeros(2), np.zeros(2 * a.n))
    assert ei.value.code == 3 and "no CPU fallback" in str(ei.value)
    a.close()


def test_the_restatement_returns_its_own_knots_at_dt_zero(built):
    d = _data("oscillator")
    ph, tail0, xs, lam = d["phases"], d["tail0"], d["xs"][:3], d["lam"][:3]
    ref = _shift_ref(ph, tail0, np.zeros((3, 2)), xs, lam, d["zl"][:3], d["zu"][:3])
    cols, scal = _x_columns(ph)
    lcols, copied = _lam_columns(ph, tail0, d["m"])
    _close(ref["x"], xs, cols, "x")
    _close(ref["lambda"], lam, lcols, "lambda")
    _close(ref["z_L"], d["zl"][:3], cols, "z_L")
    _close(ref["z_U"], d["zu"][:3], cols, "z_U")
    assert np.array_equal(ref["lambda"][:, copied], lam[:, copied])
    assert copied.size == d["m"] - sum(h["N"] * (h["nx"] + h["nc"]) for h in ph) >= 2 + 1 + 4      # events, linkages
    assert np.array_equal(ref["z_L"][:, scal], d["zl"][:3][:, scal])
    par = np.array([i for ph_ in ph for i in range(ph_["off"] + ph_["nx"] * (ph_["N"] + 1) + ph_["nu"] * ph_["N"] + 2,
                                                    ph_["off"] + ph_["nx"] * (ph_["N"] + 1) + ph_["nu"] * ph_["N"] + 2 + ph_["nq"])])
    assert np.array_equal(ref["x"][:, par], xs[:, par]) and par.size == 4
    assert np.all(np.abs(ref["x"][:, scal] - xs[:, scal]) <= 2.0 ** -51 * np.maximum(1.0, np.abs(xs[:, scal])))   # t0 = time[0], tf = time[N]
    assert not np.isnan(ref["x"]).any() and not np.isnan(ref["lambda"]).any() and not np.isnan(ref["z_L"]).any()


def test_the_restatement_shifts_straight_lines_exactly(built):
    """columns a + b t, costates and path densities a + b t, z = a + b t >= 0: shifted by dt they are a + b clip(t + dt, t0, tf);
    the z of a control stops rising at its last node, where the piecewise-linear rule holds it"""
    d = _data("oscillator")
    ph, tail0, B = d["phases"], d["tail0"], N_KINDS
    xs, lam, zl = np.array(d["xs"][:B]), np.array(d["lam"][:B]), np.array(d["zl"][:B])
    dt = _dts(ph, xs)
    assert {_kind(b, 0) for b in range(B)} == set(range(N_KINDS))
    want_x, want_l, want_z = np.array(xs), np.array(lam), np.array(zl)
    rng = np.random.RandomState(5)
    for b in range(B):
        for p, h in enumerate(ph):
            off, N, nx, nu, nq, g0, nc, pts, w = (h[k] for k in ("off", "N", "nx", "nu", "nq", "g0", "nc", "pts", "w"))
            M, u0 = N + 1, off + nx * (N + 1)
            it0 = u0 + nu * N
            t0, tf = xs[b, it0], xs[b, it0 + 1]
            t = _post_time(t0, tf, np.append(pts, 1.0))
            ts = np.clip(t + dt[b, p], t0, tf) if tf > t0 else np.clip(t + dt[b, p], tf, t0)
            for c in range(nx + nu):
                a_, b_ = rng.uniform(-2, 2, 2)
                sl = slice(off + c * M, off + (c + 1) * M) if c < nx else slice(u0 + (c - nx) * N, u0 + (c - nx + 1) * N)
                k = M if c < nx else N
                xs[b, sl], want_x[b, sl] = a_ + b_ * t[:k], a_ + b_ * ts[:k]
                a_, b_ = rng.uniform(0.5, 2, 2) * (1.0, 0.1)
                base = abs(b_) * max(abs(t0), abs(tf))                  # keeps a + b t >= 0 whatever the sign of t
                zl[b, sl], want_z[b, sl] = a_ + base + b_ * t[:k], a_ + base + b_ * ts[:k]
                if c >= nx:        # z of a control: its knot at 1 holds the last node's value, so its last piece is flat
                    want_z[b, sl] = a_ + base + b_ * np.minimum(ts[:k], t[N - 1])
            for c in range(nx + nc):
                a_, b_ = rng.uniform(-2, 2, 2)
                sl = slice(g0 + c * N, g0 + (c + 1) * N)
                sign = -1.0 if c < nx else 1.0
                lam[b, sl], want_l[b, sl] = sign * w * (a_ + b_ * t[:N]), sign * w * (a_ + b_ * ts[:N])
    ref = _shift_ref(ph, tail0, dt, xs, lam, zl, zl)
    cols, _ = _x_columns(ph)
    lcols, _ = _lam_columns(ph, tail0, d["m"])
    print("straight lines: worst x %.2e, lambda %.2e, z %.2e (bound 1e-12)" % (
        _close(ref["x"], want_x, cols, "x"), _close(ref["lambda"], want_l, lcols, "lambda"), _close(ref["z_L"], want_z, cols, "z")))
    assert np.array_equal(ref["z_L"], ref["z_U"])


# ---- on the device ----------------------------------------------------------------------------------------------
def _engine(case):
    d = _data(case)
    return sc._batched([m() for m in d["makers"]]), d


def _shift(eng, d, dt=None, rows=slice(None)):
    return eng.shift_plan_batch(d["dt"][rows] if dt is None else dt, d["xs"][rows], d["lam"][rows], (d["zl"][rows], d["zu"][rows]))


KEYS = ("x", "lambda", "z_L", "z_U", "nonfinite")


def _same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_against_the_restatement(built, case):
    eng, d = _engine(case)
    if case not in _REF:
        _REF[case] = _shift_ref(d["phases"], d["tail0"], d["dt"], d["xs"], d["lam"], d["zl"], d["zu"])
    ref = _REF[case]
    got = _shift(eng, d)
    assert not got["nonfinite"].any() and all(np.isfinite(got[k]).all() for k in KEYS)
    cols, scal = _x_columns(d["phases"])
    lcols, copied = _lam_columns(d["phases"], d["tail0"], d["m"])
    worst = {k: _close(got[k], ref[k], lcols if k == "lambda" else cols, k) for k in KEYS[:4]}
    equal = {k: bool(np.array_equal(got[k], ref[k])) for k in KEYS[:4]}
    print("%s: worst |shifted - restatement| / max(1, max|column|): %s (bound 1e-12); equal to the bit: %s" % (
        case, ", ".join("%s %.2e" % kv for kv in worst.items()), equal))
    for k in ("x", "z_L", "z_U"):                                   # t0, tf, the parameters: to the bit
        assert np.array_equal(got[k][:, scal], ref[k][:, scal]), k
    assert all(equal.values()), equal                               # and so is everything else (see the module's docstring)
    assert np.array_equal(got["lambda"][:, copied], d["lam"][:, copied])      # event rows, the rows after the last phase
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_zero_dt_is_the_carry_onto_the_same_engine(built, case):
    eng, d = _engine(case)
    got = _shift(eng, d, np.zeros_like(d["dt"]))
    x_carry, xf = eng.carry_solution_batch(eng, d["xs"])
    l_carry, lf = eng.carry_multipliers_batch(eng, d["xs"], d["lam"])
    assert np.array_equal(got["x"], x_carry) and np.array_equal(got["lambda"], l_carry)
    assert not got["nonfinite"].any() and not xf.any() and not lf.any()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_exact_properties(built, case):
    eng, d = _engine(case)
    got = _shift(eng, d)
    B = len(d["xs"])
    kinds_held = 0
    for b in range(B):
        for p, ph in enumerate(d["phases"]):
            off, N, nx, nu, pts = (ph[k] for k in ("off", "N", "nx", "nu", "pts"))
            M, u0 = N + 1, off + nx * (N + 1)
            it0 = u0 + nu * N
            _, time_0, time_N = _knots(d["xs"][b, it0], d["xs"][b, it0 + 1], pts)
            sq, s1 = _points(ph, d["dt"][b, p], time_0, time_N)
            at_end = np.array([s == 1.0 for s in sq + [s1]])
            if _kind(b, p) in (4, 5):                               # dt = H: all but perhaps the first point; 1.5 H: all
                assert at_end[1:].all() and (at_end[0] or _kind(b, p) == 4)
                kinds_held += 1
            for c in range(nx + nu):
                k = M if c < nx else N
                sl = slice(off + c * M, off + (c + 1) * M) if c < nx else slice(u0 + (c - nx) * N, u0 + (c - nx + 1) * N)
                held = at_end[:k]
                # the column's end value: a state's own last entry; a control's spline value at 1, which every held entry shares
                row = got["x"][b, sl][held]
                if c < nx:
                    assert np.array_equal(row, np.full(row.size, d["xs"][b, sl][-1])), (case, b, c)
                elif row.size:
                    end = _spline_end(pts, d["xs"][b, sl])
                    assert np.array_equal(row, np.full(row.size, row[0])) and abs(row[0] - end) <= 1e-12 * max(1.0, np.abs(d["xs"][b, sl]).max())
                for key, z in (("z_L", d["zl"]), ("z_U", d["zu"])):
                    zin, zout = z[b, sl], got[key][b, sl]
                    assert np.array_equal(zout[held], np.full(int(held.sum()), zin[-1])), (case, key, b, c)
                    assert (zout >= 0).all() and zout.min() >= zin.min() and zout.max() <= zin.max(), (case, key, b, c)
    assert kinds_held >= 1
    # an instance alone equals itself inside the batch
    for b in sorted({1 % B, 4 % B, B - 1}):
        one = NLPEngine(d["makers"][b](), device=0)
        _same(_shift(one, d, rows=slice(b, b + 1)), {k: got[k][b:b + 1] for k in KEYS}, (case, "alone", b))
        one.close()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_every_form_tile_split_and_share_gives_the_same_bits(built, case):
    import torch
    eng, d = _engine(case)
    B = len(d["xs"])
    base = _shift(eng, d)
    s = torch.cuda.Stream()
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()             # noqa: E731
    d_dt, d_x, d_lam, d_zl, d_zu = (dev(d[k]) for k in ("dt", "xs", "lam", "zl", "zu"))
    outs = [torch.empty_like(t) for t in (d_x, d_lam, d_zl, d_zu)]
    d_flag = torch.empty(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for tile in TILES:
        eng.set_option("carry_tile", tile)
        _same(_shift(eng, d), base, (case, "host", tile))
        for _ in range(2):                                           # outputs pre-filled with NaN, twice
            for t in outs:
                t.fill_(float("nan"))
            d_flag.fill_(7)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                eng.shift_plan_batch_dev(d_dt, d_x, outs[0], d_lam, outs[1], d_zl, d_zu, outs[2], outs[3], d_flag, stream=s.cuda_stream)
            s.synchronize()
            _same(dict(zip(KEYS, [t.cpu().numpy() for t in outs + [d_flag]])), base, (case, "dev", tile))
    # x alone, without the verdicts
    outs[0].fill_(float("nan"))
    torch.cuda.synchronize()
    eng.shift_plan_batch_dev(d_dt, d_x, outs[0], stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(outs[0].cpu().numpy(), base["x"])
    eng.set_option("carry_tile", 0)
    if case == "quadrotor":                                          # columns dealt over several workgroups (25 knots, TB = 2)
        assert eng.get_option("carry_groups") == 1
        eng.set_option("carry_lds_bytes", 8 * 25 * (1 + 2 * 2 + 2 * 2 * 5))
        assert eng.get_option("carry_groups") == 4
        _same(_shift(eng, d), base, (case, "split"))
        eng.set_option("carry_lds_bytes", 0)
    g = SweepGroup(d["makers"][0](), [0, 0, 0], B)
    assert len(g.shares()) == 3
    _same(g.shift_plan(d["dt"], d["xs"], d["lam"], (d["zl"], d["zu"])), base, (case, "shares"))
    only_x = g.shift_plan(d["dt"], d["xs"])
    assert np.array_equal(only_x["x"], base["x"]) and set(only_x) == {"x", "nonfinite"}
    g.close()
    eng.close()


@pytest.mark.gpu
def test_spoiled_instances_are_flagged_and_disturb_nobody(built):
    eng, d = _engine("quadrotor")
    B = len(d["xs"])
    clean = _shift(eng, d)
    assert not clean["nonfinite"].any()
    xs, dt = np.array(d["xs"]), np.array(d["dt"])
    xs[17, 5] = np.nan                                               # a state value of instance 17
    dt[8, 0] = np.nan
    it0 = _x_columns(d["phases"])[1][0]
    xs[3, it0 + 1] = xs[3, it0]                                      # tf == t0 in instance 3
    got = eng.shift_plan_batch(dt, xs, d["lam"], (d["zl"], d["zu"]))
    want = np.zeros(B, dtype=np.int32)
    want[[3, 8, 17]] = 1
    assert np.array_equal(got["nonfinite"], want)
    ok = want == 0
    for k in KEYS[:4]:
        assert np.array_equal(got[k][ok], clean[k][ok]), k
    for b in (3, 8, 17):
        assert not np.isfinite(got["x"][b]).all()
    eng.close()


@pytest.mark.gpu
def test_captured_graph_of_shift_and_initial_states_replayed_on_new_inputs(built):
    import torch
    import test_ipm_warm_start as wsm
    from lpopc_amd.engine import BatchedIPM
    eng, XL, XU, idx, x0 = wsm._quadrotor_sweep()
    B, n, m = len(x0), eng.n, eng.m
    solver = BatchedIPM(eng)
    solver.set_all_bounds(XL, XU)
    rng = np.random.RandomState(21)
    xl, xu, _, _ = eng.get_bounds_info()
    mk_x = lambda seed: np.stack([problems.seeded_iterate(x0[b], xl, xu, seed + b) for b in range(B)])   # noqa: E731
    ins = lambda seed: (np.random.RandomState(seed).uniform(0.0, 0.5, (B, 1)), mk_x(seed),                # noqa: E731
                        np.random.RandomState(seed).standard_normal((B, m)), np.random.RandomState(seed + 1).uniform(0, 2, (B, n)),
                        np.random.RandomState(seed + 2).uniform(0, 2, (B, n)))
    first, second = ins(700), ins(800)
    s0_first, s0_second = rng.uniform(-0.2, 0.2, (B, 12)), rng.uniform(-0.2, 0.2, (B, 12))
    s = torch.cuda.Stream()
    d_in = [torch.from_numpy(a).cuda() for a in first]
    d_out = [torch.empty_like(t) for t in d_in[1:]]
    d_flag = torch.empty(B, dtype=torch.int32, device="cuda")
    d_s0 = torch.from_numpy(s0_first).cuda()
    torch.cuda.synchronize()

    def queue():
        eng.shift_plan_batch_dev(d_in[0], d_in[1], d_out[0], d_in[2], d_out[1], d_in[3], d_in[4], d_out[2], d_out[3], d_flag,
                                 stream=s.cuda_stream)
        solver.set_initial_states_dev(0, d_s0, stream=s.cuda_stream)

    queue()                                                          # the first call on the engine: the launch plans go up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        queue()
    for t, a in zip(d_in + [d_s0], second + (s0_second,)):
        t.copy_(torch.from_numpy(a).cuda())
    for t in d_out:
        t.fill_(float("nan"))
    d_flag.fill_(7)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    want = eng.shift_plan_batch(second[0], second[1], second[2], (second[3], second[4]))
    _same(dict(zip(KEYS, [t.cpu().numpy() for t in d_out + [d_flag]])), want, "graph")
    # the replayed states are the solver's bounds now: the solve equals the one after set_all_bounds with the same numbers
    after_graph = solver.solve(x0)
    XL2, XU2 = np.array(XL), np.array(XU)
    XL2[:, idx] = XU2[:, idx] = s0_second
    solver.set_all_bounds(XL2, XU2)
    direct = solver.solve(x0)
    for k in ("x", "lambda", "obj", "status", "iterations", "kkt_error"):
        assert np.array_equal(after_graph[k], direct[k]), k
    assert (direct["status"] == 0).all()
    solver.set_all_bounds(XL, XU)
    assert not np.array_equal(solver.solve(x0)["x"], direct["x"])    # and the states do matter
    del g
    solver.close()
    eng.close()
