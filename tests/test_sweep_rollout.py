"""The closed-loop plant of a sweep on the device: rpm_rollout_batch* (every instance's own dynamics integrated under its plan's
control) and rpm_sample_plan_batch* (the plans at caller-given times), with their sweep forms.

The reference is a numpy restatement in float64, operation by operation.  The spline is test_sweep_shift's (post_time, the knots,
the recurrences, the binary search, the cubes A * A * A, post_spline_end for a control's knot at 1) and is not written a second
time; what is new here is the coordinate of a time, s = 2 (t - time[0]) / (time[N] - time[0]) - 1 clamped into [-1, 1], and the
classical Runge-Kutta step exactly as the header states it: t_i = t_start + i h, stage times t_i, t_i + h / 2, t_i + h / 2,
t_i + h, stage states y + (h / 2) k1, y + (h / 2) k2, y + h k3, acc = k1; acc = acc + 2 k2; acc = acc + 2 k3; acc = acc + k4;
y = y + (h / 6) acc.  It is pinned without a device: dt = 0 returns the start state to the bit, sampling at time[k] returns the knot
values to the bit, and on Bryson-Denham and the parameter sled under a straight-line control, whose exact solutions are cubics that
RK4 integrates exactly, it meets the closed form evaluated in long double within n_steps * 32 ulp of max(1, largest magnitude on
the path).

Against the device the restatement is used where the functor calls no libm: hypersensitive 1 x 2 (B = 3, the smallest spline),
bryson_denham 2 x 3 (B = 5), param_sled(2, 4) (B = 5, the parameter read from x), and examples/user_problem_vanderpol.hpp in
test_z_user_rollout.py.  Plans are the seeded iterates of test_sweep_carry; dt cycles per instance through 0, 1e-9 H, 0.05 H, H,
1.5 H and -0.1 H.  The bound is the project's, 1e-12 * max(1, max|reference column|), and its worst figure is printed first.  The
library is built with -ffp-contract=off; on the MI355X every case, every n_steps, both holds and every start came out equal to the
restatement to the bit in state, traj, nonfinite and the samples (worst figure 0.00e+00 throughout), so the comparison asserts
equal bits, as test_sweep_shift does.  Everything else is an exact property and asserted bit for bit, except sampling at
time[k] + dt against shift_plan_batch (the two coordinates are formed differently: the 1e-12 bound) and hold = 1 against hold = 0
on constant non-zero controls (A y + B y is y only to an ulp: the 1e-12 bound over 0.05 H; with controls 0 it is exact over
every dt and asserted so).
"""
import ctypes as C
import os

import numpy as np
import pytest

import test_sweep_carry as sc
import test_sweep_carry_multipliers as scm
import test_sweep_shift as ss
from test_sweep_shift import _cubic, _knots, _locate, _post_time, _second, _spline_end   # noqa: F401  (the one restatement of the spline)
from lpopc_amd import problems
from lpopc_amd.engine import ABI_SYMBOLS, NLPEngine, RpmError, lib
from lpopc_amd.group import SweepGroup

F = np.float64
ULP = 2.0 ** -52
NEW_SYMBOLS = ["rpm_sample_plan_batch_dev", "rpm_sample_plan_batch", "rpm_sweep_sample_plan",
               "rpm_rollout_batch_dev", "rpm_rollout_batch", "rpm_sweep_rollout"]
TILES = (0, 1, 2, 4, 8)
STEPS = (1, 3, 8)
RK_CASES = ["hypersensitive", "bryson_denham", "param_sled"]          # functors without libm calls
ANY_CASES = ["quadrotor", "oscillator"]                                # exact properties and the sampler: any functor


# ---- the right-hand sides, as csrc/problems/problems.hpp writes them ----------------------------------------------------
def f_hypersensitive(t, y, u, par, c):
    return np.array([((-y[0]) * y[0]) * y[0] + u[0]])


def f_bryson_denham(t, y, u, par, c):
    return np.array([y[1], u[0], 0.5 * (u[0] * u[0])])


def f_param_sled(t, y, u, par, c):
    return np.array([y[1], par[0] * u[0]])


RHS = {"hypersensitive": f_hypersensitive, "bryson_denham": f_bryson_denham, "param_sled": f_param_sled}


# ---- problems and inputs ------------------------------------------------------------------------------------------------
def _makers(case):
    if case == "bryson_denham":
        return [lambda: problems.bryson_denham(2, 3)] * 5
    if case == "param_sled":
        return [lambda: problems.param_sled(2, 4)] * 5
    return sc._makers(case)          # hypersensitive 1 x 2 (3), quadrotor 4 x 6 (37), the ragged two-phase oscillator (9)


def _consts(case, makers):
    """Per instance the constants it runs under.  The quadrotor's dynamics read the mass c[0]: every instance gets its own."""
    out = [np.array(m().GetOpimalProblemFuns().consts, dtype=F) for m in makers]
    if case == "quadrotor":
        for b, c in enumerate(out):
            c[0] *= 1.0 + 0.01 * b
    return out


_DATA = {}


def _data(case):
    """-> dict(makers, consts, phases, xs, n, m, B): built once per case (no device) and never changed"""
    if case not in _DATA:
        makers = _makers(case)
        xs = sc._source(case)[1] if case in ("hypersensitive", "quadrotor", "oscillator") else sc._iterates([m() for m in makers])
        xs.setflags(write=False)
        one = NLPEngine(makers[0]())
        phases, _ = ss._phases(one)
        n, m = one.n, one.m
        one.close()
        _DATA[case] = dict(makers=makers, consts=_consts(case, makers), phases=phases, xs=xs, n=n, m=m, B=len(xs))
    return _DATA[case]


def _engine(case, rows=None, device=0):
    d = _data(case)
    rows = range(d["B"]) if rows is None else rows
    eng = NLPEngine(d["makers"][rows[0]](), n_instances=len(rows), device=device)
    for i, b in enumerate(rows):
        if len(d["consts"][b]):
            eng.set_instance_constants(i, d["consts"][b])
    return eng, d


def _t0tf(ph, xs):
    it0 = ph["off"] + ph["nx"] * (ph["N"] + 1) + ph["nu"] * ph["N"]
    return xs[:, it0], xs[:, it0 + 1]


def _dts(ph, xs):
    """per instance dt cycling through 0, 1e-9 H, 0.05 H, H, 1.5 H and -0.1 H"""
    t0, tf = _t0tf(ph, xs)
    H = tf - t0
    return np.array([(0.0, 1e-9 * h, 0.05 * h, h, 1.5 * h, -0.1 * h)[b % 6] for b, h in enumerate(H)])


def _starts(ph, xs, seed=7):
    """given start states and start times: states uniform in [-0.5, 0.5], times t0 + (0.1 + 0.2 (b mod 4)) H"""
    t0, tf = _t0tf(ph, xs)
    B = len(xs)
    s0 = np.random.RandomState(seed).uniform(-0.5, 0.5, (B, ph["nx"]))
    return s0, t0 + (0.1 + 0.2 * (np.arange(B) % 4)) * (tf - t0)


def _node_times(ph, xb):
    """time[0 .. N] of one instance, as the library forms them"""
    it0 = ph["off"] + ph["nx"] * (ph["N"] + 1) + ph["nu"] * ph["N"]
    return _post_time(xb[it0], xb[it0 + 1], np.append(ph["pts"], F(1.0)))


# ---- the restatement: the plan at time t, and RK4 under it ----------------------------------------------------------------
def _coord(t, time_0, time_N):
    s = 2 * (t - time_0) / (time_N - time_0) - 1
    s = F(1.0) if s > 1.0 else s
    return F(-1.0) if s < -1.0 else s


def _plan(ph, xb):
    """one instance's knots and its columns (values, second derivatives), states first; its static parameters"""
    off, N, nx, nu, nq, pts = (ph[k] for k in ("off", "N", "nx", "nu", "nq", "pts"))
    M, u0 = N + 1, off + nx * (N + 1)
    it0 = u0 + nu * N
    xd, time_0, time_N = _knots(xb[it0], xb[it0 + 1], pts)
    cols = []
    for s in range(nx):
        y = xb[off + s * M:off + (s + 1) * M]
        cols.append((y, _second(xd, y)))
    for j in range(nu):
        yn = xb[u0 + j * N:u0 + (j + 1) * N]
        y = np.append(yn, _spline_end(pts, yn))
        cols.append((y, _second(xd, y)))
    return dict(xd=xd, time_0=time_0, time_N=time_N, cols=cols, par=xb[it0 + 2:it0 + 2 + nq])


def _sample_ref(ph, xs, times):
    """-> (samples B x (nx + nu) x n_times, nonfinite B)"""
    B = len(xs)
    times = np.asarray(times, dtype=F).reshape(B, -1)
    out = np.zeros((B, ph["nx"] + ph["nu"], times.shape[1]))
    with np.errstate(all="ignore"):
        for b in range(B):
            pl = _plan(ph, xs[b])
            for q, t in enumerate(times[b]):
                s = _coord(t, pl["time_0"], pl["time_N"])
                out[b, :, q] = [_cubic(s, pl["xd"], y, c) for y, c in pl["cols"]]
    return out, (~np.isfinite(out).all(axis=(1, 2))).astype(np.int32)


def _rollout_ref(f, ph, xs, dt, n_steps, hold, state0=None, t_start=None, consts=None):
    """-> dict(state B x nx, traj B x (n_steps + 1) x nx, nonfinite B)"""
    B, nx = len(xs), ph["nx"]
    out = {"state": np.zeros((B, nx)), "traj": np.zeros((B, n_steps + 1, nx)), "nonfinite": np.zeros(B, dtype=np.int32)}
    with np.errstate(all="ignore"):
        for b in range(B):
            pl = _plan(ph, xs[b])
            c = None if consts is None else consts[b]

            def u_at(t):
                s = _coord(t, pl["time_0"], pl["time_N"])
                return np.array([_cubic(s, pl["xd"], yc, cc) for yc, cc in pl["cols"][nx:]])

            y = np.array(state0[b], dtype=F) if state0 is not None else np.array([yc[0] for yc, _ in pl["cols"][:nx]])
            ts = F(t_start[b]) if t_start is not None else pl["time_0"]
            h = F(dt[b]) / n_steps
            bad = not np.isfinite(y).all()
            out["traj"][b, 0] = y
            u = u_at(ts) if hold else None
            for i in range(n_steps):
                ti = ts + i * h
                k = f(ti, y, u if hold else u_at(ti), pl["par"], c)
                acc = k
                st = y + (h / 2) * k
                um = u if hold else u_at(ti + h / 2)
                k = f(ti + h / 2, st, um, pl["par"], c)
                acc = acc + 2 * k
                st = y + (h / 2) * k
                k = f(ti + h / 2, st, um, pl["par"], c)
                acc = acc + 2 * k
                st = y + h * k
                k = f(ti + h, st, u if hold else u_at(ti + h), pl["par"], c)
                acc = acc + k
                y = y + (h / 6) * acc
                bad = bad or not np.isfinite(y).all()
                out["traj"][b, i + 1] = y
            out["state"][b] = y
            out["nonfinite"][b] = 1 if bad else 0
    return out


def _close(got, ref, what):
    """the project's bound, per instance and column (the last axis runs along the column); where the reference is NaN or Inf the
    same must stand in `got`; -> worst |got - ref| / max(1, max|ref column|)"""
    worst = 0.0
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), (what, "non-finite entries differ")
    for idx in np.ndindex(*ref.shape[:-1]):
        r, g, ok = ref[idx], got[idx], fin[idx]
        if not ok.any():
            continue
        scale = max(1.0, np.abs(r[ok]).max())
        dist = np.abs(g[ok] - r[ok]).max()
        worst = max(worst, dist / scale)
        assert dist <= 1e-12 * scale, (what, idx, dist, scale)
    return worst


KEYS = ("state", "traj", "nonfinite")


def _same(got, want, what, keys=KEYS):
    for k in keys:
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)


# ---- without a device ---------------------------------------------------------------------------------------------------
def test_symbols_exist_and_are_listed(built):
    L = lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rpm_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
    flat = " ".join(header.split())
    assert ("int rpm_sample_plan_batch_dev(rpm_engine* e, int phase, const double* d_x, int n_times, const double* d_times, "
            "double* d_out, int* d_nonfinite, void* stream);") in flat
    assert ("int rpm_rollout_batch_dev(rpm_engine* e, int phase, const double* d_x, const double* d_t_start, const double* d_dt, "
            "int n_steps, int hold, const double* d_state0, double* d_state_out, double* d_traj, int* d_nonfinite, void* stream);") in flat
    assert "int rpm_sample_plan_batch(rpm_engine* e, int phase, const double* x, int n_times," in flat
    assert "int rpm_rollout_batch(rpm_engine* e, int phase, const double* x, const double* t_start," in flat
    assert "int rpm_sweep_sample_plan(rpm_sweep* s, int phase," in flat and "int rpm_sweep_rollout(rpm_sweep* s, int phase," in flat
    assert "not clipped" in flat.lower()                                 # the header says that controls are not clipped


def test_argument_errors_are_decided_on_the_host(built):
    L = lib()
    dp = C.POINTER(C.c_double)
    B, T, S = 4, 3, 5
    quad = NLPEngine(problems.quadrotor(3, 5), n_instances=B)
    n, nx, nu = quad.n, 12, 4
    # one buffer: x | times | out | t_start | dt | state0 | state_out | traj
    o = {"x": 0, "times": B * n, "out": B * n + B * T}
    o["ts"] = o["out"] + B * (nx + nu) * T
    o["dt"] = o["ts"] + B
    o["s0"] = o["dt"] + B
    o["so"] = o["s0"] + B * nx
    o["traj"] = o["so"] + B * nx
    buf = np.zeros(o["traj"] + B * (S + 1) * nx + 8)
    at = lambda off: None if off is None else C.cast(C.c_void_p(buf.ctypes.data + 8 * off), dp)       # noqa: E731
    vp = lambda p: None if p is None else C.cast(p, C.c_void_p)                                          # noqa: E731

    def sample(dev=False, phase=0, n_times=T, **change):
        f = dict(o, **change)
        a = [at(f["x"]), n_times, at(f["times"]), at(f["out"])]
        if dev:
            return L.rpm_sample_plan_batch_dev(quad._h, phase, vp(a[0]), a[1], vp(a[2]), vp(a[3]), None, None)
        return L.rpm_sample_plan_batch(quad._h, phase, *a, None)

    def rollout(dev=False, phase=0, n_steps=S, hold=0, **change):
        f = dict(o, **change)
        a = [at(f[k]) for k in ("x", "ts", "dt", "s0", "so", "traj")]
        if dev:
            return L.rpm_rollout_batch_dev(quad._h, phase, vp(a[0]), vp(a[1]), vp(a[2]), n_steps, hold, vp(a[3]), vp(a[4]), vp(a[5]), None, None)
        return L.rpm_rollout_batch(quad._h, phase, a[0], a[1], a[2], n_steps, hold, a[3], a[4], a[5], None)

    def refused(fn, code, text, **kw):
        for dev in (False, True):
            assert fn(dev, **kw) == code, (kw, dev)
            assert text in quad.last_error(), quad.last_error()

    refused(sample, 1, "sample_plan_batch: x is NULL", x=None)
    refused(sample, 1, "sample_plan_batch: times is NULL", times=None)
    refused(sample, 1, "sample_plan_batch: out is NULL", out=None)
    refused(sample, 1, "sample_plan_batch: n_times must be at least 1", n_times=0)
    refused(sample, 1, "sample_plan_batch: the phase index is out of range", phase=1)
    refused(sample, 1, "sample_plan_batch: the phase index is out of range", phase=-1)
    refused(sample, 1, "sample_plan_batch: out and x overlap", out=B * n - 1, times=o["out"])      # by one double
    refused(sample, 1, "sample_plan_batch: out and times overlap", out=o["times"] + B * T - 1)
    refused(rollout, 1, "rollout_batch: x is NULL", x=None)
    refused(rollout, 1, "rollout_batch: dt is NULL", dt=None)
    refused(rollout, 1, "rollout_batch: state_out is NULL", so=None)
    for bad in (0, -1, 65537):
        refused(rollout, 1, "rollout_batch: n_steps must be 1 ... 65536", n_steps=bad)
    for bad in (-1, 2):
        refused(rollout, 1, "rollout_batch: hold must be 0 or 1", hold=bad)
    refused(rollout, 1, "rollout_batch: the phase index is out of range", phase=1)
    refused(rollout, 1, "rollout_batch: state_out and x overlap", so=B * n - 1)
    refused(rollout, 1, "rollout_batch: state_out and dt overlap", so=o["dt"] + B - 1, s0=o["so"])
    refused(rollout, 1, "rollout_batch: state_out and t_start overlap", so=o["ts"], s0=o["so"])
    refused(rollout, 1, "rollout_batch: state_out and state0 overlap", so=o["s0"] + 1)               # in place is the same pointer only
    refused(rollout, 1, "rollout_batch: traj and state0 overlap", traj=o["s0"] + B * nx - 1, so=o["traj"])
    refused(rollout, 1, "rollout_batch: state_out and traj overlap", so=o["traj"] + B * (S + 1) * nx - 1)
    # in place, NULL t_start / state0 / traj: past the argument checks, then it needs a device (the host form only: these
    # are host arrays)
    assert rollout(False, so=o["s0"]) in (0, 3)
    assert rollout(False, ts=None, s0=None, traj=None) in (0, 3)
    assert L.rpm_sample_plan_batch(None, 0, at(0), 1, at(0), at(0), None) == 1
    assert L.rpm_rollout_batch(None, 0, at(0), None, at(0), 1, 0, None, at(0), None, None) == 1
    assert L.rpm_sweep_sample_plan(None, 0, at(0), 1, at(0), at(0), None) == 1
    assert L.rpm_sweep_rollout(None, 0, at(0), None, at(0), 1, 0, None, at(0), None, None) == 1
    # the Python wrappers check sizes before the library sees a pointer
    with pytest.raises(RpmError) as ei:
        quad.rollout_batch(0, np.zeros(B * n), np.zeros(B + 1), 4)
    assert "dt has 5 entries, expected 4" in str(ei.value)
    with pytest.raises(RpmError) as ei:
        quad.rollout_batch(0, np.zeros(B * n), np.zeros(B), 4, state0=np.zeros(B * nx - 1))
    assert "state0 has 47 entries, expected 48" in str(ei.value)
    with pytest.raises(RpmError) as ei:
        quad.sample_plan_batch(0, np.zeros(B * n), np.zeros(B * T + 1))
    assert "times has 13 entries, expected a multiple of 4" in str(ei.value)
    # interval sharding
    sh = NLPEngine(problems.launch(8, 8), shard_mode=1, shard_rank=1, shard_world=2)
    with pytest.raises(RpmError) as ei:
        sh.sample_plan_batch(0, np.zeros(sh.n), np.zeros(2))
    assert ei.value.code == 2 and "sample_plan_batch: not with interval sharding" in str(ei.value)
    with pytest.raises(RpmError) as ei:
        sh.rollout_batch(0, np.zeros(sh.n), np.zeros(1), 4)
    assert ei.value.code == 2 and "rollout_batch: not with interval sharding" in str(ei.value)
    # LDS: one column for the sampler; all nu control columns of an instance for the roll-out (16 knots, rows of 17 doubles)
    quad.set_option("carry_lds_bytes", 8 * 16 * 3)
    with pytest.raises(RpmError) as ei:
        quad.sample_plan_batch(0, np.zeros(B * n), np.zeros(B))
    assert ei.value.code == 2 and "sample_plan_batch: a column of 16 knots does not fit one workgroup's LDS" in str(ei.value)
    quad.set_option("carry_lds_bytes", 8 * 17 * (3 + 2 * nu) - 8)           # one double short of pts, tau, mu and 2 x 4 rows
    with pytest.raises(RpmError) as ei:
        quad.rollout_batch(0, np.zeros(B * n), np.zeros(B), 4)
    assert ei.value.code == 2 and "rollout_batch: the 4 control columns of 16 knots do not fit one workgroup's LDS" in str(ei.value)
    quad.set_option("carry_lds_bytes", 0)
    for bad in (3, 16, -1):
        with pytest.raises(RpmError):
            quad.set_option("rollout_tile", bad)
    for tile in TILES:
        quad.set_option("rollout_tile", tile)
        assert quad.get_option("rollout_tile") == tile
    quad.close()
    sh.close()


def test_no_gpu_means_loud_failure_not_fallback(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    a = NLPEngine(problems.quadrotor(3, 5), n_instances=2)
    with pytest.raises(RpmError) as ei:
        a.rollout_batch(0, np.zeros(2 * a.n), np.zeros(2), 4)
    assert ei.value.code == 3 and "no CPU fallback" in str(ei.value)
    with pytest.raises(RpmError) as ei:
        a.sample_plan_batch(0, np.zeros(2 * a.n), np.zeros(2))
    assert ei.value.code == 3 and "no CPU fallback" in str(ei.value)
    a.close()


def test_the_restatement_returns_the_start_state_at_dt_zero_and_its_knots_at_their_times(built):
    for case in ("oscillator", "bryson_denham"):
        d = _data(case)
        for ph in d["phases"]:
            xs = d["xs"]
            s0, ts = _starts(ph, xs)
            f = RHS.get(case, lambda t, y, u, par, c: np.array([y[1], (-(par[0] * y[0]) - c[0] * y[1]) + u[0]]))
            for hold in (0, 1):
                r = _rollout_ref(f, ph, xs, np.zeros(len(xs)), 3, hold, s0, ts, d["consts"])
                assert np.array_equal(r["state"], s0) and np.array_equal(r["traj"], np.repeat(s0[:, None, :], 4, axis=1))
                assert not r["nonfinite"].any()
            N, nx, nu, off = ph["N"], ph["nx"], ph["nu"], ph["off"]
            M, u0 = N + 1, off + nx * (N + 1)
            times = np.stack([_node_times(ph, xb) for xb in xs])
            got, flags = _sample_ref(ph, xs, times)
            assert not flags.any()
            for s in range(nx):
                assert np.array_equal(got[:, s, :], xs[:, off + s * M:off + (s + 1) * M]), (case, s)
            for j in range(nu):
                assert np.array_equal(got[:, nx + j, :N], xs[:, u0 + j * N:u0 + (j + 1) * N]), (case, j)
                ends = [_spline_end(ph["pts"], xb[u0 + j * N:u0 + (j + 1) * N]) for xb in xs]
                assert np.array_equal(got[:, nx + j, N], ends)
            # outside the horizon the end values are held
            far, _ = _sample_ref(ph, xs, np.stack([[t[0] - 3.0, t[-1] + 3.0] for t in times]))
            assert np.array_equal(far[:, :, 0], got[:, :, 0]) and np.array_equal(far[:, :, 1], got[:, :, N])


def _line_plan(case, a, b, p=None):
    """a plan on t0 = 0, tf = 2 whose control column is the straight line a + b t (and whose parameter is p)"""
    d = _data(case)
    ph = d["phases"][0]
    xb = np.array(d["xs"][0])
    off, N, nx, nu = ph["off"], ph["N"], ph["nx"], ph["nu"]
    u0 = off + nx * (N + 1)
    it0 = u0 + nu * N
    xb[it0], xb[it0 + 1] = 0.0, 2.0
    t = _node_times(ph, xb)
    assert t[0] == 0.0 and t[N] == 2.0
    xb[u0:u0 + N] = a + b * t[:N]
    if p is not None:
        xb[it0 + 2] = p
    return ph, xb[None, :]


@pytest.mark.parametrize("case", ["bryson_denham", "param_sled"])
def test_the_restatement_meets_the_closed_form_under_a_straight_line_control(built, case):
    """x' = v, v' = p u (p = 1 and e' = u^2 / 2 for Bryson-Denham), u = a + b t: cubics, which RK4 integrates exactly"""
    L = np.longdouble
    a, b, p = 0.8, -0.6, (1.7 if case == "param_sled" else None)
    ph, xs = _line_plan(case, a, b, p)
    y0 = np.array([[0.1, -0.2, 0.05][:ph["nx"]]])
    worst = 0.0
    for t_start in (None, 0.3):
        for n_steps in STEPS:
            dt = 0.7
            r = _rollout_ref(RHS[case], ph, xs, [dt], n_steps, 0, y0, None if t_start is None else [t_start], [np.array([0.5])])
            a_ = L(a) + L(b) * L(0.0 if t_start is None else t_start)         # u = a_ + b s, s the time since the start
            s = L(F(dt) / n_steps) * np.arange(n_steps + 1).astype(L)
            pp = L(1.0 if p is None else p)
            x0, v0 = L(y0[0, 0]), L(y0[0, 1])
            want = [x0 + v0 * s + pp * (a_ * s ** 2 / 2 + L(b) * s ** 3 / 6), v0 + pp * (a_ * s + L(b) * s ** 2 / 2)]
            if case == "bryson_denham":
                want.append(L(y0[0, 2]) + (a_ ** 2 * s + a_ * L(b) * s ** 2 + L(b) ** 2 * s ** 3 / 3) / 2)
            want = np.stack(want, axis=1)
            scale = max(1.0, float(np.abs(want).max()))
            err = float(np.abs(r["traj"][0].astype(L) - want).max())
            worst = max(worst, err / (n_steps * 32 * ULP * scale))
            assert err <= n_steps * 32 * ULP * scale, (case, t_start, n_steps, err / ULP, scale)
            assert np.array_equal(r["traj"][0, -1], r["state"][0])
    print("%s: worst |restatement - closed form| as a fraction of n_steps * 32 ulp * max(1, |path|): %.3f" % (case, worst))


# ---- on the device ------------------------------------------------------------------------------------------------------
def _starts_of(kind, ph, xs):
    """the four ways to start: state0 and t_start given or NULL"""
    s0, ts = _starts(ph, xs)
    return (s0 if kind & 1 else None), (ts if kind & 2 else None)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RK_CASES)
def test_rollout_against_the_restatement(built, case):
    eng, d = _engine(case)
    ph, xs = d["phases"][0], d["xs"]
    dt = _dts(ph, xs)
    worst, equal = 0.0, True
    for n_steps in STEPS:
        for hold in (0, 1):
            for kind in range(4):
                s0, ts = _starts_of(kind, ph, xs)
                ref = _rollout_ref(RHS[case], ph, xs, dt, n_steps, hold, s0, ts, d["consts"])
                got = eng.rollout_batch(0, xs, dt, n_steps, hold, s0, ts, traj=True)
                what = (case, n_steps, hold, kind)
                worst = max(worst, _close(got["state"][:, :, None], ref["state"][:, :, None], what),
                            _close(got["traj"].swapaxes(1, 2), ref["traj"].swapaxes(1, 2), what))
                assert np.array_equal(got["nonfinite"], ref["nonfinite"]), what
                equal = equal and all(np.array_equal(got[k], ref[k], equal_nan=True) for k in KEYS)
                assert np.array_equal(got["traj"][:, -1], got["state"], equal_nan=True) and np.array_equal(
                    got["traj"][:, 0], s0 if s0 is not None else got["traj"][:, 0])
    print("%s: worst |roll-out - restatement| / max(1, max|column|): %.2e (bound 1e-12); equal to the bit: %s" % (case, worst, equal))
    assert equal                                                         # see the module's docstring
    eng.close()


def _sample_times(ph, xs, n_times=7, seed=3):
    """per instance: before the horizon, its ends, inside it, past it"""
    t0, tf = _t0tf(ph, xs)
    u = np.random.RandomState(seed).uniform(-0.2, 1.2, (len(xs), n_times))
    u[:, 0], u[:, 1] = 0.0, 1.0
    return t0[:, None] + u * (tf - t0)[:, None]


@pytest.mark.gpu
@pytest.mark.parametrize("case", RK_CASES + ANY_CASES)
def test_sample_against_the_restatement(built, case):
    eng, d = _engine(case)
    worst, equal = 0.0, True
    for p, ph in enumerate(d["phases"]):
        times = _sample_times(ph, d["xs"])
        ref, rflags = _sample_ref(ph, d["xs"], times)
        got, flags = eng.sample_plan_batch(p, d["xs"], times)
        worst = max(worst, _close(got, ref, (case, p)))
        equal = equal and bool(np.array_equal(got, ref, equal_nan=True))
        assert np.array_equal(flags, rflags) and not flags.any()
    print("%s: worst |sample - restatement| / max(1, max|column|): %.2e (bound 1e-12); equal to the bit: %s" % (case, worst, equal))
    assert equal                                                         # see the module's docstring
    eng.close()


def _roll(eng, d, p, dt, n_steps=4, hold=0, kind=3, rows=None, xs=None, s0=None, ts=None):
    """a roll-out of phase p in the host form with the given starts of `kind`, over the instances `rows`"""
    ph = d["phases"][p]
    xs = d["xs"] if xs is None else xs
    a, b = _starts_of(kind, ph, d["xs"])
    s0 = a if s0 is None else s0
    ts = b if ts is None else ts
    rows = slice(None) if rows is None else rows
    cut = lambda v: None if v is None else v[rows]                       # noqa: E731
    return eng.rollout_batch(p, xs[rows], dt[rows], n_steps, hold, cut(s0), cut(ts), traj=True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ANY_CASES)
def test_exact_properties_of_the_rollout(built, case):
    import torch
    eng, d = _engine(case)
    B = d["B"]
    for p, ph in enumerate(d["phases"]):
        xs, nx = d["xs"], ph["nx"]
        dt = _dts(ph, xs)
        s0, ts = _starts(ph, xs)
        base = _roll(eng, d, p, dt)
        assert not base["nonfinite"].any() and np.isfinite(base["traj"]).all()
        assert np.array_equal(base["traj"][:, 0], s0) and np.array_equal(base["traj"][:, -1], base["state"])
        moved = np.abs(base["state"] - s0).max(axis=1) > 0
        assert np.array_equal(moved, dt != 0.0)                          # and the plant does move
        # dt = 0 returns state0; NULL state0 starts from the plan's own first state values
        zero = _roll(eng, d, p, np.zeros(B))
        assert np.array_equal(zero["state"], s0) and np.array_equal(zero["traj"], np.repeat(s0[:, None, :], 5, axis=1))
        own = _roll(eng, d, p, np.zeros(B), kind=0)
        M = ph["N"] + 1
        assert np.array_equal(own["state"], xs[:, ph["off"]:ph["off"] + nx * M:M])
        # n_steps = 2 over dt equals two calls with n_steps = 1 over dt / 2, the second from t_start + dt / 2
        for hold in (0, 1):
            two = _roll(eng, d, p, dt, 2, hold)
            first = _roll(eng, d, p, dt / 2, 1, hold)
            if hold == 0:
                second = _roll(eng, d, p, dt / 2, 1, hold, s0=first["state"], ts=ts + dt / 2)
                assert np.array_equal(two["state"], second["state"]) and np.array_equal(two["traj"][:, 2], second["traj"][:, 1])
            assert np.array_equal(two["traj"][:, :2], first["traj"])
        # the device form equals the host form; in place equals out of place; every rollout_tile gives the same bits
        s = torch.cuda.Stream()
        dev = lambda a: torch.from_numpy(np.array(a)).cuda()             # noqa: E731
        d_x, d_dt, d_s0, d_ts = dev(xs), dev(dt), dev(s0), dev(ts)
        d_out = torch.empty_like(d_s0)
        d_traj = torch.empty((B, 5, nx), dtype=torch.float64, device="cuda")
        d_flag = torch.empty(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for tile in TILES:
            eng.set_option("rollout_tile", tile)
            _same(_roll(eng, d, p, dt), base, (case, p, "host", tile))
            for t in (d_out, d_traj):
                t.fill_(float("nan"))
            d_flag.fill_(7)
            d_in = d_s0.clone()
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                eng.rollout_batch_dev(p, d_x, d_dt, 4, d_out, 0, d_s0, d_ts, d_traj, d_flag, stream=s.cuda_stream)
                eng.rollout_batch_dev(p, d_x, d_dt, 4, d_in, 0, d_in, d_ts, stream=s.cuda_stream)          # in place, nothing else
            s.synchronize()
            _same(dict(zip(KEYS, [t.cpu().numpy() for t in (d_out, d_traj, d_flag)])), base, (case, p, "dev", tile))
            assert np.array_equal(d_in.cpu().numpy(), base["state"]), (case, p, "in place", tile)
        eng.set_option("rollout_tile", 0)
        in_place = np.array(s0)
        L_ = eng._L
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))           # noqa: E731
        xs_c, dt_c, ts_c = np.ascontiguousarray(xs), np.ascontiguousarray(dt), np.ascontiguousarray(ts)
        assert L_.rpm_rollout_batch(eng._h, p, dp(xs_c), dp(ts_c), dp(dt_c), 4, 0, dp(in_place), dp(in_place), None, None) == 0
        assert np.array_equal(in_place, base["state"])                   # the host form in place
        # an instance alone equals itself inside the batch
        for b in sorted({1 % B, 4 % B, B - 1}):
            one, _ = _engine(case, rows=[b])
            _same(_roll(one, d, p, dt, rows=slice(b, b + 1)), {k: base[k][b:b + 1] for k in KEYS}, (case, p, "alone", b))
            one.close()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ANY_CASES)
def test_reversed_batch_shares_and_holds(built, case):
    eng, d = _engine(case)
    B = d["B"]
    rev, _ = _engine(case, rows=list(range(B))[::-1])
    g = SweepGroup(d["makers"][0](), [0, 0, 0], B)
    assert len(g.shares()) == 3
    for r, (first, count) in enumerate(g.shares()):                      # every share's instances get their own constants
        h = g._L.rpm_sweep_engine(g._h, r)
        for i in range(count):
            c = np.ascontiguousarray(d["consts"][first + i])
            if c.size:
                assert g._L.rpm_set_instance_constants(h, i, c.ctypes.data_as(C.POINTER(C.c_double)), int(c.size)) == 0
    for p, ph in enumerate(d["phases"]):
        xs, nx, nu, N, off = d["xs"], ph["nx"], ph["nu"], ph["N"], ph["off"]
        dt = _dts(ph, xs)
        s0, ts = _starts(ph, xs)
        base = _roll(eng, d, p, dt)
        back = rev.rollout_batch(p, xs[::-1], dt[::-1], 4, 0, s0[::-1], ts[::-1], traj=True)
        _same({k: back[k][::-1] for k in KEYS}, base, (case, p, "reversed"))
        _same(g.rollout(p, xs, dt, 4, 0, s0, ts, traj=True), base, (case, p, "shares"))
        times = _sample_times(ph, xs)
        sam, sflags = eng.sample_plan_batch(p, xs, times)
        gs, gflags = g.sample_plan(p, xs, times)
        assert np.array_equal(gs, sam) and np.array_equal(gflags, sflags)
        rs, _ = rev.sample_plan_batch(p, xs[::-1], times[::-1])
        assert np.array_equal(rs[::-1], sam)
        # hold = 1 equals hold = 0 on a plan whose control columns are constant: to the bit with the constant 0 (A 0 + B 0 is 0
        # at every stage time), over every dt of the cycle.  With another constant y the sampling rule returns A y + B y, which is
        # y to 1.5 ulp, so the two runs see controls 1.5 ulp apart: over 0.05 H (0.1 s of the quadrotor, under 2 |df/du| ~ 10,
        # a state difference of some 1e-16) they stay far inside the project's bound; over the whole horizon the quadrotor's
        # attitude dynamics amplify the ulp and no bound of this kind holds, so that run is not made.
        u0 = off + nx * (N + 1)
        t0_, tf_ = _t0tf(ph, xs)
        for const, exact in ((0.0, True), (None, False)):
            flat = np.array(xs)
            for j in range(nu):
                flat[:, u0 + j * N:u0 + (j + 1) * N] = const if const is not None else (0.3 + 0.1 * j + 0.01 * np.arange(B))[:, None]
            over = dt if exact else 0.05 * (tf_ - t0_)
            h0, h1 = _roll(eng, d, p, over, 4, 0, xs=flat), _roll(eng, d, p, over, 4, 1, xs=flat)
            if exact:
                _same(h1, h0, (case, p, "hold, controls 0"))
            else:
                _close(h1["traj"].swapaxes(1, 2), h0["traj"].swapaxes(1, 2), (case, p, "hold, constant controls"))
                assert np.array_equal(h1["nonfinite"], h0["nonfinite"])
    g.close()
    rev.close()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ANY_CASES)
def test_exact_properties_of_the_sampler(built, case):
    import torch
    eng, d = _engine(case)
    B, xs = d["B"], d["xs"]
    lam = scm._lambdas(B, d["m"])
    extracted, _ = eng.nlp2op_batch(xs, lam)
    shifted = None
    for p, ph in enumerate(d["phases"]):
        nx, nu, N, off = ph["nx"], ph["nu"], ph["N"], ph["off"]
        M, u0 = N + 1, off + nx * (N + 1)
        times = np.stack([_node_times(ph, xb) for xb in xs])
        assert np.array_equal(times, extracted[p]["time"])
        got, flags = eng.sample_plan_batch(p, xs, times)
        assert not flags.any()
        for s in range(nx):                                              # the node values, and the states' end values
            assert np.array_equal(got[:, s, :], xs[:, off + s * M:off + (s + 1) * M]), (case, p, s)
        for j in range(nu):                                              # at time[N]: the control-at-tau=1 row of nlp2op_batch
            assert np.array_equal(got[:, nx + j, :N], xs[:, u0 + j * N:u0 + (j + 1) * N]), (case, p, j)
            assert np.array_equal(got[:, nx + j, N], extracted[p]["control"][:, j * M + N]), (case, p, j)
        # time[k] + dt against the shift of the plan by dt: the 1e-12 bound (the coordinates are formed differently)
        all_dt = ss._dts(d["phases"], xs)
        if shifted is None:
            shifted = eng.shift_plan_batch(all_dt, xs)["x"]
        moved, _ = eng.sample_plan_batch(p, xs, times + all_dt[:, p:p + 1])
        want = np.concatenate([shifted[:, off:u0].reshape(B, nx, M)] +
                              [np.concatenate([shifted[:, u0:u0 + nu * N].reshape(B, nu, N), moved[:, nx:, N:]], axis=2)], axis=1)
        print("%s phase %d: worst |sample(time[k] + dt) - shifted plan| / max(1, max|column|): %.2e (bound 1e-12)" % (
            case, p, _close(moved, want, (case, p, "shift"))))
        # every carry_tile, the device form (outputs pre-filled with NaN), a forced small carry_lds
        some = _sample_times(ph, xs)
        base, bflags = eng.sample_plan_batch(p, xs, some)
        s = torch.cuda.Stream()
        d_x, d_t = torch.from_numpy(np.array(xs)).cuda(), torch.from_numpy(some).cuda()
        d_out = torch.empty((B, nx + nu, some.shape[1]), dtype=torch.float64, device="cuda")
        d_flag = torch.empty(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for tile in TILES:
            eng.set_option("carry_tile", tile)
            again, _ = eng.sample_plan_batch(p, xs, some)
            assert np.array_equal(again, base), (case, p, "host", tile)
            d_out.fill_(float("nan"))
            d_flag.fill_(7)
            torch.cuda.synchronize()
            eng.sample_plan_batch_dev(p, d_x, some.shape[1], d_t, d_out, d_flag, stream=s.cuda_stream)
            s.synchronize()
            assert np.array_equal(d_out.cpu().numpy(), base) and np.array_equal(d_flag.cpu().numpy(), bflags), (case, p, "dev", tile)
        eng.set_option("carry_tile", 0)
        groups = eng.get_option("carry_groups")
        eng.set_option("carry_lds_bytes", 8 * (max(h["N"] for h in d["phases"]) + 2) * (1 + 2 * 2 + 2 * 2 * 2))   # two columns of two instances
        assert eng.get_option("carry_groups") > groups
        split, _ = eng.sample_plan_batch(p, xs, some)
        assert np.array_equal(split, base), (case, p, "split")
        eng.set_option("carry_lds_bytes", 0)
        for b in sorted({1 % B, B - 1}):                                 # an instance alone
            one, _ = _engine(case, rows=[b])
            alone, _ = one.sample_plan_batch(p, xs[b:b + 1], some[b:b + 1])
            assert np.array_equal(alone, base[b:b + 1]), (case, p, "alone", b)
            one.close()
    eng.close()


@pytest.mark.gpu
def test_spoiled_instances_are_flagged_and_disturb_nobody(built):
    eng, d = _engine("quadrotor")
    ph, xs, B = d["phases"][0], d["xs"], d["B"]
    dt = _dts(ph, xs)
    s0, ts = _starts(ph, xs)
    clean = _roll(eng, d, 0, dt)
    times = _sample_times(ph, xs)
    sam, sflags = eng.sample_plan_batch(0, xs, times)
    assert not clean["nonfinite"].any() and not sflags.any()
    u0 = ph["off"] + ph["nx"] * (ph["N"] + 1)
    it0 = u0 + ph["nu"] * ph["N"]
    for kind, b in (("dt", 8), ("state0", 17), ("control", 3), ("horizon", 36), ("t_start", 0)):      # one instance at a time
        xs2, dt2, s02, ts2 = np.array(xs), np.array(dt), np.array(s0), np.array(ts)
        if kind == "dt":
            dt2[b] = np.nan
        elif kind == "state0":
            s02[b, 5] = np.nan
        elif kind == "control":
            xs2[b, u0 + 7] = np.nan
        elif kind == "t_start":
            ts2[b] = np.nan
        else:
            xs2[b, it0 + 1] = xs2[b, it0]                                # tf == t0
        got = _roll(eng, d, 0, dt2, xs=xs2, s0=s02, ts=ts2)
        want = np.zeros(B, dtype=np.int32)
        want[b] = 1
        assert np.array_equal(got["nonfinite"], want), kind
        ok = want == 0
        for k in KEYS:
            assert np.array_equal(got[k][ok], clean[k][ok]), (kind, k)
        assert not np.isfinite(got["state"][b]).all(), kind
        if kind in ("control", "horizon"):                               # the sampler reads these too
            got_s, flags = eng.sample_plan_batch(0, xs2, times)
            assert np.array_equal(flags, want) and np.array_equal(got_s[ok], sam[ok]), kind
    t2 = np.array(times)
    t2[5, 2] = np.nan
    got_s, flags = eng.sample_plan_batch(0, xs, t2)
    want = np.zeros(B, dtype=np.int32)
    want[5] = 1
    assert np.array_equal(flags, want) and np.array_equal(got_s[want == 0], sam[want == 0])
    eng.close()


@pytest.mark.gpu
def test_captured_graph_of_rollout_and_initial_states_replayed_on_new_inputs(built):
    import torch
    import test_ipm_warm_start as wsm
    from lpopc_amd.engine import BatchedIPM
    eng, XL, XU, idx, x0 = wsm._quadrotor_sweep()
    B, n = len(x0), eng.n
    solver = BatchedIPM(eng)
    solver.set_all_bounds(XL, XU)
    xl, xu, _, _ = eng.get_bounds_info()
    mk_x = lambda seed: np.stack([problems.seeded_iterate(x0[b], xl, xu, seed + b) for b in range(B)])   # noqa: E731
    rng = np.random.RandomState(21)
    plans = [mk_x(700), mk_x(800)]
    states = [rng.uniform(-0.2, 0.2, (B, 12)), rng.uniform(-0.2, 0.2, (B, 12))]
    dts = [np.full(B, 0.1), np.array([0.1, 0.05, 0.2])]
    s = torch.cuda.Stream()
    d_x, d_dt, d_s0 = (torch.from_numpy(a[0]).cuda() for a in (plans, dts, states))
    d_flag = torch.empty(B, dtype=torch.int32, device="cuda")
    d_times = torch.from_numpy(np.tile(np.linspace(0.0, 0.4, 5), (B, 1))).cuda()
    d_sam = torch.empty((B, 16, 5), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def queue():
        eng.rollout_batch_dev(0, d_x, d_dt, 4, d_s0, 0, d_s0, None, None, d_flag, stream=s.cuda_stream)      # in place
        solver.set_initial_states_dev(0, d_s0, stream=s.cuda_stream)
        eng.sample_plan_batch_dev(0, d_x, 5, d_times, d_sam, stream=s.cuda_stream)

    queue()                                                          # the first call on the engine: the launch plan goes up
    s.synchronize()
    assert np.array_equal(d_s0.cpu().numpy(), eng.rollout_batch(0, plans[0], dts[0], 4, 0, states[0])["state"])
    held = torch.cuda.memory_allocated()
    for _ in range(3):                                               # the second and later direct calls allocate nothing
        queue()
    s.synchronize()
    assert torch.cuda.memory_allocated() == held
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        queue()
    for t, a in zip((d_x, d_dt, d_s0), (plans[1], dts[1], states[1])):
        t.copy_(torch.from_numpy(a).cuda())
    d_flag.fill_(7)
    d_sam.fill_(float("nan"))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    want = eng.rollout_batch(0, plans[1], dts[1], 4, 0, states[1])
    next_state = d_s0.cpu().numpy()
    assert np.array_equal(next_state, want["state"]) and np.array_equal(d_flag.cpu().numpy(), want["nonfinite"])
    assert not np.array_equal(next_state, states[1])
    assert np.array_equal(d_sam.cpu().numpy(), eng.sample_plan_batch(0, plans[1], d_times.cpu().numpy())[0])
    # the replayed states are the solver's bounds now: the solve equals the one after set_all_bounds with the same numbers
    after_graph = solver.solve(x0)
    XL2, XU2 = np.array(XL), np.array(XU)
    XL2[:, idx] = XU2[:, idx] = next_state
    solver.set_all_bounds(XL2, XU2)
    direct = solver.solve(x0)
    for k in ("x", "lambda", "obj", "status", "iterations", "kkt_error"):
        assert np.array_equal(after_graph[k], direct[k], equal_nan=True), k
    solver.set_all_bounds(XL, XU)
    assert not np.array_equal(solver.solve(x0)["x"], direct["x"])    # and the states do matter
    del g
    solver.close()
    eng.close()
