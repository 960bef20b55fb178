"""One process, several GPUs: rpm_group_* (include/rpm_hip.h) — the mesh intervals of ONE NLP sharded over the devices of
a node behind the C ABI, for the caller lpopc actually has: a single-process NLPSolver::SolveNlp driving one TNLP object
from one thread (Core/LpNLPSolver.cpp:13-53).  Method names follow LpopcIpopt (Core/LpopcIpopt.h:33-82).  Nothing here
computes; host arrays are numpy float64, device arrays torch CUDA tensors (HBM handles)."""
import ctypes as C

import numpy as np

from . import _abi
from .engine import RPM_E_INVALID, RPM_OK, RpmError, _batch_estimate, _batch_extract, _dp, _extract_layout, _ip, _phase_shapes, _rollout, _sample_plan, _shift_plan, lib


class _EngineView:
    """rpm_group_engine(g, rank): set-up calls and options of one member engine (borrowed handle, never destroyed here)."""

    def __init__(self, L, h):
        self._L, self._h = L, h

    def get_option(self, key):
        v = C.c_int()
        rc = self._L.rpm_get_option(self._h, key.encode(), C.byref(v))
        if rc != RPM_OK:
            raise RpmError(rc, self._L.rpm_last_error(self._h).decode())
        return v.value


class EngineGroup:
    """One interval-sharded engine per entry of `devices` (a device may be listed more than once).  The host-consumer
    methods take caller-owned numpy arrays that every device addresses directly: they are page-locked on first sight and must
    stay allocated until close() or release_arrays()."""

    def __init__(self, problem, devices, options=None, n_instances=1):
        self._L = lib(getattr(problem.GetOpimalProblemFuns(), "library", None))
        self._desc, self._keep = _abi.lower(problem, options, n_instances, 0, 0, 1)
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self._L.rpm_group_create(C.byref(self._desc), len(devices), devs, C.byref(h))
        if rc != RPM_OK:
            raise RpmError(rc, self._L.rpm_group_last_error(None).decode())
        self._h = h
        self.size = self._L.rpm_group_size(h)
        e0 = self._L.rpm_group_engine(h, 0)
        n, m, nj, nh, st = (C.c_int() for _ in range(5))
        self._check(self._L.rpm_get_nlp_info(e0, C.byref(n), C.byref(m), C.byref(nj), C.byref(nh), C.byref(st)))
        self.n, self.m, self.nnz_jac, self.nnz_h = n.value, m.value, nj.value, nh.value
        self.n_instances = n_instances

    def close(self):
        if getattr(self, "_h", None):
            self._L.rpm_group_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc != RPM_OK:
            raise RpmError(rc, self._L.rpm_group_last_error(self._h).decode())

    def engine(self, rank):
        h = self._L.rpm_group_engine(self._h, int(rank))
        if not h:
            raise RpmError(RPM_E_INVALID, "no such rank")
        return _EngineView(self._L, h)

    def device_init(self):
        self._check(self._L.rpm_group_device_init(self._h))

    def set_option(self, key, value):
        self._check(self._L.rpm_group_set_option(self._h, key.encode(), int(value)))

    def release_arrays(self):
        """Let go of every page-locked caller array (before freeing them)."""
        self.set_option("pin_host", 0)

    def _x(self, x):
        if not (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous and x.size == self.n * self.n_instances):
            raise RpmError(RPM_E_INVALID, "x must be a caller-owned contiguous float64 array of n * n_instances entries")
        return x

    # ---- host consumer -----------------------------------------------------------------------------------------------
    def eval_f(self, x, new_x=True):
        out = np.zeros(self.n_instances)
        self._check(self._L.rpm_group_eval_f(self._h, self.n, _dp(self._x(x)), int(new_x), _dp(out)))
        return float(out[0]) if self.n_instances == 1 else out

    def eval_grad_f(self, x, out, new_x=True):
        self._check(self._L.rpm_group_eval_grad_f(self._h, self.n, _dp(self._x(x)), int(new_x), _dp(out)))
        return out

    def eval_g(self, x, out, new_x=True):
        self._check(self._L.rpm_group_eval_g(self._h, self.n, _dp(self._x(x)), int(new_x), self.m, _dp(out)))
        return out

    def eval_jac_g_structure(self):
        i, j = np.zeros(self.nnz_jac, dtype=np.int32), np.zeros(self.nnz_jac, dtype=np.int32)
        self._check(self._L.rpm_group_eval_jac_g(self._h, self.n, None, 0, self.m, self.nnz_jac, _ip(i), _ip(j), None))
        return i, j

    def eval_jac_g(self, x, out, new_x=True):
        self._check(self._L.rpm_group_eval_jac_g(self._h, self.n, _dp(self._x(x)), int(new_x), self.m, self.nnz_jac, None, None, _dp(out)))
        return out

    def eval_pair(self, x, g_out, values_out):
        self._check(self._L.rpm_group_eval_pair(self._h, self.n, _dp(self._x(x)), self.m, _dp(g_out), self.nnz_jac, _dp(values_out)))
        return g_out, values_out

    # ---- device consumer ---------------------------------------------------------------------------------------------
    def eval_pair_dev(self, home, d_x, d_g, d_values):
        """x, g, values in the HBM of rank `home`'s device; the other ranks store into them over xGMI.  Blocking."""
        self._check(self._L.rpm_group_eval_pair_dev(self._h, int(home), C.c_void_p(d_x.data_ptr()), C.c_void_p(d_g.data_ptr()),
                                                    C.c_void_p(d_values.data_ptr())))

    def allgather_pair_dev(self, d_x, d_g, d_values):
        """Lists of per-rank tensors (each on its rank's device); afterwards every rank's g / values are complete.  Blocking."""
        arr = lambda ts: (C.c_void_p * self.size)(*[t.data_ptr() for t in ts])   # noqa: E731
        self._check(self._L.rpm_group_allgather_pair_dev(self._h, arr(d_x), arr(d_g), arr(d_values)))


class SweepGroup:
    """rpm_sweep_*: the batched device solver (BatchedIPM) over several GPUs from one process — the B instances of one
    transcription dealt to `devices` in contiguous shares, solved side by side (a host thread per share inside the library)."""

    def __init__(self, problem, devices, n_instances, options=None, **solver_options):
        self._L = lib(getattr(problem.GetOpimalProblemFuns(), "library", None))
        self._desc, self._keep = _abi.lower(problem, options, n_instances, 0, 0, 1)
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self._L.rpm_sweep_create(C.byref(self._desc), len(devices), devs, C.byref(h))
        if rc != RPM_OK:
            raise RpmError(rc, self._L.rpm_sweep_last_error(None).decode())
        self._h = h
        self.size = self._L.rpm_sweep_size(h)
        self.n_instances = int(n_instances)
        e0 = self._L.rpm_sweep_engine(h, 0)
        n, m, nj, nh, st = (C.c_int() for _ in range(5))
        self._check(self._L.rpm_get_nlp_info(e0, C.byref(n), C.byref(m), C.byref(nj), C.byref(nh), C.byref(st)))
        self.n, self.m = n.value, m.value
        self.n_phases = problem.GetPhaseNum()
        for k, v in solver_options.items():
            self.set_option(k, v)

    def close(self):
        if getattr(self, "_h", None):
            self._L.rpm_sweep_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc != RPM_OK:
            raise RpmError(rc, self._L.rpm_sweep_last_error(self._h).decode())

    def shares(self):
        out = []
        for r in range(self.size):
            a, b = C.c_int(), C.c_int()
            self._check(self._L.rpm_sweep_share(self._h, r, C.byref(a), C.byref(b)))
            out.append((a.value, b.value))
        return out

    def set_option(self, key, value):
        if key == "mu_strategy" and isinstance(value, str):
            value = {"monotone": 0, "adaptive": 1}[value]
        self._check(self._L.rpm_sweep_set_option(self._h, key.encode(), float(value)))

    def set_bounds(self, instance, x_l, x_u):
        x_l, x_u = np.ascontiguousarray(x_l, dtype=np.float64), np.ascontiguousarray(x_u, dtype=np.float64)
        assert x_l.size == self.n and x_u.size == self.n
        self._check(self._L.rpm_sweep_set_bounds(self._h, int(instance), _dp(x_l), _dp(x_u)))

    def solve(self, x0):
        B = self.n_instances
        x = np.ascontiguousarray(x0, dtype=np.float64).reshape(B, self.n).copy()
        lam = np.zeros((B, max(self.m, 1)))
        obj, err = np.zeros(B), np.zeros(B)
        status, its = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        self._check(self._L.rpm_sweep_solve(self._h, _dp(x), _dp(lam), _dp(obj), _ip(status), _ip(its), _dp(err)))
        return {"x": x, "lambda": lam[:, :self.m], "obj": obj, "status": status, "iterations": its, "kkt_error": err}

    def solve_warm(self, x0, lam0, z0=None):
        """rpm_sweep_solve_warm: as BatchedIPM.solve(x0, lam0, z0), over all shares."""
        B = self.n_instances
        x = np.ascontiguousarray(x0, dtype=np.float64).reshape(B, self.n).copy()
        lam = np.ascontiguousarray(lam0, dtype=np.float64).reshape(B, self.m).copy()
        obj, err = np.zeros(B), np.zeros(B)
        status, its = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        out = {"x": x, "lambda": lam, "obj": obj, "status": status, "iterations": its, "kkt_error": err}
        zl = zu = None
        if z0 is not None:
            zl, zu = (np.ascontiguousarray(z, dtype=np.float64).reshape(B, self.n).copy() for z in z0)
            out["z_L"], out["z_U"] = zl, zu
        self._check(self._L.rpm_sweep_solve_warm(self._h, _dp(x), _dp(lam), None if zl is None else _dp(zl), None if zu is None else _dp(zu),
                                                 _dp(obj), _ip(status), _ip(its), _dp(err)))
        return out

    def bound_multipliers(self):
        """rpm_sweep_get_bound_multipliers: (z_L, z_U), B x n each, after the last solve."""
        zl, zu = np.zeros((self.n_instances, self.n)), np.zeros((self.n_instances, self.n))
        self._check(self._L.rpm_sweep_get_bound_multipliers(self._h, _dp(zl), _dp(zu)))
        return zl, zu

    def sensitivities(self, var_index, want_lambda=True, _fn=None):
        """rpm_sweep_sensitivities: as BatchedIPM.sensitivities, over all shares."""
        B = self.n_instances
        vi = np.ascontiguousarray(var_index, dtype=np.int32).ravel()
        out = {"dx": np.zeros((B, vi.size, self.n)), "dlambda": np.zeros((B, vi.size, self.m)) if want_lambda else None,
               "delta_w": np.zeros(B), "info": np.zeros(B, dtype=np.int32)}
        self._check((_fn or self._L.rpm_sweep_sensitivities)(self._h, vi.size, _ip(vi), _dp(out["dx"]),
                                                             _dp(out["dlambda"]) if want_lambda else None, _dp(out["delta_w"]), _ip(out["info"])))
        return out

    def constant_sensitivities(self, const_index, want_lambda=True):
        """rpm_sweep_constant_sensitivities: as BatchedIPM.constant_sensitivities, over all shares."""
        return self.sensitivities(const_index, want_lambda, _fn=self._L.rpm_sweep_constant_sensitivities)

    def stats(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._check(self._L.rpm_sweep_get_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"iterations": a.value, "factorizations": b.value, "trial_points": c.value}

    # ---- mesh-error estimate and ph refinement of the whole sweep ------------------------------------------------
    def _sizes_and_shapes(self):
        e0 = self._L.rpm_sweep_engine(self._h, 0)
        kt, rt = C.c_int(), C.c_longlong()
        self._check(self._L.rpm_solution_error_batch_sizes(e0, C.byref(kt), C.byref(rt)))
        return (kt.value, rt.value), _phase_shapes(self._L, e0, self._desc, self.n_phases, self._check)

    def solution_error(self, x, mask=None, full=False):
        """rpm_sweep_solution_error: as NLPEngine.solution_error_batch, over all shares; equal to one engine holding all
        instances bit for bit."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        if x.size != self.n * self.n_instances:
            raise RpmError(RPM_E_INVALID, "x has %d entries, expected %d" % (x.size, self.n * self.n_instances))
        sizes, shapes = self._sizes_and_shapes()
        return _batch_estimate(self._L.rpm_sweep_solution_error, self._check, self._h, x, self.n_instances, sizes, shapes,
                               mask, full)

    def carry_solution(self, to, x):
        """rpm_sweep_carry_solution: the sweep's solutions x (B x n) splined onto the mesh of sweep `to` (same problem, same
        shares) -> (x_to: B x to.n, nonfinite: B ints); equal to one engine holding all instances bit for bit."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        if x.size != self.n * self.n_instances:
            raise RpmError(RPM_E_INVALID, "x has %d entries, expected %d" % (x.size, self.n * self.n_instances))
        out = np.zeros((self.n_instances, to.n))
        flags = np.zeros(self.n_instances, dtype=np.int32)
        self._check(self._L.rpm_sweep_carry_solution(self._h, to._h, _dp(x), _dp(out), _ip(flags)))
        return out, flags

    def carry_multipliers(self, to, x, lam):
        """rpm_sweep_carry_multipliers: the multipliers lam (B x m) of the sweep's solutions x carried onto the mesh of sweep `to`
        -> (lambda_to: B x to.m, nonfinite: B ints); equal to one engine holding all instances bit for bit."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        lam = np.ascontiguousarray(lam, dtype=np.float64).ravel()
        if x.size != self.n * self.n_instances or lam.size != self.m * self.n_instances:
            raise RpmError(RPM_E_INVALID, "x / lambda have %d / %d entries, expected %d / %d" %
                           (x.size, lam.size, self.n * self.n_instances, self.m * self.n_instances))
        out = np.zeros((self.n_instances, to.m))
        flags = np.zeros(self.n_instances, dtype=np.int32)
        self._check(self._L.rpm_sweep_carry_multipliers(self._h, to._h, _dp(x), _dp(lam), _dp(out), _ip(flags)))
        return out, flags

    def shift_plan(self, dt, x, lam=None, z=None):
        """rpm_sweep_shift_plan: as NLPEngine.shift_plan_batch (dt: B x n_phases), over all shares; equal to one engine holding
        all instances bit for bit."""
        return _shift_plan(self._L.rpm_sweep_shift_plan, self._check, self._h, self.n_instances, self.n_phases, self.n, self.m,
                           dt, x, lam, z)

    def sample_plan(self, phase, x, times):
        """rpm_sweep_sample_plan: as NLPEngine.sample_plan_batch, over all shares; equal to one engine holding all instances bit
        for bit."""
        return _sample_plan(self._L.rpm_sweep_sample_plan, self._check, self._h, self._desc, self.n_instances, self.n, phase, x, times)

    def rollout(self, phase, x, dt, n_steps, hold=0, state0=None, t_start=None, traj=False):
        """rpm_sweep_rollout: as NLPEngine.rollout_batch, over all shares; equal to one engine holding all instances bit for bit."""
        return _rollout(self._L.rpm_sweep_rollout, self._check, self._h, self._desc, self.n_instances, self.n, phase, x, dt, n_steps,
                        hold, state0, t_start, traj)

    def set_initial_states(self, phase, state0):
        """rpm_sweep_set_initial_states: the measured initial states of `phase`, B x nx, to every share's solver."""
        s0 = np.ascontiguousarray(state0, dtype=np.float64)
        nx = self._desc.phases[int(phase)].nx if 0 <= int(phase) < self.n_phases else 0
        if nx and s0.size != self.n_instances * nx:
            raise RpmError(RPM_E_INVALID, "state0 has %d entries, expected %d" % (s0.size, self.n_instances * nx))
        self._check(self._L.rpm_sweep_set_initial_states(self._h, int(phase), _dp(s0)))

    def nlp2op(self, x, lam):
        """rpm_sweep_nlp2op: as NLPEngine.nlp2op_batch, over all shares; equal to one engine holding all instances bit for bit."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        if x.size != self.n * self.n_instances:
            raise RpmError(RPM_E_INVALID, "x has %d entries, expected %d" % (x.size, self.n * self.n_instances))
        e0 = self._L.rpm_sweep_engine(self._h, 0)
        return _batch_extract(self._L.rpm_sweep_nlp2op, self._check, self._h, x, lam, self.n_instances, self.m,
                              _extract_layout(self._L, e0, self.n_phases, self._check))

    def ph_refine(self, x, tol, nmin, nmax, mask=None):
        """The sweep's next mesh: per phase (no_more_refine, mesh, nodes, interval_error) from rel_err_max."""
        est = self.solution_error(x, mask)
        e0 = self._L.rpm_sweep_engine(self._h, 0)
        out = []
        for p in range(self.n_phases):
            rel = np.asfortranarray(est["rel_err_max"][p]).ravel(order="F").copy()
            K = self._desc.phases[p].n_intervals
            nk, done, emax = C.c_int(), C.c_int(), np.zeros(K)
            args = (e0, p, _dp(rel), float(tol), int(nmin), int(nmax))
            rc = self._L.rpm_ph_refine_from_error(*args, 0, None, None, C.byref(nk), _dp(emax), C.byref(done))
            mesh, nodes = np.zeros(nk.value + 1), np.zeros(nk.value, dtype=np.int32)
            if rc == RPM_OK:
                rc = self._L.rpm_ph_refine_from_error(*args, nk.value, _dp(mesh), _ip(nodes), C.byref(nk), None, None)
            if rc != RPM_OK:
                raise RpmError(rc, self._L.rpm_last_error(e0).decode())
            out.append((bool(done.value), mesh, nodes, emax))
        return out
