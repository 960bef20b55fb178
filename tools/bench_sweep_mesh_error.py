"""Row f-3 for a sweep: the mesh-error estimate of B quadrotor instances (8 intervals x 8 LGR points, per-instance
initial states as in tools/bench_ipm.py and per-instance tracking targets), measured four ways in one process:
  - rpm_solution_error_batch_dev (device events around enough repetitions to fill a fraction of a second), for every
    instances-per-workgroup layout the kernel offers (option "mesh_err_tile"; 1 = one workgroup per interval and instance);
  - rpm_solution_error_batch through host arrays;
  - the one-instance path: one engine, per instance rpm_set_instance_constants(e, 0, ...) + rpm_solution_error(e, 0, x_b, ...);
  - the sweep solve itself, for scale.
The two paths must agree bit for bit before anything is timed.  Writes profiles/sweep_mesh_error.json (or the path given
as second argument) and prints it.   Run on the GPU box:  python tools/bench_sweep_mesh_error.py [instances] [out.json]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from lpopc_amd import problems
from lpopc_amd.engine import BatchedIPM, NLPEngine, _dp
from lpopc_amd.problem import Options

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "sweep_mesh_error.json")
o = Options()
o.SetStringValue("hessian-approximation", "exact")
rng = np.random.RandomState(5)
prefs = [(1.0 + rng.uniform(-0.2, 0.2), -0.5 + rng.uniform(-0.2, 0.2), 1.5 + rng.uniform(-0.2, 0.2)) for _ in range(B)]
consts = [np.ascontiguousarray(problems.quadrotor(8, 8, pref=p).GetOpimalProblemFuns().consts, dtype=np.float64) for p in prefs]
prob = problems.quadrotor(8, 8, pref=prefs[0])
eng = NLPEngine(prob, o, n_instances=B, device=0)
eng.set_option("instance_align", 16)
for b in range(1, B):
    eng.set_instance_constants(b, consts[b])
ipm = BatchedIPM(eng)
one = NLPEngine(prob, o, device=0)
xl, xu, _, _ = one.get_bounds_info()
x_start = one.get_starting_point()
N1 = 8 * 8 + 1
x0_idx = [i * N1 for i in range(12)]
for b in range(B):
    l, u = xl.copy(), xu.copy()
    l[x0_idx] = u[x0_idx] = np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.1, 0.1, 6)])
    ipm.set_bounds(b, l, u)
d_start = torch.from_numpy(np.tile(x_start, (B, 1))).cuda()

# ---- the sweep solve, for scale ---------------------------------------------------------------------------------
r = ipm.solve_dev(d_start.clone())            # warm-up (module load, first touch)
torch.cuda.synchronize()
solve_s = []
for rep in range(3):
    d_x = d_start.clone()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = ipm.solve_dev(d_x)
    torch.cuda.synchronize()
    solve_s.append(time.perf_counter() - t0)
xs = d_x.cpu().numpy()

# ---- agreement first --------------------------------------------------------------------------------------------
KT, RT = eng.solution_error_batch_sizes()
est = eng.solution_error_batch(xs, full=True)          # also the first call: tables up, workspace allocated
rel_one = np.zeros(RT)
rows = C.c_int()
L = one._L


def per_instance_loop(check):
    for b in range(B):
        rc = L.rpm_set_instance_constants(one._h, 0, _dp(consts[b]), consts[b].size)
        rc = rc or L.rpm_solution_error(one._h, 0, _dp(xs[b]), _dp(rel_one), C.byref(rows))
        if rc:
            raise RuntimeError(one.last_error())
        if check and not np.array_equal(rel_one.reshape(12, rows.value).T, est["rel_err"][0][b], equal_nan=True):
            raise AssertionError("instance %d: the batched estimate differs from the one-instance path" % b)


per_instance_loop(True)

# ---- the device-resident call, per layout -----------------------------------------------------------------------
f64 = dict(dtype=torch.float64, device="cuda")
d_iv, d_max, d_flag = torch.empty((B, KT), **f64), torch.empty(RT, **f64), torch.empty(B, dtype=torch.int32, device="cuda")


def time_dev():
    call = lambda: eng.solution_error_batch_dev(d_x, None, d_iv, d_max, None, d_flag)     # noqa: E731
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    reps, best = 20, None
    for attempt in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms < 200.0 and attempt == 0:              # fill about a quarter of a second
            reps = int(reps * 250.0 / max(ms, 1e-3)) + 1
            continue
        best = ms / reps if best is None else min(best, ms / reps)
    return best * 1e-3, reps


layouts = {}
ref_iv = None
for tile in (1, 2, 4, 8, 16):
    eng.set_option("mesh_err_tile", tile)
    s, reps = time_dev()
    iv = d_iv.cpu().numpy()
    assert ref_iv is None or np.array_equal(iv, ref_iv, equal_nan=True)     # the layout changes no bit
    ref_iv = iv
    layouts[str(tile)] = {"instances_per_workgroup": tile, "dev_call_s": s, "repetitions": reps}
eng.set_option("mesh_err_tile", 0)
dev_s, reps = time_dev()
assert np.array_equal(ref_iv, np.concatenate(est["interval_error"], axis=1), equal_nan=True)
assert np.array_equal(d_max.cpu().numpy().reshape(12, -1).T, np.maximum.reduce(est["rel_err"][0], axis=0), equal_nan=True)

# ---- host-pointer call and the one-instance loop ----------------------------------------------------------------
host_s = []
for rep in range(5):
    t0 = time.perf_counter()
    eng.solution_error_batch(xs)
    host_s.append(time.perf_counter() - t0)
loop_s = []
for rep in range(2):
    t0 = time.perf_counter()
    per_instance_loop(False)
    loop_s.append(time.perf_counter() - t0)

out = {"workload": "quadrotor MPC sweep, %d instances x (8x8), per-instance initial states and tracking targets" % B,
       "instances": B, "n_intervals_total": KT, "rel_doubles_per_instance": RT,
       "sweep_solve_s": min(solve_s), "converged": int((r["status"] == 0).sum()),
       "nonfinite_instances": int(est["nonfinite"].sum()),
       "dev_call_s": dev_s, "dev_call_repetitions": reps, "dev_call_share_of_solve": dev_s / min(solve_s),
       "dev_call_outputs": "interval_error, rel_err_max, nonfinite",
       "host_pointer_call_s": min(host_s), "host_pointer_call_s_all": host_s,
       "host_pointer_call_outputs": "interval_error, rel_err_max, nonfinite",
       "one_instance_loop_s": min(loop_s), "one_instance_loop_s_all": loop_s,
       "one_instance_loop": "one engine; per instance rpm_set_instance_constants(e, 0) + rpm_solution_error(e, 0, x_b)",
       "speedup_host_pointer_over_loop": min(loop_s) / min(host_s),
       "layouts_dev_call": layouts, "layout_kept": "automatic: 8 instances per workgroup, the interval's tables staged in LDS",
       "bit_identical_to_one_instance_path": True}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
