"""The last step of a sweep: B quadrotor solutions (8 intervals x 8 LGR points, per-instance initial states and tracking
targets as in tools/bench_sweep_carry.py) turned into time / state / control / costate / Hamiltonian / costs, measured in one
process:
  - rpm_nlp2op_batch_dev (device events around enough repetitions to fill a fraction of a second; warm-up first; the median
    of the timed regions), for every instances-per-workgroup layout (option "extract_tile") and the automatic one;
  - rpm_nlp2op_batch through host arrays;
  - the one-instance route that was the only way before: one engine, per instance rpm_set_instance_constants(e, 0) and
    rpm_nlp2op_control per phase — timed over a subset of the instances and scaled to B (the subset size is recorded);
  - the sweep solve itself, for scale.
The batched result must equal the one-instance route bit for bit on the subset before anything is timed.  Writes
profiles/sweep_extract.json (or the path given as second argument) and prints it.
Run on the GPU box:  python tools/bench_sweep_extract.py [instances] [out.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from lpopc_amd import problems
from lpopc_amd.engine import EXTRACT_FIELDS, BatchedIPM, NLPEngine
from lpopc_amd.problem import Options

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "sweep_extract.json")
SUBSET = min(B, 64)
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
d_lam = torch.zeros((B, eng.m), dtype=torch.float64, device="cuda")

# ---- the sweep solve, for scale ---------------------------------------------------------------------------------
r = ipm.solve_dev(d_start.clone(), d_lam)     # warm-up (module load, first touch)
torch.cuda.synchronize()
solve_s = []
for rep in range(3):
    d_x = d_start.clone()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = ipm.solve_dev(d_x, d_lam)
    torch.cuda.synchronize()
    solve_s.append(time.perf_counter() - t0)
xs, lams = d_x.cpu().numpy(), d_lam.cpu().numpy()


def one_instance_route(b):
    one.set_instance_constants(0, consts[b])
    return one.nlp2op_control(0, x=xs[b], lam=lams[b])


# ---- agreement first: bit for bit -------------------------------------------------------------------------------
got, flags = eng.nlp2op_batch(xs, lams)                  # also the first call on the engine: the launch plan is made
for b in range(SUBSET):
    ref = one_instance_route(b)
    for k in EXTRACT_FIELDS:
        assert np.array_equal(got[0][k][b], ref[k], equal_nan=True), "instance %d: %s differs from the one-instance route" % (b, k)

# ---- the device-resident call, per layout -----------------------------------------------------------------------
_, EB = eng.nlp2op_batch_layout()
d_out = torch.empty((B, EB), dtype=torch.float64, device="cuda")
d_flag = torch.empty(B, dtype=torch.int32, device="cuda")


def time_dev(flag):
    call = lambda: eng.nlp2op_batch_dev(d_x, d_lam, d_out, flag)     # noqa: E731
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    reps, times = 20, []
    for attempt in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms < 100.0 and attempt == 0:              # fill about a fifth of a second
            reps = int(reps * 200.0 / max(ms, 1e-3)) + 1
            continue
        times.append(ms / reps)
    return statistics.median(times) * 1e-3, min(times) * 1e-3, reps


eng.set_option("extract_tile", 0)
first = d_out.clone()
eng.nlp2op_batch_dev(d_x, d_lam, first, d_flag)
torch.cuda.synchronize()
first = first.cpu().numpy()
layouts = {}
for tile in (1, 2, 4, 8):
    eng.set_option("extract_tile", tile)
    s, best, reps = time_dev(d_flag)
    assert np.array_equal(d_out.cpu().numpy(), first, equal_nan=True)          # the layout changes no bit
    layouts[str(tile)] = {"instances_per_workgroup": tile, "dev_call_s": s, "dev_call_s_min": best, "repetitions": reps}
eng.set_option("extract_tile", 0)
dev_s, dev_best, reps = time_dev(d_flag)
assert np.array_equal(d_out.cpu().numpy(), first, equal_nan=True) and np.array_equal(d_flag.cpu().numpy(), flags)
noflag_s, _, _ = time_dev(None)

# ---- host-pointer call and the one-instance route ---------------------------------------------------------------
host_s = []
for rep in range(5):
    t0 = time.perf_counter()
    eng.nlp2op_batch(xs, lams)
    host_s.append(time.perf_counter() - t0)
raw_s = []                                               # the C call alone, without the wrapper's slicing into fields
import ctypes as C
h_out, h_flag = np.zeros((B, EB)), np.zeros(B, dtype=np.int32)
dp = C.POINTER(C.c_double)
for rep in range(5):
    t0 = time.perf_counter()
    rc = eng._L.rpm_nlp2op_batch(eng._h, xs.ctypes.data_as(dp), lams.ctypes.data_as(dp), h_out.ctypes.data_as(dp),
                                 h_flag.ctypes.data_as(C.POINTER(C.c_int)))
    raw_s.append(time.perf_counter() - t0)
    assert rc == 0
assert np.array_equal(h_out, first, equal_nan=True)
loop_s = []
for rep in range(3):
    t0 = time.perf_counter()
    for b in range(SUBSET):
        one_instance_route(b)
    loop_s.append((time.perf_counter() - t0) * B / SUBSET)

best_tile = min(layouts, key=lambda k: layouts[k]["dev_call_s"])
out = {"workload": "quadrotor MPC sweep, %d instances x (8x8), per-instance initial states and tracking targets: the solutions "
                   "and multipliers of the sweep solve extracted (time, state, control, costate, pathmult, Hamiltonian, costs)" % B,
       "instances": B, "nodes": 64, "block_doubles": EB, "output_bytes": B * EB * 8,
       "sweep_solve_s": min(solve_s), "converged": int((r["status"] == 0).sum()), "nonfinite_instances": int(flags.sum()),
       "dev_call_s": dev_s, "dev_call_s_min": dev_best, "dev_call_repetitions": reps, "dev_call_share_of_solve": dev_s / min(solve_s),
       "dev_call_without_nonfinite_s": noflag_s,
       "host_pointer_call_s": min(raw_s), "host_pointer_call_s_all": raw_s,
       "python_wrapper_call_s": min(host_s), "python_wrapper_call_s_all": host_s,
       "one_instance_loop_s": min(loop_s), "one_instance_loop_s_all": loop_s, "one_instance_loop_subset": SUBSET,
       "one_instance_loop": "one engine; per instance rpm_set_instance_constants(e, 0) + rpm_nlp2op_control per phase; timed over the "
                            "subset, scaled to all instances",
       "speedup_dev_call_over_loop": min(loop_s) / dev_s, "speedup_host_pointer_over_loop": min(loop_s) / min(raw_s),
       "layouts_dev_call": layouts, "fastest_layout": int(best_tile),
       "timing": "5 warm-up calls, then 5 timed regions of `repetitions` calls between device events; medians",
       "agreement": "every field of the first %d instances equal to the one-instance route bit for bit; every layout and both forms "
                    "equal to each other bit for bit" % SUBSET}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
