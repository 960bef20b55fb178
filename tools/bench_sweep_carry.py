"""The fourth step of the sweep's outer loop: B quadrotor solutions (8 intervals x 8 LGR points, per-instance initial states
and tracking targets as in tools/bench_sweep_mesh_error.py) carried onto the mesh the sweep's own ph_refine asks for, measured
in one process:
  - rpm_carry_solution_batch_dev (device events around enough repetitions to fill a fraction of a second; warm-up first;
    the median of the timed regions), for every instances-per-workgroup layout (option "carry_tile") and the automatic one;
  - rpm_carry_solution_batch through host arrays;
  - the one-instance route that was the only way before: one engine, per instance rpm_set_instance_constants(e, 0),
    rpm_nlp2op_control per phase, a new rpm_create carrying the extracted guess, rpm_get_starting_point — timed over a
    subset of the instances and scaled to B (the subset size is recorded);
  - the sweep solve itself, for scale.
The batched result must agree with the one-instance route (1e-12 * max(1, max|column|), t0 / tf to the bit) before anything
is timed.  Writes profiles/sweep_carry.json (or the path given as second argument) and prints it.
Run on the GPU box:  python tools/bench_sweep_carry.py [instances] [out.json]"""
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
from lpopc_amd.engine import BatchedIPM, NLPEngine
from lpopc_amd.mesh import install_guess, install_sweep_mesh
from lpopc_amd.problem import Options

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "sweep_carry.json")
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

# ---- the mesh the sweep asks for, and an engine on it -----------------------------------------------------------
refined = eng.ph_refine_sweep(xs, 1e-6, 4, 16)
target = problems.quadrotor(8, 8, pref=prefs[0])
install_sweep_mesh(target, refined)
to = NLPEngine(target, o, n_instances=B, device=0)
nodes_to = [int(v) for v in refined[0][2]]


def one_instance_route(b, fresh):
    one.set_instance_constants(0, consts[b])
    install_guess(one, fresh, x=xs[b], lam=lam0)
    nxt = NLPEngine(fresh, o)
    x = nxt.get_starting_point()
    nxt.close()
    return x


lam0 = np.zeros(one.m)
fresh = problems.quadrotor(8, 8, pref=prefs[0])
install_sweep_mesh(fresh, refined)

# ---- agreement first --------------------------------------------------------------------------------------------
got, flags = eng.carry_solution_batch(to, xs)            # also the first call on the pair: the launch plan goes up
Nt = sum(nodes_to)
cols = [slice(s * (Nt + 1), (s + 1) * (Nt + 1)) for s in range(12)] + [slice(12 * (Nt + 1) + j * Nt, 12 * (Nt + 1) + (j + 1) * Nt) for j in range(4)]
worst = 0.0
for b in range(SUBSET):
    ref = one_instance_route(b, fresh)
    if flags[b]:
        continue
    assert np.array_equal(got[b, -2:], ref[-2:]), "instance %d: t0 / tf differ from the one-instance route" % b
    for c in cols:
        worst = max(worst, np.abs(got[b, c] - ref[c]).max() / max(1.0, np.abs(ref[c]).max()))
assert worst <= 1e-12, "the batched carry differs from the one-instance route: %g" % worst

# ---- the device-resident call, per layout -----------------------------------------------------------------------
d_out = torch.empty((B, to.n), dtype=torch.float64, device="cuda")
d_flag = torch.empty(B, dtype=torch.int32, device="cuda")


def time_dev():
    call = lambda: eng.carry_solution_batch_dev(to, d_x, d_out, d_flag)     # noqa: E731
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


layouts = {}
for tile in (1, 2, 4, 8):
    eng.set_option("carry_tile", tile)
    s, best, reps = time_dev()
    assert np.array_equal(d_out.cpu().numpy(), got, equal_nan=True)          # the layout changes no bit
    layouts[str(tile)] = {"instances_per_workgroup": tile, "dev_call_s": s, "dev_call_s_min": best, "repetitions": reps,
                          "workgroups_per_tile": eng.get_option("carry_groups")}
eng.set_option("carry_tile", 0)
dev_s, dev_best, reps = time_dev()
assert np.array_equal(d_out.cpu().numpy(), got, equal_nan=True) and np.array_equal(d_flag.cpu().numpy(), flags)
call = lambda: eng.carry_solution_batch_dev(to, d_x, d_out, None)            # noqa: E731
noflag_s = []
for attempt in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    noflag_s.append(e0.elapsed_time(e1) / reps * 1e-3)

# ---- host-pointer call and the one-instance route ---------------------------------------------------------------
host_s = []
for rep in range(5):
    t0 = time.perf_counter()
    eng.carry_solution_batch(to, xs)
    host_s.append(time.perf_counter() - t0)
loop_s = []
for rep in range(2):
    t0 = time.perf_counter()
    for b in range(SUBSET):
        one_instance_route(b, fresh)
    loop_s.append((time.perf_counter() - t0) * B / SUBSET)

out = {"workload": "quadrotor MPC sweep, %d instances x (8x8), per-instance initial states and tracking targets, carried onto "
                   "the mesh ph_refine(1e-6, 4, 16) asks for" % B,
       "instances": B, "source_nodes": 64, "target_nodes_per_interval": nodes_to, "target_nodes": Nt,
       "sweep_solve_s": min(solve_s), "converged": int((r["status"] == 0).sum()), "nonfinite_instances": int(flags.sum()),
       "dev_call_s": dev_s, "dev_call_s_min": dev_best, "dev_call_repetitions": reps, "dev_call_share_of_solve": dev_s / min(solve_s),
       "dev_call_without_nonfinite_s": statistics.median(noflag_s),
       "host_pointer_call_s": min(host_s), "host_pointer_call_s_all": host_s,
       "one_instance_loop_s": min(loop_s), "one_instance_loop_s_all": loop_s, "one_instance_loop_subset": SUBSET,
       "one_instance_loop": "one engine; per instance rpm_set_instance_constants(e, 0) + rpm_nlp2op_control per phase + rpm_create "
                            "with the extracted guess + rpm_get_starting_point; timed over the subset, scaled to all instances",
       "speedup_host_pointer_over_loop": min(loop_s) / min(host_s),
       "layouts_dev_call": layouts, "timing": "5 warm-up calls, then 5 timed regions of `repetitions` calls between device events; medians",
       "worst_difference_to_one_instance_route": worst, "difference_bound": 1e-12}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
