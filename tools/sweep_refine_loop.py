"""One turn of lpopc's outer loop for a whole sweep, every step batched and on the device: the quadrotor MPC sweep (B instances,
8 intervals x 8 LGR points, per-instance initial states and tracking targets) is solved, its mesh error estimated
(rpm_solution_error_batch), the next mesh decided (ph refinement on the worst instance), the solutions carried onto it
(rpm_carry_solution_batch_dev) and the refined sweep solved from them — next to a cold start of the same refined sweep from
its own starting point (the problem's guess), which is what a refined sweep had to do without the carry, and next to the
primal + dual start: the first mesh's multipliers carried as costates (rpm_carry_multipliers_batch_dev) into rpm_ipm_solve_warm_dev
(z from mu_init, mu_init 1e-6, the warm start's pushes 1e-9).
Records statuses, batched iteration counts and solve times of all three; asserts nothing about them.
Writes profiles/sweep_refine_loop.json (or the path given as second argument) and prints it.
Run on the GPU box:  python tools/sweep_refine_loop.py [instances] [out.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from lpopc_amd import problems
from lpopc_amd.engine import BatchedIPM, NLPEngine
from lpopc_amd.mesh import install_sweep_mesh
from lpopc_amd.problem import Options

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "sweep_refine_loop.json")
o = Options()
o.SetStringValue("hessian-approximation", "exact")
rng = np.random.RandomState(5)
prefs = [(1.0 + rng.uniform(-0.2, 0.2), -0.5 + rng.uniform(-0.2, 0.2), 1.5 + rng.uniform(-0.2, 0.2)) for _ in range(B)]
consts = [np.ascontiguousarray(problems.quadrotor(8, 8, pref=p).GetOpimalProblemFuns().consts, dtype=np.float64) for p in prefs]
x0s = [np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.1, 0.1, 6)]) for _ in range(B)]


WARM = {"mu_init": 1e-6, "warm_start_bound_push": 1e-9, "warm_start_bound_frac": 1e-9, "warm_start_slack_bound_push": 1e-9,
        "warm_start_slack_bound_frac": 1e-9}


def sweep(prob, **solver_options):
    """Engine + solver for `prob`'s mesh with every instance's constants and initial-state bounds applied."""
    eng = NLPEngine(prob, o, n_instances=B, device=0)
    eng.set_option("instance_align", 16)
    for b in range(1, B):
        eng.set_instance_constants(b, consts[b])
    return (eng,) + solver(eng, prob, **solver_options)


def solver(eng, prob, **solver_options):
    """One more solver on `eng`, the instances' initial-state bounds applied -> (solver, the mesh's own starting point)"""
    ipm = BatchedIPM(eng, **solver_options)
    one = NLPEngine(prob, o)
    xl, xu, _, _ = one.get_bounds_info()
    start = one.get_starting_point()
    n1 = one.phase_tables(0)["points"].size + 1
    one.close()
    idx = [i * n1 for i in range(12)]
    for b in range(B):
        l, u = xl.copy(), xu.copy()
        l[idx] = u[idx] = x0s[b]
        ipm.set_bounds(b, l, u)
    return ipm, start


def solve(ipm, d_x, d_lambda=None, warm=False):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = ipm.solve_dev(d_x, d_lambda, warm=warm)
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    status = r["status"]
    return {"solve_s": s, "batched_iterations": ipm.stats()["iterations"], "iterations_max": int(r["iterations"].max()),
            "iterations_mean": float(r["iterations"].mean()),
            "statuses": {BatchedIPM.STATUS[int(k)]: int((status == k).sum()) for k in np.unique(status)},
            "objective_mean": float(np.mean(r["obj"][status == 0])) if (status == 0).any() else None}


# ---- first mesh: solve, estimate, decide ------------------------------------------------------------------------
prob = problems.quadrotor(8, 8, pref=prefs[0])
eng, ipm, start = sweep(prob)
d_start = torch.from_numpy(np.tile(start, (B, 1))).cuda()
ipm.solve_dev(d_start.clone())                 # warm-up (module load, first touch)
d_x = d_start.clone()
d_lam = torch.empty((B, eng.m), dtype=torch.float64, device="cuda")
first = solve(ipm, d_x, d_lam)
xs = d_x.cpu().numpy()
t0 = time.perf_counter()
refined = eng.ph_refine_sweep(xs, 1e-6, 4, 16)
estimate_s = time.perf_counter() - t0

# ---- refined mesh: carry, then warm and cold solves --------------------------------------------------------------
target = problems.quadrotor(8, 8, pref=prefs[0])
no_more = install_sweep_mesh(target, refined)
eng2, ipm2, start2 = sweep(target)
d_warm = torch.empty((B, eng2.n), dtype=torch.float64, device="cuda")
d_flag = torch.empty(B, dtype=torch.int32, device="cuda")
eng.carry_solution_batch_dev(eng2, d_x, d_warm, d_flag)          # the first call on the pair: the launch plan goes up
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
eng.carry_solution_batch_dev(eng2, d_x, d_warm, d_flag)
e1.record()
torch.cuda.synchronize()
carry_s = e0.elapsed_time(e1) * 1e-3
d_lam2 = torch.empty((B, eng2.m), dtype=torch.float64, device="cuda")
d_flag2 = torch.empty(B, dtype=torch.int32, device="cuda")
eng.carry_multipliers_batch_dev(eng2, d_x, d_lam, d_lam2, d_flag2)    # the multipliers' own launch plan goes up
torch.cuda.synchronize()
e0.record()
eng.carry_multipliers_batch_dev(eng2, d_x, d_lam, d_lam2, d_flag2)
e1.record()
torch.cuda.synchronize()
carry_mult_s = e0.elapsed_time(e1) * 1e-3
ipm3, _ = solver(eng2, target, **WARM)
d_cold = torch.from_numpy(np.tile(start2, (B, 1))).cuda()
ipm2.solve_dev(d_cold.clone())                 # warm-up of the refined sweep's kernels, so no timed solve pays for it
d_dual = d_warm.clone()
cold = solve(ipm2, d_cold)
warm = solve(ipm2, d_warm)
dual = solve(ipm3, d_dual, d_lam2, warm=True)

out = {"workload": "quadrotor MPC sweep, %d instances, 8x8 -> the mesh ph_refine(1e-6, 4, 16) asks for" % B, "instances": B,
       "first_mesh": {"nodes_per_interval": [8] * 8, "n": eng.n, **first},
       "estimate_and_decision_s": estimate_s, "no_more_refine": bool(no_more),
       "refined_mesh": {"mesh_points": [float(v) for v in refined[0][1]], "nodes_per_interval": [int(v) for v in refined[0][2]], "n": eng2.n},
       "carry_dev_call_s": carry_s, "carried_nonfinite_instances": int(d_flag.cpu().numpy().sum()),
       "carry_multipliers_dev_call_s": carry_mult_s, "carried_nonfinite_multipliers": int(d_flag2.cpu().numpy().sum()),
       "refined_warm_start": warm, "refined_cold_start": cold, "refined_primal_dual_start": dual,
       "note": "one run; warm = starting points carried from the first mesh's solutions, cold = the problem's own guess on the refined mesh, "
               "primal_dual = the carried starting points and the carried multipliers into the warm solve (z from mu_init)"}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
for name, leg in (("cold", cold), ("primal-only (carried x)", warm), ("primal + dual (carried x, lambda)", dual)):
    print("%-34s batched iterations %3d  mean %.1f  max %d  %.1f ms  %s" % (name, leg["batched_iterations"], leg["iterations_mean"],
                                                                          leg["iterations_max"], 1e3 * leg["solve_s"], leg["statuses"]))
