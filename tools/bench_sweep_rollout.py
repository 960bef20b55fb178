"""The plant of the sweep's closed loop: B quadrotor plans (8 intervals x 8 LGR points, per-instance initial states and tracking
targets as in tools/bench_sweep_carry.py, solved once) rolled out and sampled on the device, measured in one process:
  - rpm_rollout_batch_dev over 0.1 s in 4 steps, hold 0, out of place so that every repetition integrates the same 0.1 s (device
    events around enough repetitions to fill a fraction of a second; warm-up first; the median of the timed regions), for every instances-per-workgroup layout
    (option "rollout_tile") and the automatic one; the same with hold 1, with a trajectory and with the verdicts;
  - rpm_sample_plan_batch_dev at 20 times per instance;
  - rpm_rollout_batch through host arrays;
  - the demo's host plant, the only way before: the download of x plus tools/mpc_closed_loop.py's np.interp loop.
Before anything is timed the roll-out is compared with a numpy RK4 of the quadrotor's dynamics under the controls the sampler
returns at the stage times (numpy's sin / cos against the device's: to rounding, not to the bit), 1e-12 * max(1, max|column|).
Writes profiles/sweep_rollout.json (or the path given as second argument) and prints it.
Run on the GPU box:  python tools/bench_sweep_rollout.py [instances] [out.json]"""
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
from lpopc_amd.problem import Options

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "sweep_rollout.json")
DT, STEPS, N_TIMES = 0.1, 4, 20
o = Options()
o.SetStringValue("hessian-approximation", "exact")
rng = np.random.RandomState(5)
prefs = [(1.0 + rng.uniform(-0.2, 0.2), -0.5 + rng.uniform(-0.2, 0.2), 1.5 + rng.uniform(-0.2, 0.2)) for _ in range(B)]
consts = np.stack([np.ascontiguousarray(problems.quadrotor(8, 8, pref=p).GetOpimalProblemFuns().consts, dtype=np.float64) for p in prefs])
prob = problems.quadrotor(8, 8, pref=prefs[0])
eng = NLPEngine(prob, o, n_instances=B, device=0)
eng.set_option("instance_align", 16)
for b in range(1, B):
    eng.set_instance_constants(b, consts[b])
ipm = BatchedIPM(eng)
xl, xu, _, _ = eng.get_bounds_info()
x_start = eng.get_starting_point()[:eng.n]
N1 = 8 * 8 + 1
x0_idx = [i * N1 for i in range(12)]
for b in range(B):
    l, u = xl.copy(), xu.copy()
    l[x0_idx] = u[x0_idx] = np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.1, 0.1, 6)])
    ipm.set_bounds(b, l, u)
d_x = torch.from_numpy(np.tile(x_start, (B, 1))).cuda()
ipm.solve_dev(d_x.clone())                     # warm-up (module load, first touch)
torch.cuda.synchronize()
t0 = time.perf_counter()
r = ipm.solve_dev(d_x)
torch.cuda.synchronize()
solve_s = time.perf_counter() - t0
xs = d_x.cpu().numpy()
state0 = xs[:, x0_idx].copy()


# ---- agreement first: numpy RK4 under the sampler's controls --------------------------------------------------------
def f_quadrotor(y, u, c):
    """csrc/problems/problems.hpp, QuadrotorProblem::dae, over all instances at once (rows)"""
    ph, th, ps, p, q, rr = (y[:, i] for i in range(6, 12))
    F = ((u[:, 0] + u[:, 1]) + u[:, 2]) + u[:, 3]
    tx, ty = c[:, 2] * (u[:, 1] - u[:, 3]), c[:, 2] * (u[:, 2] - u[:, 0])
    tz = c[:, 6] * (((u[:, 0] - u[:, 1]) + u[:, 2]) - u[:, 3])
    sph, cph, sth, cth, sps, cps = np.sin(ph), np.cos(ph), np.sin(th), np.cos(th), np.sin(ps), np.cos(ps)
    Fm = F / c[:, 0]
    w = q * sph + rr * cph
    return np.stack([y[:, 3], y[:, 4], y[:, 5], Fm * (cph * sth * cps + sph * sps), Fm * (cph * sth * sps - sph * cps),
                     Fm * (cph * cth) - c[:, 1], p + w * (sth / cth), q * cph - rr * sph, w / cth,
                     (tx - (c[:, 5] - c[:, 4]) * q * rr) / c[:, 3], (ty - (c[:, 3] - c[:, 5]) * p * rr) / c[:, 4],
                     (tz - (c[:, 4] - c[:, 3]) * p * q) / c[:, 5]], axis=1)


h = np.float64(DT) / STEPS
time_0 = xs[:, -2]                                                     # the first LGR point is -1: time[0] = t0
stage_t = np.stack([time_0 + i * h + off for i in range(STEPS) for off in (0.0, h / 2, h)], axis=1)
ctl = eng.sample_plan_batch(0, xs, stage_t)[0][:, 12:, :]
y = state0.copy()
ref_traj = [y.copy()]
for i in range(STEPS):
    u0_, um, u1 = (ctl[:, :, 3 * i + j] for j in range(3))
    k = f_quadrotor(y, u0_, consts)
    acc = k
    k = f_quadrotor(y + (h / 2) * k, um, consts)
    acc = acc + 2 * k
    k = f_quadrotor(y + (h / 2) * k, um, consts)
    acc = acc + 2 * k
    k = f_quadrotor(y + h * k, u1, consts)
    acc = acc + k
    y = y + (h / 6) * acc
    ref_traj.append(y.copy())
ref_traj = np.stack(ref_traj, axis=1)
got = eng.rollout_batch(0, xs, np.full(B, DT), STEPS, 0, state0, traj=True)
scale = np.maximum(1.0, np.abs(ref_traj).max(axis=1))
worst = float((np.abs(got["traj"] - ref_traj).max(axis=1) / scale).max())
assert worst <= 1e-12 and not got["nonfinite"].any(), "the roll-out differs from the numpy RK4: %g" % worst

# ---- the device-resident calls ----------------------------------------------------------------------------------
d_dt = torch.full((B,), DT, dtype=torch.float64, device="cuda")
d_state0 = torch.from_numpy(state0).cuda()
d_state = d_state0.clone()
d_traj = torch.empty((B, STEPS + 1, 12), dtype=torch.float64, device="cuda")
d_flag = torch.empty(B, dtype=torch.int32, device="cuda")
d_times = torch.from_numpy(np.ascontiguousarray(time_0[:, None] + np.linspace(0.0, 0.2, N_TIMES)[None, :])).cuda()
d_sam = torch.empty((B, 16, N_TIMES), dtype=torch.float64, device="cuda")


def time_dev(call):
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


def loop_call(hold=0):
    # the loop's call, but out of place (the same kernel, the same stores): every repetition integrates the same 0.1 s
    eng.rollout_batch_dev(0, d_x, d_dt, STEPS, d_state, hold, d_state0)


layouts = {}
for tile in (1, 2, 4, 8):
    eng.set_option("rollout_tile", tile)
    s, best, reps = time_dev(loop_call)
    assert np.array_equal(d_state.cpu().numpy(), got["state"])        # the layout changes no bit
    layouts[str(tile)] = {"instances_per_workgroup": tile, "dev_call_s": s, "dev_call_s_min": best, "repetitions": reps}
eng.set_option("rollout_tile", 0)
dev_s, dev_best, reps = time_dev(loop_call)
hold_s = time_dev(lambda: loop_call(1))[0]
full_s = time_dev(lambda: eng.rollout_batch_dev(0, d_x, d_dt, STEPS, d_state, 0, d_state0, None, d_traj, d_flag))[0]
assert np.array_equal(d_traj.cpu().numpy(), got["traj"]) and not d_flag.cpu().numpy().any()
sample_s, sample_best, sample_reps = time_dev(lambda: eng.sample_plan_batch_dev(0, d_x, N_TIMES, d_times, d_sam, d_flag))
sample_noflag_s = time_dev(lambda: eng.sample_plan_batch_dev(0, d_x, N_TIMES, d_times, d_sam))[0]

# ---- host-pointer call and the demo's host plant ----------------------------------------------------------------------
host_s = []
for rep in range(5):
    t0 = time.perf_counter()
    eng.rollout_batch(0, xs, np.full(B, DT), STEPS, 0, state0)
    host_s.append(time.perf_counter() - t0)
tau = np.concatenate([eng.phase_tables(0)["points"], [1.0]])
t_at = (tau + 1.0) * 2.0 / 2.0
plant_s = []
for rep in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    X = d_x.cpu().numpy()
    nxt = np.zeros((B, 12))
    for j in range(12):
        traj = X[:, j * N1:(j + 1) * N1]
        nxt[:, j] = np.array([np.interp(DT, t_at, traj[b]) for b in range(B)])
    plant_s.append(time.perf_counter() - t0)

out = {"workload": "quadrotor MPC sweep, %d instances x (8x8), per-instance initial states and tracking targets, solved once; "
                   "roll-out over %.1f s in %d steps, sample at %d times per instance" % (B, DT, STEPS, N_TIMES),
       "instances": B, "nodes": 64, "sweep_solve_s": solve_s, "converged": int((r["status"] == 0).sum()),
       "rollout_dev_call_s": dev_s, "rollout_dev_call_s_min": dev_best, "rollout_dev_call_repetitions": reps,
       "rollout_dev_call": "hold 0, no trajectory, no verdicts; out of place, so that every repetition integrates the same 0.1 s "
                           "(in place is the same kernel with the same loads and stores)",
       "rollout_hold1_dev_call_s": hold_s, "rollout_with_traj_and_verdicts_dev_call_s": full_s,
       "rollout_layouts_dev_call": layouts,
       "sample_dev_call_s": sample_s, "sample_dev_call_s_min": sample_best, "sample_dev_call_repetitions": sample_reps,
       "sample_dev_call_without_nonfinite_s": sample_noflag_s,
       "rollout_host_pointer_call_s": min(host_s), "rollout_host_pointer_call_s_all": host_s,
       "host_plant_s": min(plant_s), "host_plant_s_all": plant_s,
       "host_plant": "tools/mpc_closed_loop.py before the plant argument: x downloaded, np.interp per instance and state column",
       "device_step_s_for_scale": [3.2e-3, 3.9e-3], "rollout_share_of_device_step": dev_s / 3.2e-3,
       "timing": "5 warm-up calls, then 5 timed regions of `repetitions` calls between device events; medians",
       "worst_difference_to_numpy_rk4": worst, "difference_bound": 1e-12}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
