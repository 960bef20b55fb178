"""Receding-horizon demo of row f-2: B quadrotors fly to their own targets; every control period all B optimal-control
problems (8 x 8 LGR, horizon 2 s) are re-solved on the device from the measured states, warm-started from the previous
solutions (iterates stay in HBM: solve_dev in/out), and the first part of each plan is applied to a simple simulation
of the same dynamics.  Every step is solved three ways from the same measured states: cold from the problem's guess, primal-only
warm (the previous solution shifted, small mu_init, no push: the leg that drives the simulation) and primal + dual warm
(rpm_ipm_solve_warm_dev: its own previous solution shifted, with that solve's lambda and bound multipliers).  Prints per-step solve
time and iteration counts of all three.
A fourth leg keeps the whole step on the device: the measured states (B x 12 doubles, the only upload) go into the solver's bounds
with set_initial_states_dev, the warm solve, bound_multipliers_dev, then shift_plan_batch_dev moves x, lambda, z_L and z_U on by dt
into a second set of buffers, and the plan's next initial state is read from the shifted plan on the device.  Its whole step, from
bounds in to shifted plan out, is printed beside the primal + dual leg's, which is timed the same way with its set_all_bounds, its
download, its np.interp shift and its upload; that leg shifts the states only and leaves lambda and z where they were.  A fifth leg
is the fourth with everything around the solve replayed from two captured graphs (the bounds before it; multipliers, shift and
the copy back into fixed buffers after it): the solve itself reads three counters per iteration on the host and cannot be captured.
python tools/mpc_closed_loop.py [instances] [steps] [trace] [plant]
"trace": where the slowest primal + dual instance of a step needs more iterations than the slowest primal-only one, its accepted
steps are printed (f, theta, mu, alpha, alpha_z, delta_w, E_0, backtracks).
"plant": the next measured state comes from the true dynamics instead of the planned trajectory: rollout_batch_dev integrates every
instance's own dae under the primal-only leg's plan over dt = 0.1 in 4 Runge-Kutta steps (hold 0), the state updated in place on the
device and handed to the fourth leg's set_initial_states_dev without leaving it; the other legs get its download."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lpopc_amd import problems
from lpopc_amd.engine import BatchedIPM, NLPEngine
from lpopc_amd.problem import Options

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
want_trace = "trace" in sys.argv[3:]
want_plant = "plant" in sys.argv[3:]
K, NK = 8, 8
o = Options()
o.SetStringValue("hessian-approximation", "exact")
rng = np.random.RandomState(2)
targets = rng.uniform(-1.5, 1.5, size=(B, 3))
base = problems.quadrotor(K, NK)
eng = NLPEngine(base, o, n_instances=B, device=0)
for b in range(B):
    eng.set_instance_constants(b, problems.quadrotor(K, NK, pref=tuple(targets[b])).GetOpimalProblemFuns().consts)
ipm = BatchedIPM(eng, tol=1e-6)
cold_ipm, dual_ipm = BatchedIPM(eng, tol=1e-6), BatchedIPM(eng, tol=1e-6)
dev_ipm, graph_ipm = BatchedIPM(eng, tol=1e-6), BatchedIPM(eng, tol=1e-6)
if want_trace:
    dual_ipm.set_option("trace", 64)
one = NLPEngine(base, o, device=0)
xl, xu, _, _ = one.get_bounds_info()
x_guess = one.get_starting_point()
N1 = K * NK + 1
x0_idx = np.array([i * N1 for i in range(12)])
tau = np.concatenate([one.phase_tables(0)["points"], [1.0]])          # LGR points + the end point, in [-1, 1]
horizon = 2.0
dt = 0.1
state = np.zeros((B, 12))
state[:, :3] = rng.uniform(-0.3, 0.3, size=(B, 3))
XL, XU = np.tile(xl, (B, 1)), np.tile(xu, (B, 1))
d_guess = torch.from_numpy(np.tile(x_guess, (B, 1))).cuda()
d_x, d_x3 = d_guess.clone(), d_guess.clone()
d_lam3 = torch.zeros((B, eng.m), dtype=torch.float64, device="cuda")
d_zl3, d_zu3 = (torch.zeros((B, eng.n), dtype=torch.float64, device="cuda") for _ in range(2))
t_at = (tau + 1.0) * horizon / 2.0


def plan_buffers():
    return [d_guess.clone(), torch.zeros((B, eng.m), dtype=torch.float64, device="cuda"),
            torch.zeros((B, eng.n), dtype=torch.float64, device="cuda"), torch.zeros((B, eng.n), dtype=torch.float64, device="cuda")]


cur4, nxt4, cur5, nxt5 = plan_buffers(), plan_buffers(), plan_buffers(), plan_buffers()
d_dt = torch.full((B, 1), dt, dtype=torch.float64, device="cuda")
d_state4, d_state5 = (torch.zeros((B, 12), dtype=torch.float64, device="cuda") for _ in range(2))
d_x0_idx = torch.from_numpy(x0_idx).cuda()
d_plant = torch.from_numpy(state).cuda()              # "plant": the measured states, resident on the device
graphs = {}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, 1e3 * (time.perf_counter() - t0)


def shifted(X):
    """the plan moved on by dt: the next problem starts where this one is after dt; the rest is kept as the guess"""
    for j in range(12):
        traj = X[:, j * N1:(j + 1) * N1]
        X[:, j * N1:(j + 1) * N1] = np.stack([np.interp(np.minimum(t_at + dt, horizon), t_at, traj[b]) for b in range(B)])
    return torch.from_numpy(X)


def warm_options(solver):
    solver.set_option("mu_init", 1e-4)
    for k in ("warm_start_bound_push", "warm_start_bound_frac", "warm_start_slack_bound_push", "warm_start_slack_bound_frac"):
        solver.set_option(k, 1e-6)
    solver.set_option("warm_start_mult_bound_push", 1e-8)


def solve_plan(solver, plan, warm):
    t0 = time.perf_counter()
    if warm:
        r = solver.solve_dev(plan[0], plan[1], d_z_L=plan[2], d_z_U=plan[3], warm=True)
    else:                                             # no duals yet: a cold solve that keeps them
        r = solver.solve_dev(plan[0], plan[1])
    r["solve_ms"] = 1e3 * (time.perf_counter() - t0)
    return r


def device_step(warm):
    """the fourth leg: measured states in, shifted plan out, the next initial state read from it"""
    if want_plant:                                    # the roll-out left them on the device
        dev_ipm.set_initial_states_dev(0, d_plant)
    else:
        d_state4.copy_(torch.from_numpy(state))
        dev_ipm.set_initial_states_dev(0, d_state4)
    r = solve_plan(dev_ipm, cur4, warm)
    dev_ipm.bound_multipliers_dev(cur4[2], cur4[3])
    eng.shift_plan_batch_dev(d_dt, cur4[0], nxt4[0], cur4[1], nxt4[1], cur4[2], cur4[3], nxt4[2], nxt4[3])
    r["next_state"] = nxt4[0].index_select(1, d_x0_idx)
    return r


def after_solve5():
    graph_ipm.bound_multipliers_dev(cur5[2], cur5[3])
    eng.shift_plan_batch_dev(d_dt, cur5[0], nxt5[0], cur5[1], nxt5[1], cur5[2], cur5[3], nxt5[2], nxt5[3])
    for a, b_ in zip(cur5, nxt5):                     # fixed buffers: a graph replays the addresses it was captured with
        a.copy_(b_)


def graph_step(warm):
    """the fifth leg: the fourth's step with the launches around the solve replayed from captured graphs"""
    d_state5.copy_(torch.from_numpy(state))
    if graphs:
        graphs["before"].replay()
    else:
        graph_ipm.set_initial_states_dev(0, d_state5)
    r = solve_plan(graph_ipm, cur5, warm)
    if graphs:
        graphs["after"].replay()
        return r
    after_solve5()                                    # the first step runs directly (the launch plans go up), then is captured
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graphs["before"], graphs["after"] = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graphs["before"], stream=side):
        graph_ipm.set_initial_states_dev(0, d_state5)
    with torch.cuda.graph(graphs["after"], stream=side):
        after_solve5()
    return r


def host_step(warm):
    """the primal + dual leg timed like the fourth: bounds up, solve, plan down, np.interp shift of the states, plan up"""
    dual_ipm.set_all_bounds(XL, XU)
    r = solve_plan(dual_ipm, [d_x3, d_lam3, d_zl3, d_zu3], warm)
    if not warm:
        dual_ipm.bound_multipliers_dev(d_zl3, d_zu3)
    d_x3.copy_(shifted(d_x3.cpu().numpy()))
    return r


def leg(name, r, ms):
    return "%s %7.1f ms  it %d..%d  ok %d/%d" % (name, ms, r["iterations"].min(), r["iterations"].max(), int((r["status"] <= 1).sum()), B)


for step in range(steps):
    XL[:, x0_idx] = XU[:, x0_idx] = state
    for s_ in (ipm, cold_ipm):
        s_.set_all_bounds(XL, XU)
    if step == 1:                                     # warm starts: small barrier, do not push the previous solution away
        ipm.set_option("mu_init", 1e-4)
        ipm.set_option("bound_push", 1e-6)
        ipm.set_option("bound_frac", 1e-6)
        for s_ in (dual_ipm, dev_ipm, graph_ipm):
            warm_options(s_)
    d_c = d_guess.clone()
    rc, ms_c = timed(lambda: cold_ipm.solve_dev(d_c))
    r, ms = timed(lambda: ipm.solve_dev(d_x))
    r3, step3 = timed(lambda: host_step(step > 0))
    ms3 = r3["solve_ms"]
    r4, step4 = timed(lambda: device_step(step > 0))
    r5, step5 = timed(lambda: graph_step(step > 0))
    X = d_x.cpu().numpy()
    if want_plant:
        # the plant: every instance's own dynamics under the plan's control for dt, from the measured state, in place
        eng.rollout_batch_dev(0, d_x, d_dt, 4, d_plant, 0, d_plant)
        state = d_plant.cpu().numpy()
    else:
        # "plant": follow the planned state trajectory for dt (the plan is dynamically consistent to the mesh accuracy)
        for j in range(12):
            traj = X[:, j * N1:(j + 1) * N1]
            state[:, j] = np.array([np.interp(dt, t_at, traj[b]) for b in range(B)])
    dist = np.linalg.norm(state[:, :3] - targets, axis=1)
    print("step %2d  %d solves  %s | %s | %s | mean distance to target %.3f" % (
        step, B, leg("cold", rc, ms_c), leg("primal-only", r, ms), leg("primal + dual", r3, ms3), dist.mean()), flush=True)
    if want_trace and r3["iterations"].max() > r["iterations"].max():
        worst = int(np.argmax(r3["iterations"]))
        print("  instance %d: primal + dual %d iterations, primal-only %d; its accepted steps:" % (worst, r3["iterations"][worst], r["iterations"][worst]))
        for row in dual_ipm.trace(worst, 64):
            print("   f %.9g  theta %.3e  mu %.3e  alpha %.3e  alpha_z %.3e  delta_w %.3e  E_0 %.3e  backtracks %d" % (tuple(row[:7]) + (int(row[7]),)))
    print("         whole step, bounds in to shifted plan out: primal + dual (host shift, set_all_bounds) %7.1f ms | on the device %7.1f ms"
          " (solve %.1f ms, it %d..%d, ok %d/%d) | with graphs %7.1f ms (it %d..%d) | next state, device plan against the plant: mean |diff| %.2e" % (
              step3, step4, r4["solve_ms"], r4["iterations"].min(), r4["iterations"].max(), int((r4["status"] <= 1).sum()), B,
              step5, r5["iterations"].min(), r5["iterations"].max(), np.abs(r4["next_state"].cpu().numpy() - state).mean()), flush=True)
    d_x.copy_(shifted(X))
    cur4, nxt4 = nxt4, cur4
