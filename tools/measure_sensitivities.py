"""Row f-2 measurement: what the solution sensitivities (rpm_ipm_sensitivities_dev) and the predictor (rpm_ipm_apply_sensitivities_dev)
cost and what they buy, each number beside the parent's path in the same run.  Prints one JSON object per part:
  (a) the 1024-instance quadrotor sweep (8 x 8) solved, then dx / d(initial states) of all instances: time of the call against the
      time of one iteration of the solve (wall / batched iterations; factorisation and substitution per launch from HIP events)
  (b) the predictor's launch on those arrays: device time against the bytes it moves
  (c) the receding-horizon step at 256 instances, measured states that differ from the predicted ones: iterations and wall time of
      measured states + warm solve + bound multipliers + shift from the shifted plan ("plain"), and with the advanced step — solve
      for the predicted state and take its sensitivities while the plant moves ("background"), then predictor + the same step
      ("foreground")
  (d) on the sweep of (a): the sensitivities to the three target constants and the mass (rpm_ipm_constant_sensitivities_dev) beside
      those to the 12 initial states, and every instance's constants in one upload against one call per instance
  (e) a receding-horizon step at 256 instances whose targets move by up to 0.05 per axis: new constants + warm solve from the old
      plan ("plain"), and with the predictor x + S delta in between ("predictor"; its sensitivities are taken in the background)
Run on the GPU box:  python tools/measure_sensitivities.py [instances (a, b, d)] [instances (c, e)] [steps (c, e)] [parts, e.g. de]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lpopc_amd import problems
from lpopc_amd.engine import BatchedIPM, NLPEngine
from lpopc_amd.problem import Options

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
B_C = int(sys.argv[2]) if len(sys.argv) > 2 else 256
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 8
PARTS = sys.argv[4] if len(sys.argv) > 4 else "abcde"
K, NK = 8, 8
CONSTS = np.array([7, 8, 9, 0], dtype=np.int32)      # quadrotor: the target position, the mass
N1 = K * NK + 1
X0_IDX = np.array([i * N1 for i in range(12)])
o = Options()
o.SetStringValue("hessian-approximation", "exact")


def timed(fn, reps=3):
    best, r = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return r, 1e3 * best


def part_a_b():
    prob = problems.quadrotor(K, NK)
    eng = NLPEngine(prob, o, n_instances=B, device=0)
    eng.set_option("instance_align", 16)
    ipm = BatchedIPM(eng)
    xl, xu, _, _ = eng.get_bounds_info()
    rng = np.random.RandomState(5)
    XL, XU = np.tile(xl, (B, 1)), np.tile(xu, (B, 1))
    XL[:, X0_IDX] = XU[:, X0_IDX] = np.concatenate([rng.uniform(-0.5, 0.5, (B, 3)), rng.uniform(-0.3, 0.3, (B, 3)), rng.uniform(-0.1, 0.1, (B, 6))], axis=1)
    ipm.set_all_bounds(XL, XU)
    params = ipm.initial_state_variables(0)
    assert np.array_equal(params, X0_IDX)
    n, m, P = eng.n, eng.m, len(params)
    d_x0 = torch.from_numpy(np.tile(eng.get_starting_point()[:n], (B, 1))).cuda()
    d_x, d_lam = d_x0.clone(), torch.zeros((B, m), dtype=torch.float64, device="cuda")
    ipm.solve_dev(d_x0.clone())                                    # warm-up
    r, solve_ms = timed(lambda: (d_x.copy_(d_x0), ipm.solve_dev(d_x, d_lam))[1])
    st, kt = ipm.stats(), ipm.kernel_times()
    d_dx = torch.empty((B, P, n), dtype=torch.float64, device="cuda")
    d_dl = torch.empty((B, P, m), dtype=torch.float64, device="cuda")
    ipm.sensitivities_dev(params, d_dx, d_dl)                      # warm-up: table, work space
    s, sens_ms = timed(lambda: ipm.sensitivities_dev(params, d_dx, d_dl))
    _, sens_x_ms = timed(lambda: ipm.sensitivities_dev(params, d_dx))
    print(json.dumps({"part": "a", "instances": B, "n": n, "m": m, "parameters": P, "converged": int((r["status"] == 0).sum()),
                      "solve_ms": solve_ms, "batched_iterations": st["iterations"], "ms_per_iteration": solve_ms / max(1, st["iterations"]),
                      "factor_ms_per_launch": kt["factor_ms"] / max(1, st["factorizations"]),
                      "substitution_ms_per_launch": kt["substitution_ms"] / max(1, st["iterations"]),
                      "sensitivities_ms": sens_ms, "sensitivities_without_dlambda_ms": sens_x_ms,
                      "sensitivities_in_iterations": sens_ms / (solve_ms / max(1, st["iterations"])),
                      "info_counts": np.bincount(s["info"], minlength=3).tolist(), "delta_w_max": float(np.nanmax(s["delta_w"]))}))
    # (b) the predictor
    d_delta = torch.from_numpy(np.random.RandomState(3).uniform(-0.05, 0.05, (B, P))).cuda()
    d_xo, d_lo = torch.empty_like(d_x), torch.empty_like(d_lam)
    ipm.apply_sensitivities_dev(params, d_dx, d_delta, d_x, d_xo, d_dl, d_lam, d_lo)
    reps = 20
    for with_lambda in (True, False):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        torch.cuda.synchronize()
        ev[0].record()
        for i in range(reps):
            if with_lambda:
                ipm.apply_sensitivities_dev(params, d_dx, d_delta, d_x, d_xo, d_dl, d_lam, d_lo)
            else:
                ipm.apply_sensitivities_dev(params, d_dx, d_delta, d_x, d_xo)
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))
        nbytes = 8 * B * ((P + 2) * n + P + ((P + 2) * m if with_lambda else 0))
        print(json.dumps({"part": "b", "with_lambda": with_lambda, "bytes": nbytes, "median_us": 1e3 * ms[reps // 2], "min_us": 1e3 * ms[0],
                          "GBs_at_median": nbytes / (ms[reps // 2] * 1e-3) / 1e9,
                          "note": "back-to-back launches on arrays of %.0f MB: re-reads may be served by the Infinity Cache" % (nbytes / 1e6)}))
    if "d" in PARTS:
        part_d(eng, ipm, sens_ms, solve_ms / max(1, st["iterations"]))
    ipm.close()
    eng.close()


def part_d(eng, ipm, sens_ms, iteration_ms):
    n, m, Pc = eng.n, eng.m, len(CONSTS)
    d_dx = torch.empty((B, Pc, n), dtype=torch.float64, device="cuda")
    d_dl = torch.empty((B, Pc, m), dtype=torch.float64, device="cuda")
    ipm.constant_sensitivities_dev(CONSTS, d_dx, d_dl)             # warm-up: table, scratch, work space
    s, const_ms = timed(lambda: ipm.constant_sensitivities_dev(CONSTS, d_dx, d_dl))
    _, one_ms = timed(lambda: ipm.constant_sensitivities_dev(CONSTS[:1], d_dx, d_dl))
    consts = np.tile(np.array(problems.quadrotor(K, NK).GetOpimalProblemFuns().consts), (B, 1))
    _, all_ms = timed(lambda: eng.set_all_instance_constants(consts))
    _, loop_ms = timed(lambda: [eng.set_instance_constants(b, consts[b]) for b in range(B)], reps=1)
    print(json.dumps({"part": "d", "instances": B, "constants": Pc, "constant_sensitivities_ms": const_ms,
                      "constant_sensitivities_one_constant_ms": one_ms, "sensitivities_12_states_ms": sens_ms,
                      "constant_sensitivities_in_iterations": const_ms / iteration_ms,
                      "info_counts": np.bincount(s["info"], minlength=3).tolist(),
                      "set_all_instance_constants_ms": all_ms, "set_instance_constants_loop_ms": loop_ms}))


def part_e():
    Bc = B_C
    rng = np.random.RandomState(2)
    targets = rng.uniform(-1.5, 1.5, size=(Bc, 3))
    consts = np.tile(np.array(problems.quadrotor(K, NK).GetOpimalProblemFuns().consts), (Bc, 1))
    consts[:, 7:10] = targets
    eng = NLPEngine(problems.quadrotor(K, NK), o, n_instances=Bc, device=0)
    n, m = eng.n, eng.m
    ks = CONSTS[:3]
    xl, xu, _, _ = eng.get_bounds_info()
    XL, XU = np.tile(xl, (Bc, 1)), np.tile(xu, (Bc, 1))
    XL[:, X0_IDX[:3]] = XU[:, X0_IDX[:3]] = rng.uniform(-0.3, 0.3, size=(Bc, 3))
    x0 = np.tile(eng.get_starting_point()[:n], (Bc, 1))
    moves = np.random.RandomState(11).uniform(-0.05, 0.05, size=(STEPS, Bc, 3))
    for leg in ("plain", "predictor"):
        s = BatchedIPM(eng, tol=1e-6)
        s.set_all_bounds(XL, XU)
        c = consts.copy()
        eng.set_all_instance_constants(c)
        sol = s.solve(x0)
        z = s.bound_multipliers()
        s.set_option("mu_init", 1e-4)
        for k in ("warm_start_bound_push", "warm_start_bound_frac", "warm_start_slack_bound_push", "warm_start_slack_bound_frac"):
            s.set_option(k, 1e-6)
        s.set_option("warm_start_mult_bound_push", 1e-8)
        rows = []
        for step in range(STEPS):
            row = {}
            x, lam = sol["x"], sol["lambda"]
            if leg == "predictor":
                t0 = time.perf_counter()
                sens = s.constant_sensitivities(ks)
                row["background_ms"] = 1e3 * (time.perf_counter() - t0)
                row["left_out"] = int((sens["info"] == 2).sum())
            t0 = time.perf_counter()
            c[:, 7:10] += moves[step]
            eng.set_all_instance_constants(c)
            if leg == "predictor":
                x, lam = s.apply_constant_sensitivities(ks, sens["dx"], moves[step], x, sens["dlambda"], lam)
            sol_new = s.solve(x, lam, z)
            z = s.bound_multipliers()
            row.update(foreground_ms=1e3 * (time.perf_counter() - t0), iterations_max=int(sol_new["iterations"].max()),
                       iterations_mean=float(sol_new["iterations"].mean()), converged=int((sol_new["status"] == 0).sum()),
                       start_miss=float(np.abs(sol_new["x"] - x).max()))
            sol = sol_new
            rows.append(row)
        rows = rows[1:]
        out = {"part": "e", "leg": leg, "instances": Bc, "steps": len(rows), "target_move_max": 0.05,
               "foreground_ms_min_median_max": [float(f(np.array([q["foreground_ms"] for q in rows]))) for f in (np.min, np.median, np.max)],
               "iterations_max_per_step": [q["iterations_max"] for q in rows],
               "iterations_mean_per_step": [round(q["iterations_mean"], 2) for q in rows],
               "start_to_solution_inf_max": max(q["start_miss"] for q in rows), "converged_min": min(q["converged"] for q in rows)}
        if leg == "predictor":
            out["background_ms_min_median_max"] = [float(f(np.array([q["background_ms"] for q in rows]))) for f in (np.min, np.median, np.max)]
            out["left_out_max"] = max(q["left_out"] for q in rows)
        print(json.dumps(out))
        s.close()
    eng.close()


def part_c():
    Bc = B_C
    rng = np.random.RandomState(2)
    targets = rng.uniform(-1.5, 1.5, size=(Bc, 3))
    base = problems.quadrotor(K, NK)
    eng = NLPEngine(base, o, n_instances=Bc, device=0)
    for b in range(Bc):
        eng.set_instance_constants(b, problems.quadrotor(K, NK, pref=tuple(targets[b])).GetOpimalProblemFuns().consts)
    n, m = eng.n, eng.m
    params = X0_IDX.astype(np.int32)
    P = len(params)
    d_idx = torch.from_numpy(X0_IDX).cuda()
    d_dt = torch.full((Bc, 1), 0.1, dtype=torch.float64, device="cuda")
    state0 = np.zeros((Bc, 12))
    state0[:, :3] = rng.uniform(-0.3, 0.3, size=(Bc, 3))
    noise = np.random.RandomState(11).normal(0.0, 0.02, size=(STEPS, Bc, 12))

    def solver():
        s = BatchedIPM(eng, tol=1e-6)
        return s

    def warm_options(s):
        s.set_option("mu_init", 1e-4)
        for k in ("warm_start_bound_push", "warm_start_bound_frac", "warm_start_slack_bound_push", "warm_start_slack_bound_frac"):
            s.set_option(k, 1e-6)
        s.set_option("warm_start_mult_bound_push", 1e-8)

    def buffers():
        z = lambda w: torch.zeros((Bc, w), dtype=torch.float64, device="cuda")
        return [torch.from_numpy(np.tile(eng.get_starting_point()[:n], (Bc, 1))).cuda(), z(m), z(n), z(n)]

    legs = {}
    for name in ("plain", "advanced step"):
        s = solver()
        cur, nxt = buffers(), buffers()
        d_state = torch.from_numpy(state0).cuda()
        s.set_initial_states_dev(0, d_state)
        s.solve_dev(cur[0], cur[1])                                   # the first plan: cold
        s.bound_multipliers_dev(cur[2], cur[3])
        eng.shift_plan_batch_dev(d_dt, cur[0], nxt[0], cur[1], nxt[1], cur[2], cur[3], nxt[2], nxt[3])
        warm_options(s)
        legs[name] = dict(s=s, cur=nxt, nxt=cur, rows=[])
    d_dx = torch.empty((Bc, P, n), dtype=torch.float64, device="cuda")
    d_dl = torch.empty((Bc, P, m), dtype=torch.float64, device="cuda")
    d_xp, d_lp = torch.empty((Bc, n), dtype=torch.float64, device="cuda"), torch.empty((Bc, m), dtype=torch.float64, device="cuda")
    for step in range(STEPS):
        for name, L in legs.items():
            s, cur, nxt = L["s"], L["cur"], L["nxt"]
            predicted = cur[0].index_select(1, d_idx).clone()
            measured = predicted + torch.from_numpy(noise[step]).cuda()
            row = {"step": step}
            if name == "advanced step":
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.set_initial_states_dev(0, predicted)
                rb = s.solve_dev(cur[0], cur[1], d_z_L=cur[2], d_z_U=cur[3], warm=True)
                info = s.sensitivities_dev(params, d_dx, d_dl)["info"]
                torch.cuda.synchronize()
                row.update(background_ms=1e3 * (time.perf_counter() - t0), background_iterations=int(rb["iterations"].max()),
                           regularised=int((info == 1).sum()), left_out=int((info == 2).sum()))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "advanced step":
                delta = measured - predicted
                s.apply_sensitivities_dev(params, d_dx, delta, cur[0], d_xp, d_dl, cur[1], d_lp)
                cur[0].copy_(d_xp)
                cur[1].copy_(d_lp)
            s.set_initial_states_dev(0, measured)
            r = s.solve_dev(cur[0], cur[1], d_z_L=cur[2], d_z_U=cur[3], warm=True)
            s.bound_multipliers_dev(cur[2], cur[3])
            eng.shift_plan_batch_dev(d_dt, cur[0], nxt[0], cur[1], nxt[1], cur[2], cur[3], nxt[2], nxt[3])
            torch.cuda.synchronize()
            row.update(foreground_ms=1e3 * (time.perf_counter() - t0), iterations_max=int(r["iterations"].max()),
                       iterations_mean=float(r["iterations"].mean()), converged=int((r["status"] == 0).sum()))
            L["rows"].append(row)
            L["cur"], L["nxt"] = nxt, cur
    for name, L in legs.items():
        rows = L["rows"][1:]                                          # (the first step carries one-time costs)
        out = {"part": "c", "leg": name, "instances": Bc, "steps": len(rows), "measured_minus_predicted_sigma": 0.02,
               "foreground_ms_min_median_max": [float(f(np.array([q["foreground_ms"] for q in rows]))) for f in (np.min, np.median, np.max)],
               "iterations_max_per_step": [q["iterations_max"] for q in rows],
               "iterations_mean_per_step": [round(q["iterations_mean"], 2) for q in rows],
               "converged_min": min(q["converged"] for q in rows)}
        if name == "advanced step":
            out["background_ms_min_median_max"] = [float(f(np.array([q["background_ms"] for q in rows]))) for f in (np.min, np.median, np.max)]
            out["background_iterations_per_step"] = [q["background_iterations"] for q in rows]
            out["regularised_max"] = max(q["regularised"] for q in rows)
            out["left_out_max"] = max(q["left_out"] for q in rows)
        print(json.dumps(out))
        L["s"].close()
    eng.close()


if __name__ == "__main__":
    if set("abd") & set(PARTS):
        part_a_b()
    if "c" in PARTS:
        part_c()
    if "e" in PARTS:
        part_e()
