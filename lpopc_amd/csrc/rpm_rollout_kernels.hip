// rpm_rollout_kernels.hip — the plant of a sweep's closed loop: every instance's own dynamics integrated under its plan's control
// over a control period (rpm_rollout_batch*), without leaving the device.  Instance b integrates
//     y' = f(t, y, u(t), p_b; consts_b),   f = the functor's dae() (path outputs ignored), p_b = the plan's static parameters,
// with n_steps classical Runge-Kutta steps of h = dt[b] / n_steps from t_start[b].  u(t) is "the plan at time t" of
// rpm_carry_device.hpp: the carry's knots, its natural cubic spline through a control's N nodes and its value at tau = 1
// (post_spline_end), evaluated with carry_eval at carry_coord(t) — the control the shift, the sampler and the extraction see.
// Per step, exactly (the tests restate it operation by operation):
//     t_i = t_start + i h;   k1 = f(t_i, y, u(t_i));   k2 = f(t_i + h / 2, y + (h / 2) k1, u(t_i + h / 2));
//     k3 = f(t_i + h / 2, y + (h / 2) k2, u(t_i + h / 2));   k4 = f(t_i + h, y + h k3, u(t_i + h));
//     acc = k1; acc = acc + 2 k2; acc = acc + 2 k3; acc = acc + k4;   y = y + (h / 6) acc
// hold == 1: u is u(t_start) for the whole call (the zero-order hold of a digital controller).  Controls are not clipped.
#include "rpm_carry_device.hpp"

namespace rpm {

// Workgroup (tile of TB instances), 256 threads: the knots and the phase's nu control columns staged into LDS (CarryLds with
// ncols = nu) and the spline's recurrences run by all threads through the carry's stages; then one lane per instance integrates
// out of LDS, holding y, the stage state, k and acc in registers.  State columns are not splined.  state0 may be state_out.
template <class Prob>
__global__ void __launch_bounds__(256)
rpm_rollout_kernel(const KParams K, int phase, int B, int TB, const double* __restrict__ x, const double* __restrict__ t_start,
                   const double* __restrict__ dt, int n_steps, int hold, const double* state0, double* state_out,
                   double* __restrict__ traj, int* __restrict__ verdicts) {
  constexpr int NX = Prob::NX, NU = Prob::NU, NC = Prob::NC;
  constexpr int NXs = NX > 0 ? NX : 1, NUs = NU > 0 ? NU : 1, NCs = NC > 0 ? NC : 1;
  extern __shared__ __align__(16) double rollout_sm[];
  const PhaseDev ph = K.phases[phase];
  const int N = ph.N, M = N + 1;
  const CarryLds L(M, TB, NU);
  const int Mp = L.Mp;
  double* pts = rollout_sm + L.pts;
  double* tau = rollout_sm + L.tau;
  double* mu = rollout_sm + L.mu;
  double* ys = rollout_sm + L.y;
  double* cs = rollout_sm + L.c;
  const int b0 = blockIdx.x * TB;
  const int nb = B - b0 < TB ? B - b0 : TB;
  const int tid = threadIdx.x, nt = blockDim.x;
  const double* fp = K.points + ph.node0;

  // ---- stage: points, every instance's knots, the control columns; then the carry's recurrences ----------------------------
  for (int k = tid; k < N; k += nt) pts[k] = fp[k];
  carry_stage_knots(tau, Mp, fp, N, nb, [&](int bi, double* t0, double* tf) {
    const double* xb = x + size_t(b0 + bi) * K.n;
    *t0 = xb[ph.x_t0];
    *tf = xb[ph.x_t0 + 1];
  });
  for (int idx = tid; idx < nb * NU * M; idx += nt) {
    const int k = idx % M, j = (idx / M) % NUs, bi = idx / (M * NUs);
    const double* xb = x + size_t(b0 + bi) * K.n;
    ys[(bi * NU + j) * Mp + k] = k < N ? xb[ph.x_control0 + j * N + k] : 0.0;   // the entry at tau = 1 is computed below
  }
  __syncthreads();
  carry_stage_mu_and_ends(tau, mu, ys, pts, Mp, N, nb, NU, [](int) { return true; });
  __syncthreads();
  carry_stage_second(tau, mu, ys, cs, Mp, M, nb * NU, NUs);
  __syncthreads();

  // ---- one lane per instance: classical Runge-Kutta out of LDS --------------------------------------------------------------
  if (tid >= nb) return;
  const int bi = tid;
  const size_t b = size_t(b0 + bi);
  const double* xb = x + b * K.n;
  const double t0 = xb[ph.x_t0], tf = xb[ph.x_t0 + 1];
  const double* par = xb + ph.x_t0 + 2;
  const double* consts = K.consts + b * K.consts_stride;
  const double* xd = tau + bi * Mp;
  double y[NXs], st[NXs], k[NXs], acc[NXs], u[NUs], cp[NCs];
#pragma unroll
  for (int s = 0; s < NX; ++s) y[s] = state0 ? state0[b * NX + s] : xb[ph.x_state0 + s * M];
  const double ts = t_start ? t_start[b] : post_time(t0, tf, fp[0]);
  const double h = dt[b] / n_steps;
  auto control = [&](double t) {   // the sampling rule: every control column at the coordinate of t
    const double s = carry_coord(t, t0, tf, fp[0]);
#pragma unroll
    for (int j = 0; j < NU; ++j) u[j] = carry_eval(s, xd, ys + (bi * NU + j) * Mp, cs + (bi * NU + j) * Mp, M);
  };
  bool bad = false;
  double* tr = traj ? traj + b * (size_t(n_steps) + 1) * NX : nullptr;
#pragma unroll
  for (int s = 0; s < NX; ++s) {
    bad |= nonfinite(y[s]);
    if (tr) tr[s] = y[s];
  }
  if (hold) control(ts);
  for (int i = 0; i < n_steps; ++i) {
    const double ti = ts + i * h;
    if (!hold) control(ti);
    pf_dae<Prob>(ph.phase_num, ti, y, u, par, consts, k, cp);                       // k1
#pragma unroll
    for (int s = 0; s < NX; ++s) {
      acc[s] = k[s];
      st[s] = y[s] + (h / 2) * k[s];
    }
    if (!hold) control(ti + h / 2);
    pf_dae<Prob>(ph.phase_num, ti + h / 2, st, u, par, consts, k, cp);              // k2
#pragma unroll
    for (int s = 0; s < NX; ++s) {
      acc[s] = acc[s] + 2 * k[s];
      st[s] = y[s] + (h / 2) * k[s];
    }
    pf_dae<Prob>(ph.phase_num, ti + h / 2, st, u, par, consts, k, cp);              // k3, u as for k2: the same time
#pragma unroll
    for (int s = 0; s < NX; ++s) {
      acc[s] = acc[s] + 2 * k[s];
      st[s] = y[s] + h * k[s];
    }
    if (!hold) control(ti + h);
    pf_dae<Prob>(ph.phase_num, ti + h, st, u, par, consts, k, cp);                  // k4
#pragma unroll
    for (int s = 0; s < NX; ++s) {
      acc[s] = acc[s] + k[s];
      y[s] = y[s] + (h / 6) * acc[s];
      bad |= nonfinite(y[s]);
      if (tr) tr[size_t(i + 1) * NX + s] = y[s];
    }
  }
#pragma unroll
  for (int s = 0; s < NX; ++s) state_out[b * NX + s] = y[s];
  if (verdicts) verdicts[b] = bad ? 1 : 0;
}

namespace {

constexpr int kRolloutAutoTile = 4;   // DESIGN.md §4 K8; tools/bench_sweep_rollout.py measures every value

struct RolloutState {
  bool raised = false;   // the kernel's dynamic-LDS limit was raised on this device
  HostForm host;         // host-pointer form: t_start, dt, state0, state_out and traj in one block
};

RolloutState& rollout_state(Device& d) {
  if (!d.rollout) d.rollout = new RolloutState();
  return *static_cast<RolloutState*>(d.rollout);
}

// Host planner: instances per workgroup, halved until the knots and the nu control columns of the tile fit the LDS one workgroup
// may use (option "carry_lds_bytes" lowers it, as for the carry); false: they do not fit even at one instance per workgroup.
bool rollout_plan(const Engine& e, int phase, int* TB_out, size_t* lds_out) {
  const size_t budget = lds_budget(e.opt_carry_lds, kCuLdsBytes);
  const PhaseHost& p = e.ph[size_t(phase)];
  auto bytes = [&](int TB) { return size_t(CarryLds(p.N + 1, TB, p.nu).total) * sizeof(double); };
  *TB_out = halve_tile(clamp_tile(e.opt_rollout_tile > 0 ? e.opt_rollout_tile : kRolloutAutoTile, e.n_instances),
                       [&](int TB) { return bytes(TB) <= budget; });
  *lds_out = *TB_out ? bytes(*TB_out) : 0;
  return *TB_out > 0;
}

int rollout_launch(Engine& e, int phase, const RolloutArrays& a, int n_steps, int hold, int* d_nonfinite, hipStream_t st) {
  Device& d = *e.dev;   // made current by dev_bind
  RolloutState& rs = rollout_state(d);
  int TB = 1;
  size_t lds = 0;
  if (!rollout_plan(e, phase, &TB, &lds)) return step_fail(e, RPM_E_UNSUPPORTED, "rollout_batch: the control columns do not fit one workgroup's LDS");
  const int B = e.n_instances;
  hipError_t s = hipSuccess;
  const bool known = with_problem(e.problem_id, [&](auto prob) {
    using P = decltype(prob);
    if (lds > 64 * 1024 && !rs.raised) {
      s = raise_dynamic_lds(reinterpret_cast<const void*>(rpm_rollout_kernel<P>), lds);
      rs.raised = s == hipSuccess;
    }
    if (s != hipSuccess) return;
    hipLaunchKernelGGL((rpm_rollout_kernel<P>), dim3(unsigned((B + TB - 1) / TB)), dim3(256), lds, st, d.kp, phase, B, TB, a.x, a.t_start,
                       a.dt, n_steps, hold, a.state0, a.state_out, a.traj, d_nonfinite);
  });
  if (!known) return step_no_kernels(e, "rollout_batch");
  return step_launched(e, "rollout_batch", s);
}

}  // namespace

void rollout_destroy(Device* d) {
  RolloutState* rs = static_cast<RolloutState*>(d->rollout);
  if (!rs) return;
  rs->host.release();
  delete rs;
  d->rollout = nullptr;
}

// every argument error of the roll-out, decided on the host before a device is touched (all host or all device pointers)
int rollout_check(Engine& e, int phase, const RolloutArrays& a, int n_steps, int hold) {
  const std::string who = "rollout_batch: ";
  if (!a.x) return step_fail(e, RPM_E_INVALID, who + "x is NULL");
  if (!a.dt) return step_fail(e, RPM_E_INVALID, who + "dt is NULL");
  if (!a.state_out) return step_fail(e, RPM_E_INVALID, who + "state_out is NULL");
  if (n_steps < 1 || n_steps > 65536) return step_fail(e, RPM_E_INVALID, who + "n_steps must be 1 ... 65536");
  if (hold != 0 && hold != 1) return step_fail(e, RPM_E_INVALID, who + "hold must be 0 or 1");
  if (phase < 0 || phase >= e.P) return step_fail(e, RPM_E_INVALID, who + "the phase index is out of range");
  const PhaseHost& p = e.ph[size_t(phase)];
  const size_t B = size_t(e.n_instances), Bs = B * p.nx * sizeof(double);
  const ByteRange in[4] = {{"x", a.x, B * e.n * sizeof(double)}, {"t_start", a.t_start, B * sizeof(double)}, {"dt", a.dt, B * sizeof(double)},
                           {"state0", a.state0, Bs}};
  const ByteRange out[2] = {{"state_out", a.state_out, Bs}, {"traj", a.traj, Bs * (size_t(n_steps) + 1)}};
  // each output against the inputs before the outputs against each other; state0 last, left out for a state updated in place
  int rc = step_overlap(e, who, &out[0], 1, in, a.state_out == a.state0 ? 3 : 4);
  if (rc == RPM_OK) rc = step_overlap(e, who, &out[1], 1, in, 4);
  if (rc == RPM_OK) rc = step_overlap(e, who, out, 2, in, 0);
  if (rc) return rc;
  if (sharded(e)) return step_fail(e, RPM_E_UNSUPPORTED, who + "not with interval sharding");
  int TB = 0;
  size_t lds = 0;
  if (!rollout_plan(e, phase, &TB, &lds))
    return step_fail(e, RPM_E_UNSUPPORTED, who + "the " + std::to_string(p.nu) + " control columns of " + std::to_string(p.N + 1) +
                                                  " knots do not fit one workgroup's LDS");
  return RPM_OK;
}

// device-resident: one launch on `stream`, nothing else
int dev_rollout_batch(Engine& e, int phase, const RolloutArrays& a, int n_steps, int hold, int* d_nonfinite, void* stream) {
  int rc = rollout_check(e, phase, a, n_steps, hold);
  if (rc) return rc;
  DeviceRestore restore;
  rc = dev_bind(e);
  if (rc) return rc;
  return rollout_launch(e, phase, a, n_steps, hold, d_nonfinite, static_cast<hipStream_t>(stream));
}

// the same through host arrays: everything up through the staging slots into one device block, the results back; blocking
int host_rollout_batch(Engine& e, int phase, const RolloutArrays& a, int n_steps, int hold, int* nonfinite) {
  int rc = rollout_check(e, phase, a, n_steps, hold);
  if (rc) return rc;
  DeviceRestore restore;
  rc = dev_bind(e);
  if (rc) return rc;
  Device& d = *e.dev;
  const size_t B = size_t(e.n_instances), Bs = B * size_t(e.ph[size_t(phase)].nx), Bt = a.traj ? Bs * (size_t(n_steps) + 1) : 0;
  const size_t o_dt = B, o_s0 = o_dt + B, o_so = o_s0 + Bs, o_traj = o_so + Bs;   // the block: t_start first
  return rollout_state(d).host.run(
      e, o_traj + Bt,
      {{d.d_x, 0, a.x, B * e.n, STAGE_X}, {nullptr, o_dt, a.dt, B, STAGE_G}, {nullptr, 0, a.t_start, B, STAGE_V},
       {nullptr, o_s0, a.state0, Bs, STAGE_GRAD}},
      [&](double* b, int* flags) {
        const RolloutArrays dv{d.d_x, a.t_start ? b : nullptr, b + o_dt, a.state0 ? b + o_s0 : nullptr, b + o_so, a.traj ? b + o_traj : nullptr};
        return rollout_launch(e, phase, dv, n_steps, hold, flags, d.stream);
      },
      {{a.state_out, nullptr, o_so, Bs, STAGE_G}, {a.traj, nullptr, o_traj, Bt, STAGE_LAMBDA}}, nonfinite);
}

}  // namespace rpm
