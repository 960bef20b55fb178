// rpm_carry_kernels.hip — the solutions of a whole sweep carried onto another mesh of the same problem: what lpopc does
// between two meshes (Nlp2OpConverter::Nlp2OpControl installs time / state / control / parameter as the next guess,
// Core/Nlp2OPConverter.cpp:160-193; LpGuessChecker splines it onto the new nodes, Core/LpGuessChecker.cpp:208-294), for all
// instances of an engine at once and without leaving the device.  Per instance, phase and column, in this order:
//   1. time[k] = post_time(t0, tf, tau_k) at the N LGR points and at tau = 1                     (rpm_post_device.hpp)
//   2. controls only: the value at tau = 1, post_spline_end through the N points                (rpm_post_spline_kernel)
//   3. knots tau_g[k] = 2 * (time[k] - time[0]) / (time[N] - time[0]) - 1                       (rpm_setup.cpp, starting point)
//   4. the natural cubic spline of spline_eval (rpm_setup.cpp) through the N + 1 knots, evaluated at the target phase's
//      points, states also at 1.0
//   5. t0 = time[0], tf = time[N]; static parameters copied.
// Everything but the cubes of step 4 repeats the one-instance path (rpm_nlp2op_control, a new rpm_create carrying the guess,
// rpm_get_starting_point) operation by operation; the cubes are A * A * A here and glibc's pow(A, 3) there.
// The receding-horizon shift of a plan (rpm_shift_plan_batch*) is the same kernel with from == to and every evaluation point
// moved by the instance's own 2 dt / (time[N] - time[0]), clamped into [-1, 1]; bound multipliers ride it piecewise linearly.
// The plans at caller-given times (rpm_sample_plan_batch*) are steps 1 - 3 and the spline of step 4 evaluated at the coordinate
// of every time (rpm_sample_kernel).  The spline's rules are in rpm_carry_device.hpp, shared with the roll-out.
#include "rpm_carry_device.hpp"

namespace rpm {

// One workgroup's share: columns [col0, col0 + ncols) of a phase (states first, then controls) for a tile of instances.
struct CarryGroup {
  int phase, col0, ncols;
  int first;   // the phase's first group also writes t0, tf and the static parameters
};

// A phase's rows of g / lambda: defects (nx x N, state-major), path rows (nc x N), events (ne); after the last phase's: the tail.
struct CarryRows {
  int defect0, path0, event0, end;
  __host__ __device__ constexpr CarryRows(int g0, int N, int nx, int nc, int ne)
      : defect0(g0), path0(g0 + N * nx), event0(path0 + N * nc), end(event0 + ne) {}
};
static_assert(CarryRows(7, 5, 3, 2, 4).path0 == 22 && CarryRows(7, 5, 3, 2, 4).event0 == 32 && CarryRows(7, 5, 3, 2, 4).end == 36, "CarryRows");

// What the multipliers' carry needs beyond the solutions': lam_from NULL = the solution carry, which reads nothing else of this.
struct CarryMult {
  const double* lam_from;   // n_instances x m_from
  double* lam_to;           // n_instances x m_to
  KParams K;                // the source engine's tables (weights, nodes, D rows: post_end_costate)
  const double* tw;         // the target engine's weights
  int m_from, m_to, P;
};

// What the shift of a plan needs beyond the carry: dt NULL = a carry, which reads nothing else of this.
struct CarryShift {
  const double* dt;       // n_instances x P: every phase's own advance in the problem's time unit
  const double* z_from;   // not NULL: a bound-multiplier array in x's layout supplies the columns (x_from still the knots), which
                          // are interpolated piecewise linearly; its entries at t0, tf and the parameters are copied
  int P;
};

// CarryLds, the spline's helpers (carry_locate, carry_eval, carry_eval_linear, carry_shifted, carry_coord) and the three
// per-workgroup stages between staging and evaluation: rpm_carry_device.hpp, shared with the roll-out.

// Workgroup (group of columns of a phase, tile of TB instances), 256 threads.  x is instance-major with every column
// contiguous in k, so the columns are staged with k-fastest loads; one lane per (instance, column) runs the recurrences out
// of LDS; all lanes evaluate, the outputs of one (instance, column) on consecutive lanes, so the stores are contiguous runs.
__global__ void __launch_bounds__(256)
rpm_carry_kernel(const PhaseDev* __restrict__ fph, const double* __restrict__ fpts, int n_from, const PhaseDev* __restrict__ tph,
                 const double* __restrict__ tpts, int n_to, const CarryGroup* __restrict__ groups, int B, int TB,
                 const double* __restrict__ x_from, double* __restrict__ x_to, CarryMult mu_, CarryShift sh) {
  extern __shared__ __align__(16) double carry_sm[];
  const CarryGroup v = groups[blockIdx.x];
  const PhaseDev pf = fph[v.phase], pt = tph[v.phase];
  const int N = pf.N, M = N + 1, Nt = pt.N, nx = pf.nx, ncols = v.ncols;
  const bool mult = mu_.lam_from != nullptr;
  const KParams& K = mu_.K;
  const double *__restrict__ lam_from = mu_.lam_from, *__restrict__ tw = mu_.tw;
  double* __restrict__ lam_to = mu_.lam_to;
  const int m_from = mu_.m_from, m_to = mu_.m_to, P = mu_.P;
  const double *__restrict__ dts = sh.dt, *__restrict__ z_from = sh.z_from;
  const bool lin = z_from != nullptr;
  const CarryRows rf(pf.g0, N, nx, pf.nc, pf.ne), rt(pt.g0, Nt, nx, pt.nc, pt.ne);
  const CarryLds L(M, TB, ncols);
  const int Mp = L.Mp;
  double* pts = carry_sm + L.pts;
  double* tau = carry_sm + L.tau;
  double* mu = carry_sm + L.mu;
  double* ys = carry_sm + L.y;
  double* cs = carry_sm + L.c;
  const int b0 = blockIdx.y * TB;
  const int nb = B - b0 < TB ? B - b0 : TB;
  const int tid = threadIdx.x, nt = blockDim.x;
  const double* fp = fpts + pf.node0;

  // ---- stage: points, every instance's knots, the columns ------------------------------------------------------
  for (int k = tid; k < N; k += nt) pts[k] = fp[k];
  carry_stage_knots(tau, Mp, fp, N, nb, [&](int bi, double* t0, double* tf) {
    const double* xb = x_from + size_t(b0 + bi) * n_from;
    *t0 = xb[pf.x_t0];
    *tf = xb[pf.x_t0 + 1];
  });
  for (int idx = tid; idx < nb * ncols * M; idx += nt) {
    const int k = idx % M, cl = (idx / M) % ncols, bi = idx / (M * ncols);
    const double* xb = x_from + size_t(b0 + bi) * n_from;
    const int col = v.col0 + cl;
    double val = 0.0;   // a control's entry at tau = 1 is computed below
    if (mult) {
      const double* lb = lam_from + size_t(b0 + bi) * m_from;
      if (col < nx) val = k < N ? -((1 / K.weights[pf.node0 + k]) * lb[rf.defect0 + col * N + k]) : post_end_costate(K, pf, lb + pf.g0, col);
      else if (k < N) val = (1 / K.weights[pf.node0 + k]) * lb[rf.path0 + (col - nx) * N + k];
    } else {
      const double* vb = lin ? z_from + size_t(b0 + bi) * n_from : xb;
      if (col < nx) val = vb[pf.x_state0 + col * M + k];
      else if (k < N) val = vb[pf.x_control0 + (col - nx) * N + k];
    }
    ys[(bi * ncols + cl) * Mp + k] = val;
  }
  __syncthreads();

  // ---- wave 0: mu, once per instance.  The other waves: the controls' values at tau = 1 -------------------------------
  if (lin) {   // piecewise linear: no recurrences; a control's knot at 1 holds its last node's value
    for (int r = tid; r < nb * ncols; r += nt)
      if (v.col0 + r % ncols >= nx) ys[r * Mp + N] = ys[r * Mp + N - 1];
  } else
    carry_stage_mu_and_ends(tau, mu, ys, pts, Mp, N, nb, ncols, [&](int r) { return v.col0 + r % ncols >= nx; });
  __syncthreads();

  // ---- one lane per (instance, column): forward recurrence, back substitution, interior c doubled ------------------
  carry_stage_second(tau, mu, ys, cs, Mp, M, lin ? 0 : nb * ncols, ncols);
  __syncthreads();

  // ---- evaluate and store: states at the target's points and at 1.0, controls at the points ---------------------
  const double* tp = tpts + pt.node0;
  const int ns = nx - v.col0 < 0 ? 0 : (nx - v.col0 < ncols ? nx - v.col0 : ncols);   // state columns of this group
  const int nc = ncols - ns, Q = mult ? Nt : Nt + 1;
  // the point a value is taken at: the target's own, or (shift) that point moved on by the instance's dt of this phase
  auto at = [&](int bi, double tau_q) -> double {
    if (!dts) return tau_q;
    const double* xb = x_from + size_t(b0 + bi) * n_from;
    return carry_shifted(tau_q, dts[size_t(b0 + bi) * sh.P + v.phase], xb[pf.x_t0], xb[pf.x_t0 + 1], fp[0]);
  };
  auto eval = [&](int bi, int r, double tau_q) -> double {
    const double x = at(bi, tau_q);
    return lin ? carry_eval_linear(x, tau + bi * Mp, ys + r * Mp, M) : carry_eval(x, tau + bi * Mp, ys + r * Mp, cs + r * Mp, M);
  };
  for (int idx = tid; idx < nb * ns * Q; idx += nt) {
    const int q = idx % Q, cl = (idx / Q) % ns, bi = idx / (Q * ns);
    const int r = bi * ncols + cl;
    const double val = eval(bi, r, q < Nt ? tp[q] : 1.0);
    if (mult) lam_to[size_t(b0 + bi) * m_to + rt.defect0 + (v.col0 + cl) * Nt + q] = -(tw[pt.node0 + q] * val);
    else x_to[size_t(b0 + bi) * n_to + pt.x_state0 + (v.col0 + cl) * Q + q] = val;
  }
  for (int idx = tid; idx < nb * nc * Nt; idx += nt) {
    const int q = idx % Nt, cl = ns + (idx / Nt) % nc, bi = idx / (Nt * nc);
    const int r = bi * ncols + cl;
    const double val = eval(bi, r, tp[q]);
    if (mult) lam_to[size_t(b0 + bi) * m_to + rt.path0 + (v.col0 + cl - nx) * Nt + q] = tw[pt.node0 + q] * val;
    else x_to[size_t(b0 + bi) * n_to + pt.x_control0 + (v.col0 + cl - nx) * Nt + q] = val;
  }
  if (v.first && mult) {   // the phase's event rows; the last phase's first group: the rows after the phases too
    const int tail = v.phase == P - 1 ? m_from - rf.end : 0, cnt = pf.ne + tail;
    for (int idx = tid; idx < nb * cnt; idx += nt) {
      const int j = idx % cnt, bi = idx / cnt;
      lam_to[size_t(b0 + bi) * m_to + rt.event0 + j] = lam_from[size_t(b0 + bi) * m_from + rf.event0 + j];
    }
  } else if (v.first)
    for (int idx = tid; idx < nb * (2 + pf.nq); idx += nt) {
      const int j = idx % (2 + pf.nq), bi = idx / (2 + pf.nq);
      const double* xb = x_from + size_t(b0 + bi) * n_from;
      const double t0 = xb[pf.x_t0], tf = xb[pf.x_t0 + 1];
      double val;
      if (lin) val = z_from[size_t(b0 + bi) * n_from + pf.x_t0 + j];
      else if (j == 0) val = post_time(t0, tf, fp[0]);     // time[0]
      else if (j == 1) val = post_time(t0, tf, 1.0);       // time[N]
      else val = xb[pf.x_t0 + j];
      x_to[size_t(b0 + bi) * n_to + pt.x_t0 + j] = val;
    }
}

// The plans sampled at caller-given times (rpm_sample_plan_batch*): the carry's staging, knots and recurrences for one phase's
// columns, every column then evaluated with carry_eval at carry_coord(t) of the instance's n_times times.  Workgroup (group of
// columns of the phase, tile of TB instances); out: per instance (nx + nu) columns of n_times rows, states first.
__global__ void __launch_bounds__(256)
rpm_sample_kernel(const PhaseDev* __restrict__ phd, const double* __restrict__ points, int n, const CarryGroup* __restrict__ groups,
                  int B, int TB, const double* __restrict__ x, int n_times, const double* __restrict__ times, double* __restrict__ out) {
  extern __shared__ __align__(16) double sample_sm[];
  const CarryGroup v = groups[blockIdx.x];
  const PhaseDev pf = phd[v.phase];
  const int N = pf.N, M = N + 1, nx = pf.nx, ncols = v.ncols;
  const CarryLds L(M, TB, ncols);
  const int Mp = L.Mp;
  double* pts = sample_sm + L.pts;
  double* tau = sample_sm + L.tau;
  double* mu = sample_sm + L.mu;
  double* ys = sample_sm + L.y;
  double* cs = sample_sm + L.c;
  const int b0 = blockIdx.y * TB;
  const int nb = B - b0 < TB ? B - b0 : TB;
  const int tid = threadIdx.x, nt = blockDim.x;
  const double* fp = points + pf.node0;
  for (int k = tid; k < N; k += nt) pts[k] = fp[k];
  carry_stage_knots(tau, Mp, fp, N, nb, [&](int bi, double* t0, double* tf) {
    const double* xb = x + size_t(b0 + bi) * n;
    *t0 = xb[pf.x_t0];
    *tf = xb[pf.x_t0 + 1];
  });
  for (int idx = tid; idx < nb * ncols * M; idx += nt) {
    const int k = idx % M, cl = (idx / M) % ncols, bi = idx / (M * ncols);
    const double* xb = x + size_t(b0 + bi) * n;
    const int col = v.col0 + cl;
    double val = 0.0;   // a control's entry at tau = 1 is computed below
    if (col < nx) val = xb[pf.x_state0 + col * M + k];
    else if (k < N) val = xb[pf.x_control0 + (col - nx) * N + k];
    ys[(bi * ncols + cl) * Mp + k] = val;
  }
  __syncthreads();
  carry_stage_mu_and_ends(tau, mu, ys, pts, Mp, N, nb, ncols, [&](int r) { return v.col0 + r % ncols >= nx; });
  __syncthreads();
  carry_stage_second(tau, mu, ys, cs, Mp, M, nb * ncols, ncols);
  __syncthreads();
  const int cols = nx + pf.nu;
  for (long long idx = tid; idx < (long long)nb * ncols * n_times; idx += nt) {
    const int q = int(idx % n_times), r = int(idx / n_times), bi = r / ncols, cl = r % ncols;
    const size_t b = size_t(b0 + bi);
    const double* xb = x + b * n;
    const double s = carry_coord(times[b * n_times + q], xb[pf.x_t0], xb[pf.x_t0 + 1], fp[0]);
    out[(b * cols + v.col0 + cl) * n_times + q] = carry_eval(s, tau + bi * Mp, ys + r * Mp, cs + r * Mp, M);
  }
}

static CarryRows carry_rows(const Engine& e, int phase) {
  const PhaseHost& p = e.ph[size_t(phase)];
  return CarryRows(p.con0, p.N, p.nx, p.nc, p.ne);
}

namespace {

struct CarryPlan {
  long long to_serial = 0;
  int tile_opt = 0, lds_opt = 0;   // the options the plan was made under
  int mult = 0;                    // 1: the plan of the multipliers' columns (nx + nc per phase), 0: the solution's (nx + nu)
  int TB = 1, n_groups = 0;
  size_t lds = 0;
  CarryGroup* d_groups = nullptr;
  std::vector<int> group0;         // per phase its first group, then n_groups: the sampler launches one phase's groups
};
struct CarryState {
  std::vector<CarryPlan> plans;
  HostForm host;    // host-pointer form: the carried block
  HostForm shift;   // host-pointer form of the shift: dt, the four inputs and the four outputs in one block
  HostForm sample;  // host-pointer form of the sampler: the times and the samples in one block
};

// Host planner: instances per workgroup and the split of every phase's columns over workgroups.  Columns are independent,
// so a phase whose columns do not fit one workgroup's LDS is dealt over several; the tile shrinks before one column is refused.
bool carry_plan(const Engine& from, int mult, int* TB_out, std::vector<CarryGroup>* groups, size_t* lds_out) {
  const size_t budget = lds_budget(from.opt_carry_lds, kCuLdsBytes) / sizeof(double);
  auto fits = [&](const PhaseHost& p, int TB, int ncols) { return size_t(CarryLds(p.N + 1, TB, ncols).total) <= budget; };
  // automatic: 2 instances per workgroup (reasoned; tools/bench_sweep_carry.py measures every value)
  const int TB = halve_tile(clamp_tile(from.opt_carry_tile > 0 ? from.opt_carry_tile : 2, from.n_instances), [&](int tb) {
    return std::all_of(from.ph.begin(), from.ph.end(), [&](const PhaseHost& p) { return fits(p, tb, 1); });
  });
  if (!TB) return false;
  size_t lds = 0;
  if (groups) groups->clear();
  for (size_t ip = 0; ip < from.ph.size(); ++ip) {
    const PhaseHost& p = from.ph[ip];
    for (const auto& [col0, ncols] : split_columns(p.nx + (mult ? p.nc : p.nu), [&](int nc) { return fits(p, TB, nc); })) {
      lds = std::max(lds, size_t(CarryLds(p.N + 1, TB, ncols).total) * sizeof(double));
      if (groups) groups->push_back(CarryGroup{int(ip), col0, ncols, col0 == 0 ? 1 : 0});
    }
  }
  *TB_out = TB;
  *lds_out = lds;
  return true;
}
bool carry_fits(const Engine& e, int mult) {
  int TB = 0;
  size_t lds = 0;
  return carry_plan(e, mult, &TB, nullptr, &lds);
}

CarryState& carry_state(Device& d) {
  if (!d.carry) d.carry = new CarryState();
  return *static_cast<CarryState*>(d.carry);
}

// The launch plan of a pair of engines under from's options, made on the first call: the only allocation and the only blocking
// copy.  from's device is current (dev_bind).
int carry_plan_for(Engine& from, const Engine& to, int mult, const std::string& who, const CarryPlan** out) {
  CarryState& cs = carry_state(*from.dev);
  for (const CarryPlan& p : cs.plans)
    if (p.to_serial == to.serial && p.tile_opt == from.opt_carry_tile && p.lds_opt == from.opt_carry_lds && p.mult == mult) {
      *out = &p;
      return RPM_OK;
    }
  CarryPlan p;
  std::vector<CarryGroup> groups;
  if (!carry_plan(from, mult, &p.TB, &groups, &p.lds)) return step_fail(from, RPM_E_UNSUPPORTED, who + ": a column does not fit one workgroup's LDS");
  p.mult = mult;
  p.to_serial = to.serial;
  p.tile_opt = from.opt_carry_tile;
  p.lds_opt = from.opt_carry_lds;
  p.n_groups = int(groups.size());
  p.group0.assign(size_t(from.P) + 1, p.n_groups);   // groups are phase-major: phase i owns [group0[i], group0[i + 1])
  for (int g = p.n_groups - 1; g >= 0; --g) p.group0[size_t(groups[size_t(g)].phase)] = g;
  for (int i = from.P - 1; i >= 0; --i) p.group0[size_t(i)] = std::min(p.group0[size_t(i)], p.group0[size_t(i) + 1]);
  HIP_TRY(from, upload(&p.d_groups, groups));
  HIP_TRY(from, raise_dynamic_lds(reinterpret_cast<const void*>(rpm_carry_kernel), p.lds));
  HIP_TRY(from, raise_dynamic_lds(reinterpret_cast<const void*>(rpm_sample_kernel), p.lds));
  cs.plans.push_back(p);
  *out = &cs.plans.back();
  return RPM_OK;
}

// d_lam_from NULL: the solutions, x_from -> x_to; else the multipliers, lam_from -> lam_to with x_from's t0 / tf for the knots.
// sh.dt not NULL: the shift of a plan (from == to); sh.z_from not NULL: a bound-multiplier array z_from -> x_to.
int carry_launch(Engine& from, Engine& to, const double* d_x_from, double* d_x_to, const double* d_lam_from, double* d_lam_to,
                 int* d_nonfinite, hipStream_t st, CarryShift sh = CarryShift{}) {
  const char* who = sh.dt ? "shift_plan_batch" : (d_lam_from ? "carry_multipliers_batch" : "carry_solution_batch");
  const int mult = d_lam_from ? 1 : 0;
  const CarryPlan* plan = nullptr;
  const int rc = carry_plan_for(from, to, mult, who, &plan);
  if (rc) return rc;
  Device& d = *from.dev;
  const int B = from.n_instances;
  CarryMult cm{};
  if (mult) cm = CarryMult{d_lam_from, d_lam_to, d.kp, to.dev->d_weights, from.m, to.m, from.P};
  hipLaunchKernelGGL(rpm_carry_kernel, dim3(unsigned(plan->n_groups), unsigned((B + plan->TB - 1) / plan->TB)), dim3(256), plan->lds, st,
                     d.d_phases, d.d_points, from.n, to.dev->d_phases, to.dev->d_points, to.n, plan->d_groups, B, plan->TB, d_x_from,
                     d_x_to, cm, sh);
  if (d_nonfinite) flag_launch(mult ? to.m : to.n, mult ? d_lam_to : d_x_to, d_nonfinite, B, st);
  return step_launched(from, who);
}

}  // namespace

void carry_destroy(Device* d) {
  CarryState* cs = static_cast<CarryState*>(d->carry);
  if (!cs) return;
  for (CarryPlan& p : cs->plans)
    if (p.d_groups) (void)hipFree(p.d_groups);
  cs->host.release();
  cs->shift.release();
  cs->sample.release();
  delete cs;
  d->carry = nullptr;
}

int carry_group_count(const Engine& from) {
  int TB = 0;
  size_t lds = 0;
  std::vector<CarryGroup> groups;
  return carry_plan(from, 0, &TB, &groups, &lds) ? int(groups.size()) : 0;
}

// every argument error, decided on the host before a device is touched (x_from / x_to: both host or both device pointers;
// mult: the multipliers' arrays, n_instances x m, and the multipliers' columns)
int carry_check(Engine& from, const Engine& to, const void* x_from, const void* x_to, int mult) {
  const std::string who = mult ? "carry_multipliers_batch: " : "carry_solution_batch: ";
  for (int i = 0; i < std::min(from.P, to.P); ++i) {   // the sizes first: they say more than "another problem"
    const PhaseHost &a = from.ph[size_t(i)], &b = to.ph[size_t(i)];
    const std::string tag = " differs in phase " + std::to_string(i + 1);
    if (a.nx != b.nx) return step_fail(from, RPM_E_INVALID, who + "nx" + tag);
    if (a.nu != b.nu) return step_fail(from, RPM_E_INVALID, who + "nu" + tag);
    if (a.nq != b.nq) return step_fail(from, RPM_E_INVALID, who + "nq" + tag);
    if (mult && a.nc != b.nc) return step_fail(from, RPM_E_INVALID, who + "nc" + tag);
    if (mult && a.ne != b.ne) return step_fail(from, RPM_E_INVALID, who + "ne" + tag);
  }
  if (from.P != to.P) return step_fail(from, RPM_E_INVALID, who + "the engines have different phase counts");
  if (from.problem_id != to.problem_id) return step_fail(from, RPM_E_INVALID, who + "the engines hold different problems");
  if (from.n_instances != to.n_instances)
    return step_fail(from, RPM_E_INVALID, who + "n_instances differs (" + std::to_string(from.n_instances) + " and " +
                                               std::to_string(to.n_instances) + ")");
  if (from.dev && to.dev && from.dev->device_id != to.dev->device_id)
    return step_fail(from, RPM_E_INVALID, who + "the engines are bound to different devices");
  const size_t B = size_t(from.n_instances) * sizeof(double);   // two ranges, named in the arguments' order
  const ByteRange a{mult ? "lambda_from" : "x_from", x_from, B * (mult ? from.m : from.n)}, b{mult ? "lambda_to" : "x_to", x_to, B * (mult ? to.m : to.n)};
  if (const int rc = step_overlap(from, who, &a, 1, &b, 1)) return rc;
  if (mult && from.P > 0 && from.m - carry_rows(from, from.P - 1).end != to.m - carry_rows(to, to.P - 1).end)
    return step_fail(from, RPM_E_INVALID, who + "the rows after the last phase differ in number");
  if (sharded(from) || sharded(to)) return step_fail(from, RPM_E_UNSUPPORTED, who + "not with interval sharding");
  if (!carry_fits(from, mult)) return step_no_fit(from, who, "knots", 1);
  return RPM_OK;
}

// device-resident: one launch (two with the verdicts) on `stream`; after the first call on a pair of engines nothing else
int dev_carry_batch(Engine& from, Engine& to, const double* d_x_from, double* d_x_to, int* d_nonfinite, void* stream) {
  int rc = carry_check(from, to, d_x_from, d_x_to);
  if (rc) return rc;
  DeviceRestore restore;
  rc = dev_bind(from, &to);
  if (rc) return rc;
  return carry_launch(from, to, d_x_from, d_x_to, nullptr, nullptr, d_nonfinite, static_cast<hipStream_t>(stream));
}
int dev_carry_mult_batch(Engine& from, Engine& to, const double* d_x_from, const double* d_lam_from, double* d_lam_to, int* d_nonfinite,
                         void* stream) {
  int rc = carry_check(from, to, d_lam_from, d_lam_to, 1);
  if (rc) return rc;
  DeviceRestore restore;
  rc = dev_bind(from, &to);
  if (rc) return rc;
  return carry_launch(from, to, d_x_from, nullptr, d_lam_from, d_lam_to, d_nonfinite, static_cast<hipStream_t>(stream));
}

// the same through host arrays: x_from (and lam_from) up through the staging slots, the carried block and the verdicts back; blocking
int host_carry_batch(Engine& from, Engine& to, const double* x_from, double* x_to, int* nonfinite) {
  int rc = carry_check(from, to, x_from, x_to);
  if (rc) return rc;
  DeviceRestore restore;
  rc = dev_bind(from, &to);
  if (rc) return rc;
  Device& d = *from.dev;
  const size_t B = size_t(from.n_instances), count = B * to.n;
  return carry_state(d).host.run(
      from, count, {{d.d_x, 0, x_from, B * from.n, STAGE_X}},
      [&](double* out, int* flags) { return carry_launch(from, to, d.d_x, out, nullptr, nullptr, flags, d.stream); },
      {{x_to, nullptr, 0, count, STAGE_G}}, nonfinite);
}
int host_carry_mult_batch(Engine& from, Engine& to, const double* x_from, const double* lam_from, double* lam_to, int* nonfinite) {
  int rc = carry_check(from, to, lam_from, lam_to, 1);
  if (rc) return rc;
  DeviceRestore restore;
  rc = dev_bind(from, &to);
  if (rc) return rc;
  Device& d = *from.dev;
  const size_t B = size_t(from.n_instances), count = B * to.m;
  return carry_state(d).host.run(
      from, count, {{d.d_x, 0, x_from, B * from.n, STAGE_X}, {d.d_lambda, 0, lam_from, B * from.m, STAGE_LAMBDA}},
      [&](double* out, int* flags) { return carry_launch(from, to, d.d_x, nullptr, d.d_lambda, out, flags, d.stream); },
      {{lam_to, nullptr, 0, count, STAGE_G}}, nonfinite);
}

// ---- the receding-horizon shift of a plan: the carry onto the engine's own mesh, every point moved by the instance's dt ----

// nonfinite[b] = 1 when any of up to four blocks of instance b holds a NaN or Inf: rpm_flag_kernel over several arrays
struct ShiftFlagged {
  const double* v[4];
  long long len[4];
};
__global__ void __launch_bounds__(256) rpm_shift_flag_kernel(ShiftFlagged f, int* __restrict__ verdicts) {
  bool bad = false;
  for (int a = 0; a < 4; ++a) {
    if (!f.v[a]) continue;
    const double* vb = f.v[a] + size_t(blockIdx.x) * f.len[a];
    for (long long i = threadIdx.x; i < f.len[a]; i += blockDim.x) bad |= nonfinite(vb[i]);
  }
  const int any = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) verdicts[blockIdx.x] = any ? 1 : 0;
}

// every argument error of the shift, decided on the host before a device is touched (all host or all device pointers)
int shift_check(Engine& e, const ShiftArrays& a) {
  const std::string who = "shift_plan_batch: ";
  if (!a.dt) return step_fail(e, RPM_E_INVALID, who + "dt is NULL");
  if (!a.x) return step_fail(e, RPM_E_INVALID, who + "x is NULL");
  if (!a.x_out) return step_fail(e, RPM_E_INVALID, who + "x_out is NULL");
  if (!a.lambda != !a.lambda_out) return step_fail(e, RPM_E_INVALID, who + "lambda and lambda_out are given together or both NULL");
  if (!a.z_L != !a.z_U || !a.z_L != !a.z_L_out || !a.z_L != !a.z_U_out)
    return step_fail(e, RPM_E_INVALID, who + "z_L, z_U, z_L_out and z_U_out are given together or all NULL");
  const size_t B = size_t(e.n_instances), Bn = B * e.n * sizeof(double), Bm = B * e.m * sizeof(double);
  const ByteRange in[5] = {{"dt", a.dt, B * e.P * sizeof(double)}, {"x", a.x, Bn}, {"lambda", a.lambda, Bm}, {"z_L", a.z_L, Bn}, {"z_U", a.z_U, Bn}};
  const ByteRange out[4] = {{"x_out", a.x_out, Bn}, {"lambda_out", a.lambda_out, Bm}, {"z_L_out", a.z_L_out, Bn}, {"z_U_out", a.z_U_out, Bn}};
  if (const int rc = step_overlap(e, who, out, 4, in, 5)) return rc;
  if (sharded(e)) return step_fail(e, RPM_E_UNSUPPORTED, who + "not with interval sharding");
  if (!carry_fits(e, 0) || (a.lambda && !carry_fits(e, 1))) return step_no_fit(e, who, "knots", 1);
  return RPM_OK;
}

namespace {
// one launch per kind of array, then the verdicts over everything produced
int shift_launch(Engine& e, const ShiftArrays& a, int* d_nonfinite, hipStream_t st) {
  const CarryShift sh{a.dt, nullptr, e.P};
  int rc = carry_launch(e, e, a.x, a.x_out, nullptr, nullptr, nullptr, st, sh);
  if (rc == RPM_OK && a.lambda) rc = carry_launch(e, e, a.x, nullptr, a.lambda, a.lambda_out, nullptr, st, sh);
  if (rc == RPM_OK && a.z_L) rc = carry_launch(e, e, a.x, a.z_L_out, nullptr, nullptr, nullptr, st, CarryShift{a.dt, a.z_L, e.P});
  if (rc == RPM_OK && a.z_U) rc = carry_launch(e, e, a.x, a.z_U_out, nullptr, nullptr, nullptr, st, CarryShift{a.dt, a.z_U, e.P});
  if (rc || !d_nonfinite) return rc;
  const ShiftFlagged f{{a.x_out, a.lambda_out, a.z_L_out, a.z_U_out}, {e.n, e.m, e.n, e.n}};
  hipLaunchKernelGGL(rpm_shift_flag_kernel, dim3(unsigned(e.n_instances)), dim3(256), 0, st, f, d_nonfinite);
  return step_launched(e, "shift_plan_batch");
}
}  // namespace

// device-resident: at most four launches and the verdicts' on `stream`; after the first call on an engine nothing else
int dev_shift_plan_batch(Engine& e, const ShiftArrays& a, int* d_nonfinite, void* stream) {
  int rc = shift_check(e, a);
  if (rc) return rc;
  DeviceRestore restore;
  rc = dev_bind(e);
  if (rc) return rc;
  return shift_launch(e, a, d_nonfinite, static_cast<hipStream_t>(stream));
}

// the same through host arrays: everything up through the staging slots into one device block, the results back; blocking
int host_shift_plan_batch(Engine& e, const ShiftArrays& a, int* nonfinite) {
  int rc = shift_check(e, a);
  if (rc) return rc;
  DeviceRestore restore;
  rc = dev_bind(e);
  if (rc) return rc;
  const size_t B = size_t(e.n_instances), Bp = B * e.P, Bn = B * e.n, Bm = B * e.m;
  // the block: dt, x, lambda, z_L, z_U, then x_out, lambda_out, z_L_out, z_U_out
  const size_t o_x = Bp, o_lam = o_x + Bn, o_zl = o_lam + Bm, o_zu = o_zl + Bn, o_xo = o_zu + Bn, o_lo = o_xo + Bn, o_zlo = o_lo + Bm,
               o_zuo = o_zlo + Bn;
  return carry_state(*e.dev).shift.run(
      e, o_zuo + Bn,
      {{nullptr, 0, a.dt, Bp, STAGE_V}, {nullptr, o_x, a.x, Bn, STAGE_X}, {nullptr, o_lam, a.lambda, Bm, STAGE_LAMBDA},
       {nullptr, o_zl, a.z_L, Bn, STAGE_G}, {nullptr, o_zu, a.z_U, Bn, STAGE_GRAD}},
      [&](double* b, int* flags) {
        auto at = [&](const double* given, size_t off) { return given ? b + off : nullptr; };
        const ShiftArrays dv{b, b + o_x, b + o_xo, at(a.lambda, o_lam), at(a.lambda, o_lo), at(a.z_L, o_zl), at(a.z_L, o_zu),
                             at(a.z_L, o_zlo), at(a.z_L, o_zuo)};
        return shift_launch(e, dv, flags, e.dev->stream);
      },
      {{a.x_out, nullptr, o_xo, Bn, STAGE_X}, {a.lambda_out, nullptr, o_lo, Bm, STAGE_LAMBDA}, {a.z_L_out, nullptr, o_zlo, Bn, STAGE_G},
       {a.z_U_out, nullptr, o_zuo, Bn, STAGE_GRAD}},
      nonfinite);
}

// ---- the plans sampled at caller-given times: one phase's columns through rpm_sample_kernel ------------------------------

// every argument error of the sampler, decided on the host before a device is touched (all host or all device pointers)
int sample_check(Engine& e, int phase, const void* x, int n_times, const void* times, const void* out) {
  const std::string who = "sample_plan_batch: ";
  if (!x) return step_fail(e, RPM_E_INVALID, who + "x is NULL");
  if (!times) return step_fail(e, RPM_E_INVALID, who + "times is NULL");
  if (!out) return step_fail(e, RPM_E_INVALID, who + "out is NULL");
  if (n_times < 1) return step_fail(e, RPM_E_INVALID, who + "n_times must be at least 1");
  if (phase < 0 || phase >= e.P) return step_fail(e, RPM_E_INVALID, who + "the phase index is out of range");
  const PhaseHost& p = e.ph[size_t(phase)];
  const size_t B = size_t(e.n_instances), bytes_x = B * e.n * sizeof(double), bytes_t = B * size_t(n_times) * sizeof(double),
               bytes_o = bytes_t * size_t(p.nx + p.nu);
  const ByteRange o{"out", out, bytes_o}, in[2] = {{"x", x, bytes_x}, {"times", times, bytes_t}};
  if (const int rc = step_overlap(e, who, &o, 1, in, 2)) return rc;
  if (sharded(e)) return step_fail(e, RPM_E_UNSUPPORTED, who + "not with interval sharding");
  if (!carry_fits(e, 0)) return step_no_fit(e, who, "knots", 1);
  return RPM_OK;
}

namespace {
int sample_launch(Engine& e, int phase, const double* d_x, int n_times, const double* d_times, double* d_out, int* d_nonfinite,
                  hipStream_t st) {
  const CarryPlan* plan = nullptr;
  const int rc = carry_plan_for(e, e, 0, "sample_plan_batch", &plan);
  if (rc) return rc;
  Device& d = *e.dev;
  const PhaseHost& p = e.ph[size_t(phase)];
  const int B = e.n_instances, g0 = plan->group0[size_t(phase)], ng = plan->group0[size_t(phase) + 1] - g0;
  hipLaunchKernelGGL(rpm_sample_kernel, dim3(unsigned(ng), unsigned((B + plan->TB - 1) / plan->TB)), dim3(256), plan->lds, st, d.d_phases,
                     d.d_points, e.n, plan->d_groups + g0, B, plan->TB, d_x, n_times, d_times, d_out);
  if (d_nonfinite) flag_launch((long long)(p.nx + p.nu) * n_times, d_out, d_nonfinite, B, st);
  return step_launched(e, "sample_plan_batch");
}
}  // namespace

// device-resident: one launch (two with the verdicts) on `stream`; after the first call on an engine nothing else
int dev_sample_plan_batch(Engine& e, int phase, const double* d_x, int n_times, const double* d_times, double* d_out, int* d_nonfinite,
                          void* stream) {
  int rc = sample_check(e, phase, d_x, n_times, d_times, d_out);
  if (rc) return rc;
  DeviceRestore restore;
  rc = dev_bind(e);
  if (rc) return rc;
  return sample_launch(e, phase, d_x, n_times, d_times, d_out, d_nonfinite, static_cast<hipStream_t>(stream));
}

// the same through host arrays: x and the times up through the staging slots, the samples and the verdicts back; blocking
int host_sample_plan_batch(Engine& e, int phase, const double* x, int n_times, const double* times, double* out, int* nonfinite) {
  int rc = sample_check(e, phase, x, n_times, times, out);
  if (rc) return rc;
  DeviceRestore restore;
  rc = dev_bind(e);
  if (rc) return rc;
  Device& d = *e.dev;
  const PhaseHost& p = e.ph[size_t(phase)];
  const size_t B = size_t(e.n_instances), Bt = B * size_t(n_times), Bo = Bt * size_t(p.nx + p.nu);   // the block: the times, the samples
  return carry_state(d).sample.run(
      e, Bt + Bo, {{d.d_x, 0, x, B * e.n, STAGE_X}, {nullptr, 0, times, Bt, STAGE_V}},
      [&](double* b, int* flags) { return sample_launch(e, phase, d.d_x, n_times, b, b + Bt, flags, d.stream); },
      {{out, nullptr, Bt, Bo, STAGE_G}}, nonfinite);
}

// the row map of the multiplier carry on the host: phase < P: {first defect row, first path row, first event row, one past the
// phase's last row}; phase == P: the rows after the phases, {first, first, first, m}
int carry_multipliers_layout(const Engine& e, int phase, int rows[4]) {
  if (phase < 0 || phase > e.P) return RPM_E_INVALID;
  if (phase == e.P) {
    const int t0 = e.P > 0 ? carry_rows(e, e.P - 1).end : 0;
    rows[0] = rows[1] = rows[2] = t0;
    rows[3] = e.m;
    return RPM_OK;
  }
  const CarryRows r = carry_rows(e, phase);
  rows[0] = r.defect0; rows[1] = r.path0; rows[2] = r.event0; rows[3] = r.end;
  return RPM_OK;
}

}  // namespace rpm
