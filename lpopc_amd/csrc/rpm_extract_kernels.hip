// rpm_extract_kernels.hip — solution extraction for a whole sweep: Nlp2OpConverter::Nlp2OpControl (Core/Nlp2OPConverter.cpp:13-196)
// for every phase and every instance of an engine in one launch (two with the NaN/Inf verdicts), nothing but the caller's arrays
// crossing the call.  The specification is the one-instance route of rpm_post_kernels.hip (rpm_post_spline_kernel + rpm_post_kernel +
// rpm_post_cost_kernel): per instance b the kernels below apply that route's rules (rpm_post_device.hpp, the one copy both
// routes call) to x + b * n and lambda + b * m, with the user functions reading instance b's constants and static parameters.
//
// One instance's block of EB doubles holds the phases one after the other, each phase time (M), state (M nx), control (M nu),
// costate (M nx), pathmult (M nc), hamiltonian (M), mayer_cost (1), lagrange_cost (1), M = N + 1, every array column-major with
// M rows: the arrays rpm_nlp2op_control returns.
#include "rpm_post_device.hpp"

namespace rpm {

// One workgroup's share of rpm_extract_spline_kernel: spline columns [col0, col0 + ncols) of a phase, the nu controls first,
// then the nc path-multiplier columns.
struct ExtractGroup {
  int phase, col0, ncols;
};

// Dynamic LDS of the two kernels, offsets in doubles.  Rows are Np = N | 1 doubles apart, so the lanes that walk different rows
// in step sit on different banks (rpm_carry_kernels.hip, CarryLds).  rpm_extract_kernel: red_rows = TB, and when it also runs
// the splines (fused) lag_rows = TB and ncols = nu + nc, else both 0; rpm_extract_spline_kernel: red_rows = lag_rows = 0.
struct ExtractLds {
  int Np;
  int red;     // [red_rows][256]      partial sums of lagrange_cost
  int lag;     // [lag_rows][Np]       the Lagrangian at the nodes of every instance
  int pts;     // [Np]                 the phase's LGR points    (ncols > 0)
  int w;       // [Np]                 its weights               (ncols > 0)
  int cols;    // [TB * ncols][Np]     the spline columns, row = instance * ncols + column
  int ends;    // [TB * ncols]         their values at tau = 1
  int total;
  __host__ __device__ constexpr ExtractLds(int N, int TB, int ncols, int red_rows, int lag_rows)
      : Np(N | 1), red(0), lag(red_rows * 256), pts(lag + lag_rows * Np), w(pts + (ncols > 0 ? Np : 0)), cols(w + (ncols > 0 ? Np : 0)),
        ends(cols + TB * ncols * Np), total(ends + TB * ncols) {}
  __host__ __device__ constexpr int staged() const { return total - lag; }   // all but the partial sums: what the planner's LDS budget counts
};
static_assert(ExtractLds(64, 8, 4, 8, 8).Np == 65 && ExtractLds(64, 8, 4, 8, 8).total == 8 * 256 + 65 * (8 + 2 + 32) + 32 &&
                  ExtractLds(64, 8, 0, 8, 0).total == 8 * 256 && ExtractLds(65, 2, 3, 0, 0).total == 65 * (2 + 6) + 6,
              "ExtractLds: an array overlaps its neighbour or the total changed");

__host__ __device__ inline long long extract_phase_doubles(int N, int nx, int nu, int nc) {
  return (long long)(N + 1) * (2 + 2 * nx + nu + nc) + 2;
}

// The values at tau = 1 of spline columns [col0, col0 + ncols) of phase `ph` for instances b0 .. b0 + nb: the columns are staged
// with k-fastest loads, then one lane per (instance, column) runs post_spline_end out of LDS.  ends[bi * ncols + cl].  A
// path-multiplier column j reads lambda WITHOUT the phase offset, lam[N * nx + j * N + k] from the base of the instance's own
// block (Nlp2OPConverter.cpp:88), and is scaled inside the accessor, 2 ((1 / w_k) lambda) / (tf - t0) (:92), as
// rpm_post_spline_kernel does it.  The caller synchronises before it reads `ends`.
__device__ __forceinline__ void extract_spline_ends(const KParams& K, const PhaseDev& ph, int col0, int ncols, int b0, int nb,
                                                    const double* __restrict__ x, const double* __restrict__ lam, double* pts,
                                                    double* w, double* cols, int Np, double* ends) {
  const int N = ph.N, nu = ph.nu, tid = threadIdx.x, nt = blockDim.x;
  for (int k = tid; k < N; k += nt) {
    pts[k] = K.points[ph.node0 + k];
    w[k] = K.weights[ph.node0 + k];
  }
  for (int idx = tid; idx < nb * ncols * N; idx += nt) {
    const int k = idx % N, cl = (idx / N) % ncols, bi = idx / (N * ncols);
    const int col = col0 + cl;
    const double* src = col < nu ? x + size_t(b0 + bi) * K.n + ph.x_control0 + col * N
                                 : lam + size_t(b0 + bi) * K.m + N * ph.nx + (col - nu) * N;
    cols[(bi * ncols + cl) * Np + k] = src[k];
  }
  __syncthreads();
  for (int r = tid; r < nb * ncols; r += nt) {
    const int bi = r / ncols, col = col0 + r % ncols;
    const double* y = cols + r * Np;
    if (col < nu) {
      ends[r] = post_spline_end(N, pts, [&](int k) -> double { return y[k]; });
    } else {
      const double* xb = x + size_t(b0 + bi) * K.n;
      const double tspan = xb[ph.x_t0 + 1] - xb[ph.x_t0];
      ends[r] = post_spline_end(N, pts, [&](int k) -> double { return 2.0 * ((1 / w[k]) * y[k]) / tspan; });
    }
  }
}

// Only when a phase's columns do not fit one workgroup's LDS next to the node part: workgroup (group of columns, tile of TB
// instances), the values at tau = 1 into the workspace, ends_ws[b * ET + phase * ecols + column].
__global__ void __launch_bounds__(256)
rpm_extract_spline_kernel(const KParams K, const ExtractGroup* __restrict__ groups, int B, int TB, const double* __restrict__ x,
                          const double* __restrict__ lam, double* __restrict__ ends_ws, int ET, int ecols) {
  extern __shared__ __align__(16) double extract_ssm[];
  const ExtractGroup v = groups[blockIdx.x];
  const PhaseDev ph = K.phases[v.phase];
  const ExtractLds L(ph.N, TB, v.ncols, 0, 0);
  const int b0 = blockIdx.y * TB;
  const int nb = B - b0 < TB ? B - b0 : TB;
  extract_spline_ends(K, ph, v.col0, v.ncols, b0, nb, x, lam, extract_ssm + L.pts, extract_ssm + L.w, extract_ssm + L.cols, L.Np,
                      extract_ssm + L.ends);
  __syncthreads();
  for (int r = threadIdx.x; r < nb * v.ncols; r += blockDim.x)
    ends_ws[size_t(b0 + r / v.ncols) * ET + v.phase * ecols + v.col0 + r % v.ncols] = extract_ssm[L.ends + r];
}

// Workgroup (phase, tile of TB instances), 256 threads.  Items run k-fastest inside an instance: the lanes that share an instance
// read every x / lambda column and store every output column as a contiguous run.  `fused`: the workgroup runs the phase's splines
// itself and keeps their end values and the Lagrangian in LDS; otherwise the end values come from rpm_extract_spline_kernel and
// the Lagrangian goes through the workspace lag_ws[b * NT + node] (written and read by this workgroup only).
template <class Prob>
__global__ void __launch_bounds__(256)
rpm_extract_kernel(const KParams K, int B, int TB, int fused, long long EB, const double* __restrict__ x,
                   const double* __restrict__ lam, const double* ends_ws, int ET, int ecols, double* lag_ws, int NT,
                   double* __restrict__ out) {
  constexpr int NX = Prob::NX, NU = Prob::NU, NC = Prob::NC;
  constexpr int NXs = NX > 0 ? NX : 1;
  extern __shared__ __align__(16) double extract_sm[];
  const int p = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const PhaseDev ph = K.phases[p];
  const int N = ph.N, M = N + 1, ncols = ph.nu + ph.nc;   // what the host planner sized the launch by
  const int b0 = blockIdx.y * TB;
  const int nb = B - b0 < TB ? B - b0 : TB;
  long long base = 0;   // the phase's offset inside an instance's block
  for (int q = 0; q < p; ++q) base += extract_phase_doubles(K.phases[q].N, K.phases[q].nx, K.phases[q].nu, K.phases[q].nc);
  const ExtractLds L(N, TB, fused ? ncols : 0, TB, fused ? TB : 0);
  double* red = extract_sm + L.red;
  if (fused && ncols > 0)
    extract_spline_ends(K, ph, 0, ncols, b0, nb, x, lam, extract_sm + L.pts, extract_sm + L.w, extract_sm + L.cols, L.Np,
                        extract_sm + L.ends);
  // ---- end-point costates (post_end_costate).  One lane per (instance, state), taken from the top of the workgroup so that
  // they run beside the spline lanes instead of behind them; inside the node loop the one lane of k = N would walk nx chains
  // of dependent loads.  Parked in `red`, which the cost reduction needs only after the node loop.
  static_assert(NX <= 256, "the end-point costates of an instance are parked in its 256 partial sums");
  for (int idx = nt - 1 - tid; idx < nb * NX; idx += nt) {
    const int s = idx % NXs, bi = idx / NXs;
    red[bi * 256 + s] = post_end_costate(K, ph, lam + size_t(b0 + bi) * K.m + ph.g0, s);
  }
  __syncthreads();
  const long long o_state = M, o_control = o_state + (long long)M * NX, o_costate = o_control + (long long)M * NU,
                  o_pathmult = o_costate + (long long)M * NX, o_ham = o_pathmult + (long long)M * NC, o_mayer = o_ham + M;

  // ---- per node: post_node, the end-point costate coming from above --------------------------------------------
  for (int idx = tid; idx < nb * M; idx += nt) {
    const int k = idx % M, bi = idx / M;
    const size_t b = size_t(b0 + bi);
    const double* u_end = fused ? extract_sm + L.ends + bi * ncols : ends_ws + b * ET + p * ecols;
    double* lag = fused ? extract_sm + L.lag + bi * L.Np : lag_ws + b * NT + ph.node0;
    double* ob = out + b * EB + base;
    post_node<Prob>(K, ph, k, x + b * K.n, lam + b * K.m, K.consts + b * K.consts_stride, u_end, u_end + NU,
                    [&](int s) { return red[bi * 256 + s]; },
                    PostOut{ob, ob + o_state, ob + o_control, ob + o_costate, ob + o_pathmult, ob + o_ham, ob + o_mayer},
                    k < N ? lag + k : nullptr);
  }
  __syncthreads();

  // ---- lagrange_cost per instance: post_cost_partial, the halving tree over every instance's 256 partial sums, post_cost_scaled
  for (int idx = tid; idx < nb * 256; idx += nt) {
    const int t = idx & 255, bi = idx >> 8;
    const double* lag = fused ? extract_sm + L.lag + bi * L.Np : lag_ws + size_t(b0 + bi) * NT + ph.node0;
    red[idx] = post_cost_partial(N, K.weights + ph.node0, lag, t);
  }
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    for (int idx = tid; idx < nb * st; idx += nt) {
      const int t = idx % st, bi = idx / st;
      red[bi * 256 + t] += red[bi * 256 + t + st];
    }
    __syncthreads();
  }
  for (int bi = tid; bi < nb; bi += nt) {
    const size_t b = size_t(b0 + bi);
    const double* xb = x + b * K.n;
    out[b * EB + base + o_mayer + 1] = post_cost_scaled(xb[ph.x_t0], xb[ph.x_t0 + 1], red[bi * 256]);
  }
}

namespace {

constexpr int kExtractAutoTile = 1;               // the fastest of 1, 2, 4, 8 in profiles/sweep_extract.json (tools/bench_sweep_extract.py)

struct ExtractPlan {
  int tile_opt = 0, lds_opt = 0;   // the options the plan was made under
  int TB = 1, fused = 1, n_groups = 0;
  size_t lds_node = 0, lds_spline = 0;
  ExtractGroup* d_groups = nullptr;
};
struct ExtractState {
  std::vector<ExtractPlan> plans;
  double *ends_ws = nullptr, *lag_ws = nullptr;   // the split plans' workspace
  HostForm host;   // host-pointer form: the instances' blocks
};

// doubles the staged arrays of one workgroup may take: what the device offers less the partial sums of the largest tile, or
// the option when that is smaller
size_t extract_budget(const Engine& e) {
  return lds_budget(e.opt_extract_lds, kCuLdsBytes - 8 * 256 * sizeof(double)) / sizeof(double);
}

// Host planner.  Fused (one launch): every phase's spline columns fit one workgroup's LDS next to the Lagrangian rows; the
// tile is halved before that is given up.  Otherwise the columns are dealt over the workgroups of a spline launch of their own,
// again halving the tile first, and only a single column that does not fit is refused.
bool extract_plan(const Engine& e, ExtractPlan* plan, std::vector<ExtractGroup>* groups) {
  const size_t budget = extract_budget(e);
  const int TB0 = clamp_tile(e.opt_extract_tile > 0 ? e.opt_extract_tile : kExtractAutoTile, e.n_instances);
  ExtractPlan pl;
  pl.tile_opt = e.opt_extract_tile;
  pl.lds_opt = e.opt_extract_lds;
  if (groups) groups->clear();
  auto all_fit = [&](auto fits) { return std::all_of(e.ph.begin(), e.ph.end(), fits); };
  pl.TB = halve_tile(TB0, [&](int TB) {
    return all_fit([&](const PhaseHost& p) { return size_t(ExtractLds(p.N, TB, p.nu + p.nc, TB, TB).staged()) <= budget; });
  });
  if (pl.TB) {
    pl.fused = 1;
    for (const PhaseHost& p : e.ph) pl.lds_node = std::max(pl.lds_node, size_t(ExtractLds(p.N, pl.TB, p.nu + p.nc, pl.TB, pl.TB).total) * sizeof(double));
    *plan = pl;
    return true;
  }
  auto fits = [&](const PhaseHost& p, int TB, int ncols) { return size_t(ExtractLds(p.N, TB, ncols, 0, 0).total) <= budget; };
  pl.TB = halve_tile(TB0, [&](int TB) { return all_fit([&](const PhaseHost& p) { return p.nu + p.nc == 0 || fits(p, TB, 1); }); });
  if (!pl.TB) return false;
  pl.fused = 0;
  pl.lds_node = size_t(ExtractLds(1, pl.TB, 0, pl.TB, 0).total) * sizeof(double);
  for (size_t ip = 0; ip < e.ph.size(); ++ip) {
    const PhaseHost& p = e.ph[ip];
    if (p.nu + p.nc == 0) continue;   // no spline columns: no workgroup of the spline launch
    for (const auto& [col0, ncols] : split_columns(p.nu + p.nc, [&](int nc) { return fits(p, pl.TB, nc); })) {
      pl.lds_spline = std::max(pl.lds_spline, size_t(ExtractLds(p.N, pl.TB, ncols, 0, 0).total) * sizeof(double));
      ++pl.n_groups;
      if (groups) groups->push_back(ExtractGroup{int(ip), col0, ncols});
    }
  }
  *plan = pl;
  return true;
}

int extract_ecols(const Engine& e) {
  int c = 0;
  for (const PhaseHost& p : e.ph) c = std::max(c, p.nu + p.nc);
  return c;
}
int extract_nodes(const Engine& e) {
  int n = 0;
  for (const PhaseHost& p : e.ph) n += p.N;
  return n;
}

ExtractState& extract_state(Device& d) {
  if (!d.extract) d.extract = new ExtractState();
  return *static_cast<ExtractState*>(d.extract);
}

int extract_launch(Engine& e, const double* d_x, const double* d_lambda, double* d_out, int* d_nonfinite, hipStream_t st) {
  Device& d = *e.dev;
  ExtractState& es = extract_state(d);
  const ExtractPlan* plan = nullptr;
  for (const ExtractPlan& p : es.plans)
    if (p.tile_opt == e.opt_extract_tile && p.lds_opt == e.opt_extract_lds) plan = &p;
  const size_t B = size_t(e.n_instances);
  const int ET = e.P * extract_ecols(e), NT = extract_nodes(e);
  if (!plan) {   // first call under these options: the only allocations and the only blocking copy
    ExtractPlan p;
    std::vector<ExtractGroup> groups;
    if (!extract_plan(e, &p, &groups)) return step_fail(e, RPM_E_UNSUPPORTED, "nlp2op_batch: a column does not fit one workgroup's LDS");
    if (!p.fused) {
      HIP_TRY(e, upload(&p.d_groups, groups));
      if (!es.ends_ws) {
        HIP_TRY(e, hipMalloc(reinterpret_cast<void**>(&es.ends_ws), std::max<size_t>(B * ET, 1) * sizeof(double)));
        HIP_TRY(e, hipMalloc(reinterpret_cast<void**>(&es.lag_ws), std::max<size_t>(B * NT, 1) * sizeof(double)));
      }
    }
    hipError_t s = hipSuccess;
    with_problem(e.problem_id, [&](auto prob) {
      using P = decltype(prob);
      s = raise_dynamic_lds(reinterpret_cast<const void*>(rpm_extract_kernel<P>), p.lds_node);
    });
    if (s == hipSuccess) s = raise_dynamic_lds(reinterpret_cast<const void*>(rpm_extract_spline_kernel), p.lds_spline);
    HIP_TRY(e, s);
    es.plans.push_back(p);
    plan = &es.plans.back();
  }
  long long EB = 0;
  nlp2op_batch_layout(e, 0, nullptr, &EB);
  const int Bi = e.n_instances, TB = plan->TB;
  const unsigned tiles = unsigned((Bi + TB - 1) / TB);
  if (!plan->fused && plan->n_groups > 0)
    hipLaunchKernelGGL(rpm_extract_spline_kernel, dim3(unsigned(plan->n_groups), tiles), dim3(256), plan->lds_spline, st, d.kp,
                       plan->d_groups, Bi, TB, d_x, d_lambda, es.ends_ws, ET, extract_ecols(e));
  const bool known = with_problem(e.problem_id, [&](auto prob) {
    using P = decltype(prob);
    hipLaunchKernelGGL((rpm_extract_kernel<P>), dim3(unsigned(e.P), tiles), dim3(256), plan->lds_node, st, d.kp, Bi, TB, plan->fused,
                       EB, d_x, d_lambda, es.ends_ws, ET, extract_ecols(e), es.lag_ws, NT, d_out);
  });
  if (!known) return step_no_kernels(e, "nlp2op_batch");
  if (d_nonfinite) flag_launch(EB, d_out, d_nonfinite, Bi, st);
  return step_launched(e, "nlp2op_batch");
}

}  // namespace

void extract_destroy(Device* d) {
  ExtractState* es = static_cast<ExtractState*>(d->extract);
  if (!es) return;
  for (ExtractPlan& p : es->plans)
    if (p.d_groups) (void)hipFree(p.d_groups);
  for (double* p : {es->ends_ws, es->lag_ws})
    if (p) (void)hipFree(p);
  es->host.release();
  delete es;
  d->extract = nullptr;
}

// host only: the offsets of a phase's eight fields inside an instance's block, and the block's length
void nlp2op_batch_layout(const Engine& e, int phase, long long field_offset[8], long long* block_doubles) {
  long long off = 0;
  for (int ip = 0; ip < e.P; ++ip) {
    const PhaseHost& p = e.ph[size_t(ip)];
    const long long M = p.N + 1;
    if (ip == phase && field_offset) {
      const long long len[8] = {M, M * p.nx, M * p.nu, M * p.nx, M * p.nc, M, 1, 1};
      long long o = off;
      for (int f = 0; f < 8; ++f) {
        field_offset[f] = o;
        o += len[f];
      }
    }
    off += extract_phase_doubles(p.N, p.nx, p.nu, p.nc);
  }
  if (block_doubles) *block_doubles = off;
}

// workgroups per tile of instances of the spline launch under the engine's options: 0 when the extraction is one fused launch,
// -1 when a column does not fit
int extract_group_count(const Engine& e) {
  ExtractPlan p;
  if (!extract_plan(e, &p, nullptr)) return -1;
  return p.fused ? 0 : p.n_groups;
}

// every error of the engine's state, decided on the host before a device is touched
int extract_check(Engine& e) {
  const std::string who = "nlp2op_batch: ";
  if (sharded(e)) return step_fail(e, RPM_E_UNSUPPORTED, who + "not with interval sharding");
  for (const PhaseHost& p : e.ph)   // the path multipliers' unshifted index stays inside the instance's own lambda block
    if ((long long)p.N * (p.nx + p.nc) > e.m) return step_fail(e, RPM_E_UNSUPPORTED, who + "a phase's path multipliers would be read past the instance's multipliers");
  ExtractPlan p;
  if (!extract_plan(e, &p, nullptr)) return step_no_fit(e, who, "nodes", 0);
  return RPM_OK;
}

// device-resident: one launch (the spline launch before it when the columns are dealt, the verdicts' after it) on `stream`; after
// the first call on an engine nothing else
int dev_nlp2op_batch(Engine& e, const double* d_x, const double* d_lambda, double* d_out, int* d_nonfinite, void* stream) {
  int rc = extract_check(e);
  if (rc) return rc;
  DeviceRestore restore;
  rc = dev_bind(e);
  if (rc) return rc;
  return extract_launch(e, d_x, d_lambda, d_out, d_nonfinite, static_cast<hipStream_t>(stream));
}

// the same through host arrays: x and lambda up through the staging slots, the blocks and the verdicts back; blocking
int host_nlp2op_batch(Engine& e, const double* x, const double* lambda, double* out, int* nonfinite) {
  int rc = extract_check(e);
  if (rc) return rc;
  DeviceRestore restore;
  rc = dev_bind(e);
  if (rc) return rc;
  Device& d = *e.dev;
  const size_t B = size_t(e.n_instances);
  long long EB = 0;
  nlp2op_batch_layout(e, 0, nullptr, &EB);
  return extract_state(d).host.run(
      e, B * size_t(EB), {{d.d_x, 0, x, B * e.n, STAGE_X}, {d.d_lambda, 0, lambda, B * e.m, STAGE_LAMBDA}},
      [&](double* blocks, int* flags) { return extract_launch(e, d.d_x, d.d_lambda, blocks, flags, d.stream); },
      {{out, nullptr, 0, B * size_t(EB), STAGE_G}}, nonfinite);
}

}  // namespace rpm
