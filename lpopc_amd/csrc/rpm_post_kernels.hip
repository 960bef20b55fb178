// rpm_post_kernels.hip — the steps after the NLP solve: solution extraction (Nlp2OpConverter) for one instance and the
// mesh-error estimate (SolutionErrorChecker) for one instance and for a whole sweep, kernels and host drivers.  Once per mesh,
// not on the metric.  The kernels here choose the work split; the rules they apply are in rpm_post_device.hpp, one copy each.
#include "rpm_post_device.hpp"

namespace rpm {

// ------------------------------------------------------------------------------------------
// Mesh-error estimate: SolutionErrorChecker::CheckSolutionDiffError, Core/LpSolutionError.cpp:112-169.
// One workgroup per mesh interval.  Phase A interpolates the interval's states / controls onto its (n+1)-point LGR
// mesh (SolutionInterpolation, :46-108, rows of the tables built in rpm_mesh.cpp), phase B evaluates the dynamics
// there, phase C integrates them with the interval's integration matrix: X(start) + A f (:147).
template <class Prob>
__global__ void rpm_mesh_err_kernel(const KParams K, int phase, const double* __restrict__ x,
                                    const MeshIvDev* __restrict__ ivs, int n_iv, const double* __restrict__ Hs,
                                    const double* __restrict__ Ss, const int* __restrict__ hit_s,
                                    const double* __restrict__ Hc, const double* __restrict__ Sc,
                                    const int* __restrict__ hit_c, const double* __restrict__ A,
                                    const double* __restrict__ ttem, int rows, double* __restrict__ fine_state,
                                    double* __restrict__ integ) {
  constexpr int NX = Prob::NX, NU = Prob::NU;
  extern __shared__ double mesh_sm[];
  const MeshIvDev v = ivs[blockIdx.x];
  const int n = v.n, n1 = n + 1;
  double* Xs = mesh_sm;            // [q * NX + s]
  double* Us = Xs + n1 * NX;       // [q * NU + j]
  double* Fs = Us + n1 * NU;       // [q * NX + s]
  const PhaseDev ph = K.phases[phase];
  const int N = ph.N, M = N + 1;
  const double t0 = x[ph.x_t0];
  const double tf = post_time(t0, x[ph.x_t0 + 1], 1.0);   // result->time's last entry
  for (int idx = threadIdx.x; idx < n1 * NX; idx += blockDim.x) {
    const int q = idx % n1, s = idx / n1;
    const double val = mesh_interp(hit_s[v.q0 + q], Hs + v.hs + q, n1, n1, x + ph.x_state0 + s * M + v.istart, Ss + v.q0 + q);
    Xs[q * NX + s] = val;
    fine_state[(v.r0 + q) + size_t(s) * rows] = val;
  }
  for (int idx = threadIdx.x; idx < n1 * NU; idx += blockDim.x) {
    const int q = idx % n1, j = idx / n1;
    Us[q * NU + j] = mesh_interp(hit_c[v.q0 + q], Hc + v.hc + q, n1, n, x + ph.x_control0 + j * N + v.istart, Sc + v.q0 + q);
  }
  __syncthreads();
  for (int q = threadIdx.x; q < n1; q += blockDim.x)
    mesh_dynamics<Prob>(ph, t0, tf, ttem[v.q0 + q], Xs + q * NX, Us + q * NU, x + ph.x_t0 + 2, K.consts, Fs + q * NX);
  __syncthreads();
  for (int idx = threadIdx.x; idx < n1 * NX; idx += blockDim.x) {
    const int r = idx % n1, s = idx / n1;
    integ[(1 + v.r0 + r) + size_t(s) * rows] = mesh_integrate(A + v.a + r, n1, Fs, NX, s, Xs);
  }
  if (blockIdx.x == 0)
    for (int s = threadIdx.x; s < NX; s += blockDim.x) integ[size_t(s) * rows] = Xs[s];
  if (blockIdx.x == n_iv - 1)
    for (int s = threadIdx.x; s < NX; s += blockDim.x)
      fine_state[(rows - 1) + size_t(s) * rows] = x[ph.x_state0 + s * M + N];
}

// relative_error(:, s), one workgroup per state: the column's maximum, then mesh_rel_entry
__global__ void rpm_mesh_rel_kernel(int rows, const double* __restrict__ fine_state, const double* __restrict__ integ,
                                    double* __restrict__ rel) {
  __shared__ double red[256];
  const double* col = fine_state + size_t(blockIdx.x) * rows;
  double mx = col[0];
  for (int r = threadIdx.x; r < rows; r += blockDim.x) mx = fmax(mx, col[r]);
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  const double den = 1 + red[0];
  for (int r = threadIdx.x; r < rows; r += blockDim.x)
    rel[r + size_t(blockIdx.x) * rows] = mesh_rel_entry(integ[r + size_t(blockIdx.x) * rows], col[r], den);
}

// ------------------------------------------------------------------------------------------
// Solution extraction: Nlp2OpConverter::Nlp2OpControl, Core/Nlp2OPConverter.cpp:13-196.
// Runs once per mesh after the NLP solve, not per iteration.
// rpm_post_spline_kernel: value at tau = +1 of the natural cubic spline through (tau_k, y_k), one thread per column
// (LpGuessChecker::spline_interpolation, Core/LpGuessChecker.cpp:208-270, specialised to the last interval: only the
// forward recurrence's final z is needed because c[n-1] = 0).
__global__ void rpm_post_spline_kernel(int N, const double* __restrict__ tau, const double* __restrict__ cols, int ncols,
                                       double scale_num, double scale_den, const double* __restrict__ w,
                                       double* __restrict__ out) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= ncols) return;
  const double* y = cols + size_t(col) * N;
  // optional scaling y_k -> scale_num * (1/w_k) * y_k / scale_den  (path multipliers, Nlp2OPConverter.cpp:92)
  auto Y = [&](int k) -> double { return w ? scale_num * ((1 / w[k]) * y[k]) / scale_den : y[k]; };
  out[col] = post_spline_end(N, tau, Y);
}

template <class Prob>
__global__ void rpm_post_kernel(const KParams K, int phase, const double* __restrict__ x, const double* __restrict__ lam,
                                const double* __restrict__ u_end, const double* __restrict__ pm_end,
                                double* __restrict__ o_time, double* __restrict__ o_state, double* __restrict__ o_control,
                                double* __restrict__ o_costate, double* __restrict__ o_pathmult,
                                double* __restrict__ o_ham, double* __restrict__ o_lag, double* __restrict__ o_mayer) {
  const PhaseDev ph = K.phases[phase];
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > ph.N) return;
  const double* lp = lam + ph.g0;
  post_node<Prob>(K, ph, k, x, lam, K.consts, u_end, pm_end, [&](int s) { return post_end_costate(K, ph, lp, s); },
                  PostOut{o_time, o_state, o_control, o_costate, o_pathmult, o_ham, o_mayer}, o_lag + k);
}

// lagrange_cost of one instance: post_cost_partial, the halving tree, post_cost_scaled
__global__ void rpm_post_cost_kernel(const KParams K, int phase, const double* __restrict__ x,
                                     const double* __restrict__ lag, double* __restrict__ out) {
  __shared__ double red[256];
  const PhaseDev ph = K.phases[phase];
  const int tid = threadIdx.x;
  red[tid] = post_cost_partial(ph.N, K.weights + ph.node0, lag, tid);
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  if (tid == 0) out[0] = post_cost_scaled(x[ph.x_t0], x[ph.x_t0 + 1], red[0]);
}

// nonfinite[b] = 1 when block b of `len` doubles holds a NaN or Inf, else 0: one workgroup per block, a block-wide OR, no atomics
__global__ void __launch_bounds__(256) rpm_flag_kernel(long long len, const double* __restrict__ v, int* __restrict__ verdicts) {
  const double* vb = v + size_t(blockIdx.x) * len;
  bool bad = false;
  for (long long i = threadIdx.x; i < len; i += blockDim.x) bad |= nonfinite(vb[i]);
  const int any = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) verdicts[blockIdx.x] = any ? 1 : 0;
}
void flag_launch(long long len, const double* v, int* nonfinite, int B, hipStream_t stream) {
  hipLaunchKernelGGL(rpm_flag_kernel, dim3(unsigned(B)), dim3(256), 0, stream, len, v, nonfinite);
}

// Nlp2OpControl for one phase: host x / lambda in, (N+1)-row column-major host arrays out (any may be NULL)
int dev_nlp2op(Engine& e, int phase, const double* x, const double* lambda, double* time, double* state, double* control,
               double* costate, double* pathmult, double* hamiltonian, double* mayer_cost, double* lagrange_cost) {
  int rc = dev_bind(e);
  if (rc) return rc;
  Device& d = *e.dev;
  const PhaseHost& p = e.ph[phase];
  const int N = p.N, M = N + 1, nx = p.nx, nu = p.nu, nc = p.nc;
  const size_t out_doubles = size_t(M) * (3 + 2 * nx + nu + nc) + 8 + nu + nc;
  double* buf = nullptr;
  HIP_TRY(e, hipMalloc(reinterpret_cast<void**>(&buf), out_doubles * sizeof(double)));
  double* o_time = buf;
  double* o_state = o_time + M;
  double* o_control = o_state + size_t(M) * nx;
  double* o_costate = o_control + size_t(M) * nu;
  double* o_pathmult = o_costate + size_t(M) * nx;
  double* o_ham = o_pathmult + size_t(M) * nc;
  double* o_lag = o_ham + M;
  double* o_scal = o_lag + M;          // [0] mayer, [1] lagrange cost
  double* u_end = o_scal + 8;
  double* pm_end = u_end + nu;
  rc = dev_upload(e, d.d_x, x, size_t(e.n), STAGE_X);
  if (rc == RPM_OK) rc = dev_upload(e, d.d_lambda, lambda, size_t(e.m), STAGE_LAMBDA);
  hipError_t s = hipSuccess;
  if (rc == RPM_OK) {
    hipStream_t st = d.stream;
    const PhaseDev& q = e.phd[phase];
    const double tspan = x[q.x_t0 + 1] - x[q.x_t0];
    if (nu > 0)
      hipLaunchKernelGGL(rpm_post_spline_kernel, dim3(1), dim3(64), 0, st, N, d.d_points + q.node0, d.d_x + q.x_control0, nu,
                         1.0, 1.0, static_cast<const double*>(nullptr), u_end);
    if (nc > 0)
      hipLaunchKernelGGL(rpm_post_spline_kernel, dim3(1), dim3(64), 0, st, N, d.d_points + q.node0,
                         d.d_lambda + size_t(N) * nx, nc, 2.0, tspan, d.d_weights + q.node0, pm_end);
    with_problem(e.problem_id, [&](auto prob) {
      using P = decltype(prob);
      hipLaunchKernelGGL((rpm_post_kernel<P>), dim3(unsigned((M + 255) / 256)), dim3(256), 0, st, d.kp, phase, d.d_x, d.d_lambda,
                         u_end, pm_end, o_time, o_state, o_control, o_costate, o_pathmult, o_ham, o_lag, o_scal);
    });
    hipLaunchKernelGGL(rpm_post_cost_kernel, dim3(1), dim3(256), 0, st, d.kp, phase, d.d_x, o_lag, o_scal + 1);
    s = hipGetLastError();
    if (s == hipSuccess) s = hipStreamSynchronize(st);
    auto get = [&](double* host, const double* dev, size_t cnt) {   // caller arrays: through the staging slot
      if (host && cnt && s == hipSuccess && rc == RPM_OK) rc = dev_download(e, host, dev, cnt, STAGE_HESS);
    };
    get(time, o_time, M);
    get(state, o_state, size_t(M) * nx);
    get(control, o_control, size_t(M) * nu);
    get(costate, o_costate, size_t(M) * nx);
    get(pathmult, o_pathmult, size_t(M) * nc);
    get(hamiltonian, o_ham, M);
    get(mayer_cost, o_scal, 1);
    get(lagrange_cost, o_scal + 1, 1);
  }
  (void)hipFree(buf);
  if (rc) return rc;
  if (s != hipSuccess) {
    e.err = std::string("nlp2op: ") + hipGetErrorString(s);
    return RPM_E_DEVICE;
  }
  return RPM_OK;
}

// CheckSolutionDiffError for one phase: host x in, relative_error ((N + K + 1) x nx, column-major) out
int dev_solution_error(Engine& e, int phase, const double* x, double* rel_err) {
  int rc = dev_bind(e);
  if (rc) return rc;
  Device& d = *e.dev;
  const PhaseHost& p = e.ph[phase];
  if (e.mesh_err.size() != e.ph.size()) e.mesh_err.assign(e.ph.size(), MeshErrTables());
  MeshErrTables& t = e.mesh_err[phase];
  if (t.iv.empty()) build_mesh_err_tables(p, t);
  const int rows = t.rows, nx = p.nx, nu = p.nu, K = int(t.iv.size());
  int nmax = 0;
  for (const MeshIvDev& iv : t.iv) nmax = std::max(nmax, iv.n + 1);
  const size_t lds = sizeof(double) * size_t(nmax) * (2 * nx + nu);
  if (lds > 60 * 1024) {
    e.err = "solution_error: a mesh interval has too many nodes for the estimator's LDS tile";
    return RPM_E_UNSUPPORTED;
  }
  // one device block: doubles first, then the ints
  const size_t nd = t.ttem.size() + t.Hs.size() + t.Ss.size() + t.Hc.size() + t.Sc.size() + t.A.size() + 3 * size_t(rows) * nx;
  const size_t ni = t.hit_s.size() + t.hit_c.size();
  const size_t bytes = nd * sizeof(double) + ni * sizeof(int) + K * sizeof(MeshIvDev);
  char* buf = nullptr;
  HIP_TRY(e, hipMalloc(reinterpret_cast<void**>(&buf), bytes));
  double* dd = reinterpret_cast<double*>(buf);
  double* d_ttem = dd; dd += t.ttem.size();
  double* d_Hs = dd; dd += t.Hs.size();
  double* d_Ss = dd; dd += t.Ss.size();
  double* d_Hc = dd; dd += t.Hc.size();
  double* d_Sc = dd; dd += t.Sc.size();
  double* d_A = dd; dd += t.A.size();
  double* d_fine = dd; dd += size_t(rows) * nx;
  double* d_integ = dd; dd += size_t(rows) * nx;
  double* d_rel = dd; dd += size_t(rows) * nx;
  int* d_hit_s = reinterpret_cast<int*>(dd);
  int* d_hit_c = d_hit_s + t.hit_s.size();
  MeshIvDev* d_iv = reinterpret_cast<MeshIvDev*>(d_hit_c + t.hit_c.size());
  hipError_t s = hipSuccess;
  auto put = [&](void* dev, const void* host, size_t cnt) {
    if (cnt && s == hipSuccess) s = hipMemcpy(dev, host, cnt, hipMemcpyHostToDevice);
  };
  put(d_ttem, t.ttem.data(), t.ttem.size() * sizeof(double));
  put(d_Hs, t.Hs.data(), t.Hs.size() * sizeof(double));
  put(d_Ss, t.Ss.data(), t.Ss.size() * sizeof(double));
  put(d_Hc, t.Hc.data(), t.Hc.size() * sizeof(double));
  put(d_Sc, t.Sc.data(), t.Sc.size() * sizeof(double));
  put(d_A, t.A.data(), t.A.size() * sizeof(double));
  put(d_hit_s, t.hit_s.data(), t.hit_s.size() * sizeof(int));
  put(d_hit_c, t.hit_c.data(), t.hit_c.size() * sizeof(int));
  put(d_iv, t.iv.data(), K * sizeof(MeshIvDev));
  rc = (s == hipSuccess) ? dev_upload(e, d.d_x, x, size_t(e.n), STAGE_X) : RPM_OK;
  if (rc == RPM_OK && s == hipSuccess) {
    hipStream_t st = d.stream;
    with_problem(e.problem_id, [&](auto prob) {
      using P = decltype(prob);
      hipLaunchKernelGGL((rpm_mesh_err_kernel<P>), dim3(unsigned(K)), dim3(128), lds, st, d.kp, phase, d.d_x, d_iv, K, d_Hs,
                         d_Ss, d_hit_s, d_Hc, d_Sc, d_hit_c, d_A, d_ttem, rows, d_fine, d_integ);
    });
    hipLaunchKernelGGL(rpm_mesh_rel_kernel, dim3(unsigned(nx)), dim3(256), 0, st, rows, d_fine, d_integ, d_rel);
    s = hipGetLastError();
    if (s == hipSuccess) s = hipStreamSynchronize(st);
    if (s == hipSuccess) rc = dev_download(e, rel_err, d_rel, size_t(rows) * nx, STAGE_HESS);
  }
  (void)hipFree(buf);
  if (rc) return rc;
  if (s != hipSuccess) {
    e.err = std::string("solution_error: ") + hipGetErrorString(s);
    return RPM_E_DEVICE;
  }
  return RPM_OK;
}

// ------------------------------------------------------------------------------------------
// The mesh-error estimate of a whole sweep: every phase and every instance of the engine in three launches, nothing but
// the caller's arrays crossing the call.  Per instance b the arithmetic is that of rpm_mesh_err_kernel + rpm_mesh_rel_kernel
// on x + b * n, the same mesh_* rules of rpm_post_device.hpp on other bases, with the dynamics reading instance b's constants
// and static parameters.  The interpolation / integration tables of all phases sit in one device block that
// lives as long as the engine's other tables (Device::mesh_batch).
struct MeshIvBatch {   // one mesh interval of any phase: MeshIvDev with offsets into the engine-wide tables
  int n, istart, r0, q0, hs, hc, a;
  int phase, rows;     // its phase and that phase's row count N + K + 1
  int base;            // offset of the phase's rows x nx matrix inside an instance's block of RT doubles
  int first, last;     // first / last interval of its phase
};

// Workgroup (interval, tile of TB instances).  `stage`: the interval's tables are copied to LDS once and serve all TB
// instances; otherwise (tables too large next to the instance arrays) they are read from global memory as the one-instance
// kernel reads them.  Items run q-fastest, so the lanes that share (instance, state) read one x column and store a run of
// consecutive rows.
template <class Prob>
__global__ void rpm_mesh_err_batch_kernel(const KParams K, int B, int TB, int stage, long long RT, const double* __restrict__ x,
                                          const MeshIvBatch* __restrict__ ivs, const double* gHs, const double* gSs,
                                          const int* ghit_s, const double* gHc, const double* gSc, const int* ghit_c,
                                          const double* gA, const double* gtt, double* __restrict__ fine_state,
                                          double* __restrict__ integ, int* __restrict__ nonfinite) {
  constexpr int NX = Prob::NX, NU = Prob::NU;
  constexpr int NXs = NX > 0 ? NX : 1, NUs = NU > 0 ? NU : 1;
  extern __shared__ __align__(16) double mesh_bsm[];
  const MeshIvBatch v = ivs[blockIdx.x];
  const int n = v.n, n1 = n + 1;
  const int b0 = blockIdx.y * TB;
  const int nb = B - b0 < TB ? B - b0 : TB;
  const double *Hs = gHs + v.hs, *Hc = gHc + v.hc, *A = gA + v.a, *Ss = gSs + v.q0, *Sc = gSc + v.q0, *tt = gtt + v.q0;
  const int *hit_s = ghit_s + v.q0, *hit_c = ghit_c + v.q0;
  double* inst = mesh_bsm;
  if (stage) {
    double* lHs = mesh_bsm;
    double* lHc = lHs + n1 * n1;
    double* lA = lHc + n1 * n;
    double* lSs = lA + n1 * n1;
    double* lSc = lSs + n1;
    double* ltt = lSc + n1;
    int* lhit_s = reinterpret_cast<int*>(ltt + n1);
    int* lhit_c = lhit_s + n1;
    inst = ltt + 2 * n1;
    for (int i = threadIdx.x; i < n1 * n1; i += blockDim.x) {
      lHs[i] = Hs[i];
      lA[i] = A[i];
    }
    for (int i = threadIdx.x; i < n1 * n; i += blockDim.x) lHc[i] = Hc[i];
    for (int i = threadIdx.x; i < n1; i += blockDim.x) {
      lSs[i] = Ss[i];
      lSc[i] = Sc[i];
      ltt[i] = tt[i];
      lhit_s[i] = hit_s[i];
      lhit_c[i] = hit_c[i];
    }
    Hs = lHs; Hc = lHc; A = lA; Ss = lSs; Sc = lSc; tt = ltt; hit_s = lhit_s; hit_c = lhit_c;
    __syncthreads();
  }
  const int per = n1 * (2 * NX + NU);   // per instance: Xs [q * NX + s], Us [q * NU + j], Fs [q * NX + s]
  const PhaseDev ph = K.phases[v.phase];
  const int N = ph.N, M = N + 1, rows = v.rows;
  if (blockIdx.x == 0 && nonfinite)     // the verdicts of this call start from 0 (rpm_mesh_rel_batch_kernel ORs into them)
    for (int bi = threadIdx.x; bi < nb; bi += blockDim.x) nonfinite[b0 + bi] = 0;
  for (int idx = threadIdx.x; idx < nb * n1 * NX; idx += blockDim.x) {
    const int q = idx % n1, s = (idx / n1) % NXs, bi = idx / (n1 * NXs);
    const size_t b = size_t(b0 + bi);
    const double val = mesh_interp(hit_s[q], Hs + q, n1, n1, x + b * K.n + ph.x_state0 + s * M + v.istart, Ss + q);
    inst[bi * per + q * NX + s] = val;
    fine_state[b * RT + v.base + (v.r0 + q) + size_t(s) * rows] = val;
  }
  for (int idx = threadIdx.x; idx < nb * n1 * NU; idx += blockDim.x) {
    const int q = idx % n1, j = (idx / n1) % NUs, bi = idx / (n1 * NUs);
    inst[bi * per + n1 * NX + q * NU + j] =
        mesh_interp(hit_c[q], Hc + q, n1, n, x + size_t(b0 + bi) * K.n + ph.x_control0 + j * N + v.istart, Sc + q);
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < nb * n1; idx += blockDim.x) {
    const int q = idx % n1, bi = idx / n1;
    const double* xb = x + size_t(b0 + bi) * K.n;
    const double* Xs = inst + bi * per;
    const double* Us = Xs + n1 * NX;
    double* Fs = inst + bi * per + n1 * (NX + NU);
    const double t0 = xb[ph.x_t0];
    mesh_dynamics<Prob>(ph, t0, post_time(t0, xb[ph.x_t0 + 1], 1.0), tt[q], Xs + q * NX, Us + q * NU, xb + ph.x_t0 + 2,
                        K.consts + size_t(b0 + bi) * K.consts_stride, Fs + q * NX);
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < nb * n1 * NX; idx += blockDim.x) {
    const int r = idx % n1, s = (idx / n1) % NXs, bi = idx / (n1 * NXs);
    const double* Xs = inst + bi * per;
    const double* Fs = Xs + n1 * (NX + NU);
    integ[size_t(b0 + bi) * RT + v.base + (1 + v.r0 + r) + size_t(s) * rows] = mesh_integrate(A + r, n1, Fs, NX, s, Xs);
  }
  if (v.first)
    for (int idx = threadIdx.x; idx < nb * NX; idx += blockDim.x) {
      const int s = idx % NXs, bi = idx / NXs;
      integ[size_t(b0 + bi) * RT + v.base + size_t(s) * rows] = inst[bi * per + s];
    }
  if (v.last)
    for (int idx = threadIdx.x; idx < nb * NX; idx += blockDim.x) {
      const int s = idx % NXs, bi = idx / NXs;
      const size_t b = size_t(b0 + bi);
      fine_state[b * RT + v.base + (rows - 1) + size_t(s) * rows] = x[b * K.n + ph.x_state0 + s * M + N];
    }
}

// Workgroup (phase, instance): the denominators 1 + max(interpolated(:, s)) (a maximum: exact in any order), the
// relative-error matrix, the instance's NaN/Inf verdict and, one thread per interval, the std::max chain of rpm::ph_refine
// over the interval's rows (started from its first entry, so a NaN never replaces a number).  `keep`: every phase's matrix
// fits in LDS, the chain reads it from there.
__global__ void rpm_mesh_rel_batch_kernel(const PhaseDev* __restrict__ phases, const MeshIvBatch* __restrict__ ivs,
                                          const int* __restrict__ ph_iv0, long long RT, int KT, const double* __restrict__ fine_state,
                                          const double* __restrict__ integ, double* __restrict__ rel,
                                          double* __restrict__ interval_error, int* verdicts, int nx_max, int keep) {
  extern __shared__ __align__(16) double mesh_den[];   // [nx_max + 2] denominators, then (keep) the phase's matrix
  double* kept = mesh_den + nx_max + 2;
  const int p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const size_t b = blockIdx.y;
  const int iv0 = ph_iv0[p], Kp = ph_iv0[p + 1] - iv0;
  const int rows = ivs[iv0].rows, nx = phases[p].nx;
  const double* fs = fine_state + b * RT + ivs[iv0].base;
  const double* in = integ + b * RT + ivs[iv0].base;
  for (int s = wave; s < nx; s += waves) {
    const double* col = fs + size_t(s) * rows;
    double mx = col[0];
    for (int r = lane; r < rows; r += 64) mx = fmax(mx, col[r]);
    for (int w = 32; w > 0; w >>= 1) mx = fmax(mx, __shfl_xor(mx, w));
    if (lane == 0) mesh_den[s] = 1 + mx;
  }
  __syncthreads();
  bool bad = false;
  for (int idx = threadIdx.x; idx < rows * nx; idx += blockDim.x) {
    const double val = mesh_rel_entry(in[idx], fs[idx], mesh_den[idx / rows]);
    if (rel) rel[b * RT + ivs[iv0].base + idx] = val;
    if (keep) kept[idx] = val;
    bad |= nonfinite(val);
  }
  if (verdicts && bad) atomicOr(verdicts + b, 1);
  if (keep) __syncthreads();
  if (interval_error)
    for (int k = threadIdx.x; k < Kp; k += blockDim.x) {
      const MeshIvBatch v = ivs[iv0 + k];
      const int istart = v.r0, ifinish = v.r0 + v.n + 1;
      // the chain is sequential: it reads the matrix from LDS when it fits there, else recomputes the entries (same bits)
      auto at = [&](int r, int s) {
        return keep ? kept[r + size_t(s) * rows] : mesh_rel_entry(in[r + size_t(s) * rows], fs[r + size_t(s) * rows], mesh_den[s]);
      };
      double emax = at(istart, 0);
      for (int s = 0; s < nx; ++s)
        for (int r = istart; r <= ifinish; ++r) {
          const double e = at(r, s);
          emax = emax < e ? e : emax;   // std::max(emax, e)
        }
      interval_error[b * KT + iv0 + k] = emax;
    }
}

// element-wise maximum of the included instances' matrices (mesh_err_max: a NaN stays).  Workgroup (16 elements, chunk y
// of `chunk` instances) x 16 instance slices, the slices combined in slice order; has[y] tells whether the chunk held an
// included instance.  Large sweeps run it twice, the second pass over the chunks' results with `has` as its mask; the
// pass that writes the caller's array (has == NULL) writes zeros when no instance was included.
__global__ void rpm_mesh_max_kernel(long long RT, int B, int chunk, const int* __restrict__ mask, const double* __restrict__ rel,
                                    double* __restrict__ out, int* __restrict__ has_out) {
  __shared__ double sv[256];
  __shared__ int sh[256];
  const int el = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const long long i = (long long)blockIdx.x * 16 + el;
  const int b0 = blockIdx.y * chunk, b1 = b0 + chunk < B ? b0 + chunk : B;
  double acc = 0.0;
  int has = 0;
  if (i < RT)
    for (int b = b0 + sl; b < b1; b += 16) {
      if (mask && mask[b] == 0) continue;
      const double val = rel[size_t(b) * RT + i];
      acc = has ? mesh_err_max(acc, val) : val;
      has = 1;
    }
  sv[threadIdx.x] = acc;
  sh[threadIdx.x] = has;
  __syncthreads();
  if (sl == 0 && i < RT) {
    for (int o = 1; o < 16; ++o)
      if (sh[o * 16 + el]) {
        acc = has ? mesh_err_max(acc, sv[o * 16 + el]) : sv[o * 16 + el];
        has = 1;
      }
    out[size_t(blockIdx.y) * RT + i] = has ? acc : 0.0;
    if (has_out && i == 0) has_out[blockIdx.y] = has;
  }
}

struct MeshBatch {
  char* block = nullptr;    // tables, then the workspace
  double *Hs, *Ss, *Hc, *Sc, *A, *tt, *fine, *integ, *rel, *part;   // part: kMaxChunks x RT, the first pass of the maximum
  int *hit_s, *hit_c, *ph_iv0, *part_has;
  MeshIvBatch* ivs;
  int KT = 0, nx_max = 0;
  long long RT = 0;
  size_t tab_doubles = 0, inst_doubles = 0;   // LDS of the largest interval: its tables / one instance's arrays
  size_t block_max = 0;                       // doubles of the largest phase's rows x nx matrix
  HostForm host;                           // host-pointer form: interval errors (B x KT), then the maximum (RT); the verdicts
  int *o_mask = nullptr, *h_mask = nullptr;   // its instance mask on the device and the page-locked block it is uploaded from
};

void mesh_batch_destroy(Device* d) {
  MeshBatch* mb = static_cast<MeshBatch*>(d->mesh_batch);
  if (!mb) return;
  if (mb->block) (void)hipFree(mb->block);
  mb->host.release();
  if (mb->o_mask) (void)hipFree(mb->o_mask);
  if (mb->h_mask) (void)hipHostFree(mb->h_mask);
  delete mb;
  d->mesh_batch = nullptr;
}

void solution_error_batch_sizes(const Engine& e, int* n_intervals_total, long long* rel_doubles_total) {
  int kt = 0;
  long long rt = 0;
  for (const PhaseHost& p : e.ph) {
    kt += p.K;
    rt += (long long)(p.N + p.K + 1) * p.nx;
  }
  if (n_intervals_total) *n_intervals_total = kt;
  if (rel_doubles_total) *rel_doubles_total = rt;
}

namespace {

constexpr size_t kMeshLdsLimit = 60 * 1024;
constexpr int kMaxChunks = 32;   // rpm_mesh_max_kernel's first pass over a large sweep

// first use on an engine: tables of all phases into one device block, workspace behind them (the only allocation and the
// only blocking copies of the batched estimate)
int mesh_batch_setup(Engine& e) {
  Device& d = *e.dev;
  if (d.mesh_batch) return RPM_OK;
  if (e.mesh_err.size() != e.ph.size()) e.mesh_err.assign(e.ph.size(), MeshErrTables());
  std::vector<MeshIvBatch> ivs;
  std::vector<double> Hs, Ss, Hc, Sc, A, tt;
  std::vector<int> hit_s, hit_c, ph_iv0;
  MeshBatch m;
  solution_error_batch_sizes(e, &m.KT, &m.RT);
  long long base = 0;
  for (size_t ip = 0; ip < e.ph.size(); ++ip) {
    const PhaseHost& p = e.ph[ip];
    MeshErrTables& t = e.mesh_err[ip];
    if (t.iv.empty()) build_mesh_err_tables(p, t);
    ph_iv0.push_back(int(ivs.size()));
    for (size_t k = 0; k < t.iv.size(); ++k) {
      const MeshIvDev& s = t.iv[k];
      MeshIvBatch v;
      v.n = s.n; v.istart = s.istart; v.r0 = s.r0;
      v.q0 = s.q0 + int(tt.size());
      v.hs = s.hs + int(Hs.size());
      v.hc = s.hc + int(Hc.size());
      v.a = s.a + int(A.size());
      v.phase = int(ip); v.rows = t.rows; v.base = int(base);
      v.first = k == 0; v.last = k + 1 == t.iv.size();
      ivs.push_back(v);
      const size_t n1 = size_t(s.n) + 1;
      m.tab_doubles = std::max(m.tab_doubles, n1 * n1 * 2 + n1 * s.n + 4 * n1);   // Hs, A, Hc, Ss, Sc, tt, two int rows
      m.inst_doubles = std::max(m.inst_doubles, n1 * size_t(2 * p.nx + p.nu));
    }
    auto app = [](auto& dst, const auto& src) { dst.insert(dst.end(), src.begin(), src.end()); };
    app(tt, t.ttem); app(Hs, t.Hs); app(Ss, t.Ss); app(Hc, t.Hc); app(Sc, t.Sc); app(A, t.A);
    app(hit_s, t.hit_s); app(hit_c, t.hit_c);
    base += (long long)t.rows * p.nx;
    m.block_max = std::max(m.block_max, size_t(t.rows) * p.nx);
    m.nx_max = std::max(m.nx_max, p.nx);
  }
  ph_iv0.push_back(int(ivs.size()));
  const size_t B = size_t(e.n_instances);
  const size_t nd = tt.size() + Hs.size() + Ss.size() + Hc.size() + Sc.size() + A.size() + (3 * B + kMaxChunks) * size_t(m.RT);
  const size_t ni = hit_s.size() + hit_c.size() + ph_iv0.size() + kMaxChunks;
  HIP_TRY(e, hipMalloc(reinterpret_cast<void**>(&m.block), nd * sizeof(double) + ni * sizeof(int) + ivs.size() * sizeof(MeshIvBatch)));
  double* dd = reinterpret_cast<double*>(m.block);
  m.tt = dd; dd += tt.size();
  m.Hs = dd; dd += Hs.size();
  m.Ss = dd; dd += Ss.size();
  m.Hc = dd; dd += Hc.size();
  m.Sc = dd; dd += Sc.size();
  m.A = dd; dd += A.size();
  m.fine = dd; dd += B * size_t(m.RT);
  m.integ = dd; dd += B * size_t(m.RT);
  m.rel = dd; dd += B * size_t(m.RT);
  m.part = dd; dd += kMaxChunks * size_t(m.RT);
  m.hit_s = reinterpret_cast<int*>(dd);
  m.hit_c = m.hit_s + hit_s.size();
  m.ph_iv0 = m.hit_c + hit_c.size();
  m.part_has = m.ph_iv0 + ph_iv0.size();
  m.ivs = reinterpret_cast<MeshIvBatch*>(m.part_has + kMaxChunks);
  hipError_t s = hipSuccess;
  auto put = [&](void* dev, const void* host, size_t cnt) {
    if (cnt && s == hipSuccess) s = hipMemcpy(dev, host, cnt, hipMemcpyHostToDevice);
  };
  put(m.tt, tt.data(), tt.size() * sizeof(double));
  put(m.Hs, Hs.data(), Hs.size() * sizeof(double));
  put(m.Ss, Ss.data(), Ss.size() * sizeof(double));
  put(m.Hc, Hc.data(), Hc.size() * sizeof(double));
  put(m.Sc, Sc.data(), Sc.size() * sizeof(double));
  put(m.A, A.data(), A.size() * sizeof(double));
  put(m.hit_s, hit_s.data(), hit_s.size() * sizeof(int));
  put(m.hit_c, hit_c.data(), hit_c.size() * sizeof(int));
  put(m.ph_iv0, ph_iv0.data(), ph_iv0.size() * sizeof(int));
  put(m.ivs, ivs.data(), ivs.size() * sizeof(MeshIvBatch));
  if (s != hipSuccess) {
    (void)hipFree(m.block);
    return step_fail(e, RPM_E_DEVICE, std::string("solution_error_batch: ") + hipGetErrorString(s));
  }
  d.mesh_batch = new MeshBatch(m);
  return RPM_OK;
}

// what the engine's mesh refuses, decided on the host before a device is touched (the arguments: rpm_abi.cpp)
int mesh_check(Engine& e) {
  size_t inst_doubles = 0;   // one instance's Xs / Us / Fs arrays of the largest interval
  for (const PhaseHost& p : e.ph)
    for (const int n : p.nk) inst_doubles = std::max(inst_doubles, (size_t(n) + 1) * size_t(2 * p.nx + p.nu));
  if (inst_doubles * sizeof(double) > kMeshLdsLimit)
    return step_fail(e, RPM_E_UNSUPPORTED, "solution_error_batch: a mesh interval has too many nodes for the estimator's LDS tile");
  return RPM_OK;
}

// three or four launches on `st`; the engine's device is current
int mesh_launch(Engine& e, const double* d_x, const int* d_mask, double* d_interval_error, double* d_rel_err_max, double* d_rel_err,
                int* d_nonfinite, hipStream_t st) {
  const int rc = mesh_batch_setup(e);
  if (rc) return rc;
  Device& d = *e.dev;
  const MeshBatch& m = *static_cast<MeshBatch*>(d.mesh_batch);
  const int B = e.n_instances;
  // instances per workgroup: the largest of 8, 4, 2, 1 (or the option) whose arrays fit next to the staged tables (one always
  // does: mesh_check), then no more than the sweep has
  const int stage = (m.tab_doubles + m.inst_doubles) * sizeof(double) <= kMeshLdsLimit ? 1 : 0;
  const size_t tab = stage ? m.tab_doubles : 0;
  auto bytes = [&](int tb) { return (tab + size_t(tb) * m.inst_doubles) * sizeof(double); };
  const int TB = clamp_tile(std::max(1, halve_tile(e.opt_mesh_err_tile > 0 ? e.opt_mesh_err_tile : 8, [&](int tb) { return bytes(tb) <= kMeshLdsLimit; })), B);
  const size_t lds = bytes(TB);
  double* rel = d_rel_err ? d_rel_err : (d_rel_err_max ? m.rel : nullptr);
  with_problem(e.problem_id, [&](auto prob) {
    using P = decltype(prob);
    hipLaunchKernelGGL((rpm_mesh_err_batch_kernel<P>), dim3(unsigned(m.KT), unsigned((B + TB - 1) / TB)), dim3(256), lds, st, d.kp, B,
                       TB, stage, m.RT, d_x, m.ivs, m.Hs, m.Ss, m.hit_s, m.Hc, m.Sc, m.hit_c, m.A, m.tt, m.fine, m.integ, d_nonfinite);
  });
  if (rel || d_interval_error || d_nonfinite) {
    const size_t den = size_t(m.nx_max) + 2;
    const int keep = d_interval_error && (den + m.block_max) * sizeof(double) <= kMeshLdsLimit ? 1 : 0;
    hipLaunchKernelGGL(rpm_mesh_rel_batch_kernel, dim3(unsigned(e.P), unsigned(B)), dim3(256), (den + (keep ? m.block_max : 0)) * sizeof(double),
                       st, d.d_phases, m.ivs, m.ph_iv0, m.RT, m.KT, m.fine, m.integ, rel, d_interval_error, d_nonfinite, m.nx_max, keep);
  }
  if (d_rel_err_max) {
    const unsigned gx = unsigned((m.RT + 15) / 16);
    int* const no_has = nullptr;
    if (B <= 2 * kMaxChunks) {
      hipLaunchKernelGGL(rpm_mesh_max_kernel, dim3(gx), dim3(256), 0, st, m.RT, B, B, d_mask, rel, d_rel_err_max, no_has);
    } else {   // 55 workgroups cannot pull 1024 matrices in at speed: chunks first, then the chunks' results
      const int chunk = (B + kMaxChunks - 1) / kMaxChunks, chunks = (B + chunk - 1) / chunk;
      hipLaunchKernelGGL(rpm_mesh_max_kernel, dim3(gx, unsigned(chunks)), dim3(256), 0, st, m.RT, B, chunk, d_mask, rel, m.part, m.part_has);
      hipLaunchKernelGGL(rpm_mesh_max_kernel, dim3(gx), dim3(256), 0, st, m.RT, chunks, chunks, m.part_has, m.part, d_rel_err_max, no_has);
    }
  }
  return step_launched(e, "solution_error_batch");
}

}  // namespace

// device-resident: three or four launches on `stream`; after the first call on an engine nothing else
int dev_solution_error_batch(Engine& e, const double* d_x, const int* d_mask, double* d_interval_error, double* d_rel_err_max,
                             double* d_rel_err, int* d_nonfinite, void* stream) {
  int rc = mesh_check(e);
  if (rc) return rc;
  DeviceRestore restore;
  rc = dev_bind(e);
  if (rc) return rc;
  return mesh_launch(e, d_x, d_mask, d_interval_error, d_rel_err_max, d_rel_err, d_nonfinite, static_cast<hipStream_t>(stream));
}

// the same through host arrays: x (and the mask) up through the staging slots, the requested results back; blocking
int host_solution_error_batch(Engine& e, const double* x, const int* mask, double* interval_error, double* rel_err_max,
                              double* rel_err, int* nonfinite) {
  int rc = mesh_check(e);
  if (rc) return rc;
  DeviceRestore restore;
  rc = dev_bind(e);
  if (rc == RPM_OK) rc = mesh_batch_setup(e);
  if (rc) return rc;
  Device& d = *e.dev;
  MeshBatch& m = *static_cast<MeshBatch*>(d.mesh_batch);
  const size_t B = size_t(e.n_instances), o_max = B * m.KT;   // the block: the interval errors, then the maximum
  if (mask && !m.o_mask) {   // sized once, unlike `host`: an engine's n_instances never changes
    HIP_TRY(e, hipMalloc(reinterpret_cast<void**>(&m.o_mask), B * sizeof(int)));
    HIP_TRY(e, hipHostMalloc(reinterpret_cast<void**>(&m.h_mask), B * sizeof(int), hipHostMallocDefault));
  }
  return m.host.run(
      e, o_max + size_t(m.RT), {{d.d_x, 0, x, B * e.n, STAGE_X}},
      [&](double* b, int* flags) -> int {
        if (mask) {
          std::memcpy(m.h_mask, mask, B * sizeof(int));
          HIP_TRY(e, hipMemcpyAsync(m.o_mask, m.h_mask, B * sizeof(int), hipMemcpyHostToDevice, d.stream));
        }
        return mesh_launch(e, d.d_x, mask ? m.o_mask : nullptr, interval_error ? b : nullptr, rel_err_max ? b + o_max : nullptr,
                           rel_err ? m.rel : nullptr, flags, d.stream);
      },
      {{interval_error, nullptr, 0, o_max, STAGE_G}, {rel_err_max, nullptr, o_max, size_t(m.RT), STAGE_V}, {rel_err, m.rel, 0, B * size_t(m.RT), STAGE_HESS}},
      nonfinite);
}

}  // namespace rpm
