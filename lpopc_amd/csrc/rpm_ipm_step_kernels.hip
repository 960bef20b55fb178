// rpm_ipm_step_kernels.hip — row f-2: the vector kernels of the batched primal-dual interior-point iteration, with every iterate
// and multiplier resident in HBM (see rpm_ipm.hpp for what is restated and what is not).  One workgroup per instance (several for
// a few large instances); the NLP callbacks are the engine's own batched launches; the KKT matrix, its LDL^T and the substitution
// are rpm_kkt_assemble.hip, rpm_kkt_factor.hip and rpm_kkt_solve.hip.
//
// Per iteration (Waechter & Biegler 2006, the equation numbers below are that paper's):
//   grad f + A^T lambda; residuals, optimality error E_0 / E_mu (5), barrier update (7) or the          ipm_jt_lambda_kernel,
//     adaptive rule, tau (8); in restoration mode the same for the restoration problem + the test to leave it   ipm_residual_kernel
//   K (13), LDL^T, inertia check / correction (Algorithm IC), solution           rpm_kkt_assemble.hip, rpm_kkt_factor.hip, rpm_kkt_solve.hip
//   direction, dz (12), fraction to the boundary (15), alpha_min (23)            ipm_direction_kernel
//   filter line search (18)-(20), (22), second-order correction (A-5.5 .. 5.9)   ipm_trial_kernel, ipm_accept_kernel, ipm_soc_rhs_kernel, ipm_soc_direction_kernel
//   step, multiplier reset (16), filter update, entry into the restoration phase ipm_update_kernel
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "rpm_device_internal.hpp"
#include "rpm_ipm_device.hpp"

namespace rpm {

// ------------------------------------------------------------------------------------------------ helpers
__device__ inline double block_red(double v, int kind, double* sh) {   // 0 sum, 1 max, 2 min; result on every thread
  for (int o = 32; o; o >>= 1) {
    const double w = __shfl_down(v, o);
    v = kind == 0 ? v + w : (kind == 1 ? fmax(v, w) : fmin(v, w));
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = sh[0];
  for (int i = 1; i < int(blockDim.x >> 6); ++i) r = kind == 0 ? r + sh[i] : (kind == 1 ? fmax(r, sh[i]) : fmin(r, sh[i]));
  return r;
}
__device__ inline bool has_lo(double l, double u) { return l > -IPM_INF && l != u; }
__device__ inline bool has_up(double l, double u) { return u < IPM_INF && l != u; }

// Several workgroups per instance (gridDim.x = G > 1; blockIdx.y = instance) when a few large instances run: every workgroup
// takes a slice and leaves its N partial results (kind 0 sum, 1 max, 2 min) in D.part; the LAST one to arrive — a ticket in
// D.tick — combines them in workgroup order, so the totals do not depend on who finishes last, and carries on alone with the
// instance's verdicts (true is returned on that workgroup only; with G = 1 always).  Until then nobody has changed the
// instance record, so every workgroup has read the same flags.
template <int N>
__device__ inline bool vec_combine(const IpmDev& D, int bi, double (&vals)[N], const int (&kind)[N]) {
  static_assert(N <= IPM_VEC_PART, "IPM_VEC_PART");
  const int G = gridDim.x;
  if (G == 1) return true;
  __shared__ int last_arrival;
  double* P = D.part + size_t(bi) * IPM_VEC_BLOCKS * IPM_VEC_PART;
  if (threadIdx.x == 0) {
    double* mine = P + size_t(blockIdx.x) * IPM_VEC_PART;
#pragma unroll
    for (int k = 0; k < N; ++k) mine[k] = vals[k];
    __threadfence();
    last_arrival = atomicAdd(&D.tick[bi], 1) == G - 1;
  }
  __syncthreads();
  if (!last_arrival) return false;
  __threadfence();
  // the partial results into LDS side by side (as G x N dependent loads of every thread they took 20 us of a 30 us kernel on the
  // metric problem), then added up in workgroup order as before
  __shared__ double staged[IPM_VEC_BLOCKS * N];
  for (int idx = threadIdx.x; idx < G * N; idx += blockDim.x) staged[idx] = P[size_t(idx / N) * IPM_VEC_PART + idx % N];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) vals[k] = kind[k] == 0 ? 0.0 : (kind[k] == 1 ? -1e300 : 1e300);
  for (int b = 0; b < G; ++b) {
    const double* q = staged + b * N;
#pragma unroll
    for (int k = 0; k < N; ++k) vals[k] = kind[k] == 0 ? vals[k] + q[k] : (kind[k] == 1 ? fmax(vals[k], q[k]) : fmin(vals[k], q[k]));
  }
  if (threadIdx.x == 0) D.tick[bi] = 0;
  return true;
}
// nothing to combine, the arrival ticket alone: true on the last workgroup of the instance to get here
__device__ inline bool vec_last_arrival(const IpmDev& D, int bi) {
  double none[1] = {0.0};
  const int none_kind[1] = {0};
  return vec_combine(D, bi, none, none_kind);
}
// A kernel's reduced quantities, each named once: reduce_and_combine(D, bi, sh, red_sum(a), red_max(b), ...) leaves in every listed
// variable its total over the instance — block_red over the workgroup, then vec_combine over the workgroups, slots in list order —
// and returns vec_combine's verdict (the totals are there only where it is true).  used = false (the same on every thread): a
// quantity the present mode does not accumulate skips the block reduction and rides along as it is.
template <int KIND>
struct Red {
  double& v;
  bool used;
  static constexpr int kind = KIND;
};
__device__ inline Red<0> red_sum(double& v, bool used = true) { return {v, used}; }
__device__ inline Red<1> red_max(double& v) { return {v, true}; }
__device__ inline Red<2> red_min(double& v) { return {v, true}; }
template <class... R>
__device__ inline bool reduce_and_combine(const IpmDev& D, int bi, double* sh, R... r) {
  double vals[sizeof...(R)] = {(r.used ? block_red(r.v, R::kind, sh) : r.v)...};      // (a braced list: left to right)
  const int kind[sizeof...(R)] = {R::kind...};
  if (!vec_combine(D, bi, vals, kind)) return false;
  int k = 0;
  ((r.v = vals[k++]), ...);
  return true;
}

// ------------------------------------------------------------------------------------------------ start
// x pushed into the interior of its bounds (Ipopt 3.12 bound_push / bound_frac, paper section 3.6), z = 1, lambda = 0.  The
// bounds themselves first move out by bound_relax * max(1, |bound|) (Ipopt's bound_relax_factor): vl0 / vu0 keep the caller's.
__device__ inline double relax(double bound, const IpmOpts& o) { return o.bound_relax * fmax(1.0, fabs(bound)); }
__device__ inline double push_inside(double x, double l, double u, bool lo, bool up, double push, double frac) {
  if (lo) {
    const double p = up ? fmin(push * fmax(1.0, fabs(l)), frac * (u - l)) : push * fmax(1.0, fabs(l));
    x = fmax(x, l + p);
  }
  if (up) {
    const double p = lo ? fmin(push * fmax(1.0, fabs(u)), frac * (u - l)) : push * fmax(1.0, fabs(u));
    x = fmin(x, u - p);
  }
  return x;
}
// The cold start (warm = 0: bound_push / bound_frac, z = 1, lambda = 0, least-squares multipliers where the option asks) and the
// warm start (warm = 1: the warm_start_* pushes; the duals are ipm_warm_duals_kernel's, after the scaling factors exist) share the
// bounds, the fixed / free pattern, the push rule and the fresh instance record.  A NaN bound (a measured state that is one,
// rpm_ipm_set_initial_states) compares unequal to itself: the variable would count as free of bounds while the KKT layout has it
// fixed, so it ends the instance with status 5 before its first pass.  So does a NaN or Inf in x0: fmax / fmin of the push rule
// return their other argument for a NaN, which would start the instance from its bound as if nothing were wrong.
__global__ __launch_bounds__(256) void ipm_init_kernel(IpmDev D, const double* x0, int warm) {
  const int bi = blockIdx.x;
  const size_t o = size_t(bi) * D.nv;
  const double push = warm ? D.o.ws_bound_push : D.o.bound_push, frac = warm ? D.o.ws_bound_frac : D.o.bound_frac;
  int bad = 0;
  for (int i = threadIdx.x; i < D.n; i += blockDim.x) {
    double x = x0[size_t(bi) * D.n + i];
    double l = D.vl0[o + i], u = D.vu0[o + i];
    bad |= (l != l) || (u != u) || nonfinite(x);
    const bool lo = has_lo(l, u), up = has_up(l, u);
    if (l == u) x = l;
    else {
      if (lo) l -= relax(l, D.o);
      if (up) u += relax(u, D.o);
      x = push_inside(x, l, u, lo, up, push, frac);
    }
    D.v[o + i] = x;
    D.vl[o + i] = l;
    D.vu[o + i] = u;
    if (!warm) {
      D.zL[o + i] = lo ? 1.0 : 0.0;
      D.zU[o + i] = up ? 1.0 : 0.0;
    }
  }
  if (!warm)
    for (int r = threadIdx.x; r < D.m; r += blockDim.x) D.lam[size_t(bi) * D.m + r] = 0.0;
  const int any_bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    IpmInst& S = D.inst[bi];
    S = IpmInst{};
    S.mu = D.o.mu_init;
    if (!warm && D.o.init_ls_mult && D.m > 0) { S.mode = 3; S.skip_update = -2; }   // first pass: least-squares multipliers at the starting point
    if (any_bad) S.status = 5;
  }
}
// The measured initial states of a receding-horizon sweep written into the caller's bounds: vl0 = vu0 = state0[b][j] at variable
// x_state0 + j M of every instance, nothing else touched.  One thread per (instance, state).
__global__ __launch_bounds__(256) void ipm_set_state0_kernel(IpmDev D, int x_state0, int M, int nx, const double* __restrict__ state0) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= D.B * nx) return;
  const int j = idx % nx, bi = idx / nx;
  const size_t o = size_t(bi) * D.nv + x_state0 + size_t(j) * M;
  const double s = state0[idx];
  D.vl0[o] = s;
  D.vu0[o] = s;
}
// slacks start at g(x0), pushed inside the (relaxed) [g_l, g_u] the same way
__global__ __launch_bounds__(256) void ipm_init_slack_kernel(IpmDev D, int warm) {
  const int bi = blockIdx.x;
  const double push = warm ? D.o.ws_slack_bound_push : D.o.bound_push, frac = warm ? D.o.ws_slack_bound_frac : D.o.bound_frac;
  for (int s = threadIdx.x; s < D.ns; s += blockDim.x) {
    const int r = D.slack_row[s];
    double l = D.gl[r], u = D.gu[r];
    const bool lo = l > -IPM_INF, up = u < IPM_INF;
    if (D.scal_on) {           // the rows are scaled (nlp_scaling): so are their bounds
      const double sr = D.sc[size_t(bi) * D.m + r];
      if (lo) l *= sr;
      if (up) u *= sr;
    }
    if (lo) l -= relax(l, D.o);
    if (up) u += relax(u, D.o);
    const size_t o = size_t(bi) * D.nv + D.n + s;
    D.v[o] = push_inside(D.g[size_t(bi) * D.sg + r], l, u, lo, up, push, frac);
    D.vl[o] = l;
    D.vu[o] = u;
    if (!warm) {
      D.zL[o] = lo ? 1.0 : 0.0;
      D.zU[o] = up ? 1.0 : 0.0;
    }
  }
}
// The warm start's duals, after ipm_init_slack_kernel and (nlp_scaling) the scaling factors.  lambda: the caller's, clipped to
// +-warm_start_mult_init_max, then into the scaled problem, (lambda sf) / sc.  z of a variable: the caller's raised to
// warm_start_mult_bound_push, then times sf — or, z_L / z_U NULL, mu_init over the distance of the pushed x to its relaxed bound —
// where the bound exists and the variable is free, else 0.  z of the slack of row r from its stationarity -lambda_r - zL + zU = 0:
// zL = max(-lambda_r, floor), zU = max(lambda_r, floor) where the bound exists.  A NaN or Inf in x0 (n per instance), lambda or z ends
// the instance with status 5 before its first pass.
__device__ inline double dual_floor(double z, const IpmOpts& o) { return fmax(z, o.ws_mult_bound_push); }
__global__ __launch_bounds__(256) void ipm_warm_duals_kernel(IpmDev D, const double* x0, const double* lam_in, const double* zL_in,
                                                             const double* zU_in) {
  const int bi = blockIdx.x;
  const size_t o = size_t(bi) * D.nv;
  const double sf = D.scal_on ? D.sf[bi] : 1.0;
  const double* vl = D.vl + o, *vu = D.vu + o;
  int bad = 0;
  for (int r = threadIdx.x; r < D.m; r += blockDim.x) {
    double lam = lam_in[size_t(bi) * D.m + r];
    bad |= nonfinite(lam);
    lam = fmax(fmin(lam, D.o.ws_mult_init_max), -D.o.ws_mult_init_max);
    if (D.scal_on) lam = (lam * sf) / D.sc[size_t(bi) * D.m + r];
    D.lam[size_t(bi) * D.m + r] = lam;
    const int s = D.row_slack[r];
    if (s >= 0) {
      const double l = vl[D.n + s], u = vu[D.n + s];
      D.zL[o + D.n + s] = l > -IPM_INF ? dual_floor(-lam, D.o) : 0.0;
      D.zU[o + D.n + s] = u < IPM_INF ? dual_floor(lam, D.o) : 0.0;
    }
  }
  for (int i = threadIdx.x; i < D.n; i += blockDim.x) {
    const double l = vl[i], u = vu[i], x = D.v[o + i];
    const bool lo = has_lo(l, u), up = has_up(l, u);
    bad |= nonfinite(x0[size_t(bi) * D.n + i]);
    double zl, zu;
    if (zL_in) {
      zl = zL_in[size_t(bi) * D.n + i];
      zu = zU_in[size_t(bi) * D.n + i];
      bad |= nonfinite(zl) || nonfinite(zu);
      zl = dual_floor(zl, D.o);
      zu = dual_floor(zu, D.o);
      if (D.scal_on) { zl *= sf; zu *= sf; }
    } else {
      zl = D.o.mu_init / (x - l);
      zu = D.o.mu_init / (u - x);
    }
    D.zL[o + i] = lo ? zl : 0.0;
    D.zU[o + i] = up ? zu : 0.0;
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) D.inst[bi].status = 5;
}
// the multipliers of the variables' bounds as the caller's (unscaled) problem has them: z / sf, 0 where there is no bound or the
// variable is fixed; instance-major B x n
__global__ void ipm_bound_mult_kernel(IpmDev D, double* zL_out, double* zU_out) {
  const int bi = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.n) return;
  const size_t o = size_t(bi) * D.nv + i;
  const double l = D.vl[o], u = D.vu[o];
  double zl = has_lo(l, u) ? D.zL[o] : 0.0, zu = has_up(l, u) ? D.zU[o] : 0.0;
  if (D.scal_on) { const double sf = D.sf[bi]; zl /= sf; zu /= sf; }
  zL_out[size_t(bi) * D.n + i] = zl;
  zU_out[size_t(bi) * D.n + i] = zu;
}
__global__ void ipm_pack_x_kernel(IpmDev D) {
  const int bi = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < D.n) D.xe[size_t(bi) * D.n + i] = D.v[size_t(bi) * D.nv + i];
}

// ------------------------------------------------------------------------------------------------ residuals, E_mu, mu
// multiplier reset (16) of a bound multiplier z for the slack s
__device__ inline double reset16(double z, double s, double mu, double ks) { return fmax(fmin(z, ks * mu / s), mu / (ks * s)); }

// monotone barrier update (7): mu falls for as long as the barrier problem is solved to kappa_eps mu, E_mu (5) from the dual and
// primal errors and the extreme complementarity products (over sc; none: comp_on false).  Returns whether mu fell; *at_floor: it
// stopped at mu_min with the barrier problem solved there too.
__device__ inline bool monotone_mu(const IpmOpts& o, double dual, double prim, double cmax, double cmin, bool comp_on, double sc,
                                   double mu_min, double* mu, bool* at_floor) {
  bool fell = false;
  *at_floor = false;
  for (int guard = 0; guard < 64; ++guard) {
    const double comp = comp_on ? fmax(fabs(cmax - *mu), fabs(cmin - *mu)) : 0.0;
    const double emu = fmax(fmax(dual, prim), comp / sc);
    if (!(emu <= o.kappa_eps * *mu)) break;
    if (*mu <= mu_min) { *at_floor = true; break; }
    *mu = fmax(mu_min, fmin(o.kappa_mu * *mu, pow(*mu, o.theta_mu)));   // (7)
    fell = true;
  }
  return fell;
}

// grad f + A^T lambda by column (the restoration problem has no grad f).  A thread per unknown for the short columns; the long
// ones — t0, tf, the final states: every defect row of a phase, 7 168 entries on the metric problem, which one thread walked
// in 1.4 ms — take a workgroup each (blockIdx.x >= the thread-per-unknown blocks), summed in a fixed order.
__global__ __launch_bounds__(256) void ipm_jt_lambda_kernel(IpmDev D, int n_thread_blocks) {
  __shared__ double sh[16];
  const int bi = blockIdx.y;
  const IpmInst& S = D.inst[bi];
  if (S.status != 0) return;
  const double *lam = D.lam + size_t(bi) * D.m, *jac = D.jac + size_t(bi) * D.sv;
  const bool resto = S.mode == 2;
  if (int(blockIdx.x) >= n_thread_blocks) {
    const int i = D.long_cols[blockIdx.x - n_thread_blocks];
    double acc = 0.0;
    for (int q = D.jt_ptr[i] + threadIdx.x; q < D.jt_ptr[i + 1]; q += blockDim.x) acc += jac[D.jt_ent[q]] * lam[D.jt_row[q]];
    acc = block_red(acc, 0, sh);           // (one workgroup per column: nothing to combine)
    if (threadIdx.x == 0) D.glag[size_t(bi) * D.nv + i] = (resto ? 0.0 : D.grad[size_t(bi) * D.n + i]) + acc;
    return;
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.nv) return;
  double acc;
  if (i < D.n) {
    if (D.jt_ptr[i + 1] - D.jt_ptr[i] > IPM_LONG_COLUMN) return;
    acc = resto ? 0.0 : D.grad[size_t(bi) * D.n + i];
    for (int q = D.jt_ptr[i]; q < D.jt_ptr[i + 1]; ++q) acc += jac[D.jt_ent[q]] * lam[D.jt_row[q]];
  } else {
    acc = -lam[D.slack_row[i - D.n]];
  }
  D.glag[size_t(bi) * D.nv + i] = acc;
}
__global__ __launch_bounds__(1024) void ipm_residual_kernel(IpmDev D) {
  __shared__ double sh[16];
  __shared__ int verdict;       // restoration: 0 stay, 1 leave it (least-squares multipliers next), 2 stop
  // (several workgroups per instance when a few large instances run: slices i0, i0 + stride, ...; vec_combine)
  const int bi = blockIdx.y, t = threadIdx.x, i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  IpmInst& S = D.inst[bi];
  if (S.status != 0) return;
  const int mode_in = S.mode;
  if (mode_in == 3) {           // recalc_y: a pass that only recomputes the multipliers at this point (set by ipm_update_kernel)
    if (t == 0 && blockIdx.x == 0) { S.refactor = 1; S.delta_w = 0.0; atomicAdd(&D.cnt[0], 1); }
    return;
  }
  const double *v = D.v + size_t(bi) * D.nv, *vl = D.vl + size_t(bi) * D.nv, *vu = D.vu + size_t(bi) * D.nv;
  const double *zL = D.zL + size_t(bi) * D.nv, *zU = D.zU + size_t(bi) * D.nv, *lam = D.lam + size_t(bi) * D.m;
  const double *g = D.g + size_t(bi) * D.sg, *glag = D.glag + size_t(bi) * D.nv;
  double dinf = 0, cinf = 0, th1 = 0, cmax = 0, cmin = 1e300, sl = 0, sz = 0, ln = 0, bad = 0, nzb = 0;
  double csq = 0, dsq = 0, psum = 0, psq = 0, nfree = 0;      // 2-norms for the adaptive barrier update's KKT error
  double cinf_u = 0;            // nlp_scaling: the constraint violation of the unscaled problem (Ipopt's constr_viol_tol applies to it)
  // pass 1: constraint values and what does not depend on the multipliers
  #pragma unroll 4
  for (int r = i0; r < D.m; r += stride) {
    const int s = D.row_slack[r];
    const double glr = D.scal_on ? D.sc[size_t(bi) * D.m + r] * D.gl[r] : D.gl[r];
    const double cr = s < 0 ? g[r] - glr : g[r] - v[D.n + s];
    D.c[size_t(bi) * D.m + r] = cr;
    if (!(fabs(cr) < 1e300)) bad = 1;
    cinf = fmax(cinf, fabs(cr));
    cinf_u = fmax(cinf_u, D.scal_on ? fabs(cr / D.sc[size_t(bi) * D.m + r]) : fabs(cr));
    th1 += fabs(cr);
    csq += cr * cr;
  }
  if (mode_in == 2) {
    // ---- restoration phase (paper section 3.3): min rho sum(p + n) + zeta/2 |D_R (v - v_R)|^2  s.t.  c(v) - p + n = 0, p, n >= 0, bounds
    const IpmOpts& o = D.o;
    const double rho = o.resto_rho, zeta = S.zeta;
    const double *pp = D.pp + size_t(bi) * D.m, *nn = D.nn + size_t(bi) * D.m, *zp = D.zp + size_t(bi) * D.m, *zn = D.zn + size_t(bi) * D.m;
    const double *vR = D.vR + size_t(bi) * D.nv, *dr2 = D.dr2 + size_t(bi) * D.nv;
    double thr = 0, rinf = 0, spn = 0, lnpn = 0, qd = 0;
    #pragma unroll 4
    for (int r = i0; r < D.m; r += stride) {
      const double rc = D.c[size_t(bi) * D.m + r] - pp[r] + nn[r];
      thr += fabs(rc); rinf = fmax(rinf, fabs(rc));
      spn += pp[r] + nn[r];
      lnpn += log(pp[r]) + log(nn[r]);
      dinf = fmax(dinf, fmax(fabs(rho - lam[r] - zp[r]), fabs(rho + lam[r] - zn[r])));
      const double p1 = zp[r] * pp[r], p2 = zn[r] * nn[r];
      cmax = fmax(cmax, fmax(p1, p2)); cmin = fmin(cmin, fmin(p1, p2));
    }
    #pragma unroll 4
    for (int i = i0; i < D.nv; i += stride) {
      const double acc = glag[i];             // A^T lambda only (ipm_jt_lambda_kernel): the proximity term is added where zeta is known
      const double l = vl[i], u = vu[i];
      if (l == u) continue;
      const double dd = v[i] - vR[i];
      qd += dr2[i] * dd * dd;
      dinf = fmax(dinf, fabs(zeta * dr2[i] * dd + acc - zL[i] + zU[i]));
      if (!(fabs(acc) < 1e300)) bad = 1;
      if (l > -IPM_INF) { const double d = v[i] - l, pr = zL[i] * d; cmax = fmax(cmax, pr); cmin = fmin(cmin, pr); ln += log(d); }
      if (u < IPM_INF) { const double d = u - v[i], pr = zU[i] * d; cmax = fmax(cmax, pr); cmin = fmin(cmin, pr); ln += log(d); }
    }
    if (!reduce_and_combine(D, bi, sh, red_sum(thr), red_max(rinf), red_sum(spn), red_sum(lnpn), red_sum(qd), red_max(dinf), red_max(cmax),
                            red_min(cmin), red_sum(ln), red_max(bad), red_max(cinf), red_sum(th1))) return;
    if (t == 0) {
      const double f = D.obj[bi];
      verdict = 0;
      if (bad != 0 || !(fabs(f) < 1e300) || !(fabs(ln) < 1e300) || !(fabs(lnpn) < 1e300)) { S.status = 5; verdict = 2; }
      else {
        const double phi_o = f - S.mu * ln;      // the ORIGINAL barrier objective: what the original filter is asked about
        bool back = S.resto_it > 0 && th1 <= o.kappa_resto * S.th0 && th1 <= S.theta_max;
        const double* F = D.filt + size_t(bi) * 2 * IPM_FMAX;
        for (int k = 0; back && k < S.nfilt; ++k)
          if (th1 >= F[2 * k] && phi_o >= F[2 * k + 1]) back = false;
        if (back) verdict = 1;
        else if (S.resto_it >= o.resto_max) { S.status = 3; verdict = 2; }
        else if (S.iter >= o.max_iter) { S.status = 2; verdict = 2; }
        else {
          if (S.resto_it == 0) { S.thr_max = 1e4 * fmax(1.0, thr); S.thr_min = 1e-4 * fmax(1.0, thr); }
          double mu_r = S.mu_r;
          bool stuck;                                        // at the floor: a minimiser of the infeasibility that the filter does not take
          if (monotone_mu(o, dinf, rinf, cmax, cmin, true, 1.0, o.tol / 10.0, &mu_r, &stuck)) S.nrfilt = 0;
          if (stuck) { S.status = 3; verdict = 2; }
          else {
            S.mu_r = mu_r; S.zeta = sqrt(mu_r); S.tau = fmax(o.tau_min, 1.0 - mu_r);
            S.f = f; S.theta = th1; S.lnsum = ln; S.cinf = cinf; S.th_r = thr;
            S.phi_r = rho * spn + 0.5 * S.zeta * qd - mu_r * (ln + lnpn);
            S.refactor = 1;
            S.delta_w = 0.0;
            atomicAdd(&D.cnt[0], 1);
          }
        }
      }
    }
    __syncthreads();
    if (verdict != 1) return;
    // leaving the restoration: bound multipliers clipped against the ORIGINAL mu, then one pass that only computes
    // least-squares multipliers (mode 3; paper section 3.6) before the regular iteration resumes at this point
    #pragma unroll 4
    for (int i = t; i < D.nv; i += blockDim.x) {
      const double l = vl[i], u = vu[i];
      if (l == u) continue;
      const size_t o2 = size_t(bi) * D.nv + i;
      if (l > -IPM_INF) D.zL[o2] = reset16(fmin(D.zL[o2], 1e3), v[i] - l, S.mu, D.o.kappa_sigma);
      if (u < IPM_INF) D.zU[o2] = reset16(fmin(D.zU[o2], 1e3), u - v[i], S.mu, D.o.kappa_sigma);
    }
    if (t == 0) { S.mode = 3; S.refactor = 1; S.delta_w = 0.0; atomicAdd(&D.cnt[0], 1); }
    return;
  }
  // pass 2: gradient of the Lagrangian, complementarity products
  #pragma unroll 4
  for (int i = i0; i < D.nv; i += stride) {
    const double acc = glag[i];               // grad f + A^T lambda (ipm_jt_lambda_kernel)
    const double l = vl[i], u = vu[i], vi = v[i], zli = zL[i], zui = zU[i];    // loads ahead of the branch
    if (l != u) {
      const double dres = acc - zli + zui;
      dinf = fmax(dinf, fabs(dres));
      dsq += dres * dres; nfree += 1;
      if (!(fabs(acc) < 1e300)) bad = 1;
      if (l > -IPM_INF) {
        const double d = vi - l, pr = zli * d;
        cmax = fmax(cmax, pr); cmin = fmin(cmin, pr); sz += zli; ln += log(d); nzb += 1; psum += pr; psq += pr * pr;
      }
      if (u < IPM_INF) {
        const double d = u - vi, pr = zui * d;
        cmax = fmax(cmax, pr); cmin = fmin(cmin, pr); sz += zui; ln += log(d); nzb += 1; psum += pr; psq += pr * pr;
      }
    }
  }
  #pragma unroll 4
  for (int r = i0; r < D.m; r += stride) sl += fabs(lam[r]);
  if (!reduce_and_combine(D, bi, sh, red_max(dinf), red_max(cmax), red_min(cmin), red_sum(sl), red_sum(sz), red_sum(ln), red_max(bad), red_sum(nzb),
                          red_max(cinf), red_sum(th1), red_sum(csq), red_sum(dsq), red_sum(psum), red_sum(psq), red_sum(nfree), red_max(cinf_u))) return;
  if (t != 0) return;
  const IpmOpts& o = D.o;
  S.f = D.obj[bi]; S.theta = th1; S.lnsum = ln; S.dinf = dinf; S.cinf = cinf; S.comp_max = cmax; S.comp_min = cmin;
  S.sum_lam = sl; S.sum_z = sz; S.nzb = int(nzb);
  if (!(fabs(S.f) < 1e300) || !(fabs(ln) < 1e300)) bad = 1;
  const double sd = fmax(o.s_max, (sl + sz) / fmax(1.0, double(D.m) + nzb)) / o.s_max;   // (6)
  const double sc = nzb > 0 ? fmax(o.s_max, sz / nzb) / o.s_max : 1.0;
  S.err0 = fmax(fmax(dinf / sd, cinf), nzb > 0 ? cmax / sc : 0.0);
  if (bad != 0) { S.status = 5; return; }
  // Ipopt's secondary thresholds apply to the unscaled problem: gradient of the Lagrangian and complementarity / sf, rows / sc
  const double sfu = D.scal_on ? D.sf[bi] : 1.0;
  const double cm = (nzb > 0 ? cmax : 0.0) / sfu, dinf_u = dinf / sfu;
  if (S.err0 <= o.tol && dinf_u <= o.dual_inf_tol && cinf_u <= o.constr_viol_tol && cm <= o.compl_inf_tol) { S.status = 1; return; }
  S.n_acc = (S.err0 <= o.acceptable_tol && dinf_u <= o.acc_dual_inf_tol && cinf_u <= o.acc_constr_viol_tol && cm <= o.acc_compl_inf_tol) ? S.n_acc + 1 : 0;
  if (o.acceptable_iter > 0 && S.n_acc >= o.acceptable_iter) { S.status = 6; return; }
  if (S.iter >= o.max_iter) { S.status = 2; return; }
  if (S.iter == 0) {
    S.theta_max = 1e4 * fmax(1.0, th1);
    S.theta_min = 1e-4 * fmax(1.0, th1);
  }
  const double mu_min = o.tol / 10.0;
  double mu = S.mu;
  bool from_oracle = false;
  if (o.mu_adaptive && nzb > 0) {      // Ipopt's adaptive update: LOQO oracle, kkt-error globalisation (oracle/ipm_oracle.py)
    const double avg = psum / nzb;
    if (S.mu_max == 0.0) S.mu_max = o.mu_max_fact * avg;
    const double kkt_err = dsq / fmax(1.0, nfree) + (D.m ? csq / D.m : 0.0) + psq / nzb;
    bool progress = S.nrefs < 4;
    for (int k = 0; !progress && k < S.nrefs; ++k) progress = kkt_err <= o.mu_red_fact * S.refs[k];
    double mu_new = -1.0;
    if (progress) {
      S.fixed_mode = 0;
      if (S.nrefs < 4) S.refs[S.nrefs++] = kkt_err;
      else { S.refs[0] = S.refs[1]; S.refs[1] = S.refs[2]; S.refs[2] = S.refs[3]; S.refs[3] = kkt_err; }
      const double xi = cmin / avg, fac = fmin(0.05 * (1.0 - xi) / xi, 2.0);
      mu_new = fmax(mu_min, fmin(0.1 * fac * fac * fac * avg, S.mu_max));
    } else if (!S.fixed_mode) {        // no progress in the free mode: the monotone rule takes over from here
      S.fixed_mode = 1;
      mu_new = fmax(mu_min, fmin(o.mu_init_factor * avg, S.mu_max));
    }
    if (mu_new >= 0.0) {
      if (mu_new != mu) S.nfilt = 0;
      mu = mu_new;
      from_oracle = true;
    }
  }
  bool at_floor;                // (no event here: mu stays at mu_min)
  if (!from_oracle && monotone_mu(o, dinf / sd, cinf, cmax, cmin, nzb > 0, sc, mu_min, &mu, &at_floor)) S.nfilt = 0;
  S.mu = mu;
  S.tau = fmax(o.tau_min, 1.0 - mu);   // (8)
  S.phi = S.f - mu * ln;
  S.refactor = 1;
  S.delta_w = 0.0;
  if (o.ic_hot && S.ic_hot && o.kw_dec * S.delta_w_last >= o.ic_hot_min) S.delta_w = o.kw_dec * S.delta_w_last;
  atomicAdd(&D.cnt[0], 1);
}

// ------------------------------------------------------------------------------------------------ direction
// fraction to the boundary (15): largest a in (0, 1] with w + a dw >= (1 - tau) w
__device__ inline double ftb(double w, double dw, double tau, double a) { return dw < 0 ? fmin(a, -tau * w / dw) : a; }

// One bound of one unknown in a Newton step: slack s, multiplier z, d the step of the slack (the unknown's step; minus it for an
// upper bound).  Returns dz and takes the bound into the step lengths and into *gphi, the barrier objective's gradient in the unknown.
__device__ inline double bound_step(double s, double z, double d, bool upper, double mu, double tau, double* amax, double* az, double* gphi) {
  const double dz = mu / s - z - z / s * d;                // (12)
  *amax = ftb(s, d, tau, *amax);                           // (15a)
  *az = ftb(z, dz, tau, *az);                              // (15b)
  *gphi = upper ? *gphi + mu / s : *gphi - mu / s;
  return dz;
}
// The unknowns' part of a step from a solution of (13): dv, dz (12), step lengths (15), slope of the barrier objective — of the
// regular iteration (gradient: grad f) or, resto, of the restoration problem (gradient: its proximity term zeta D_R^2 (v - v_R)).
__device__ inline void newton_step_unknowns(const IpmDev& D, int bi, const double* sol, double* dv, double* dzL, double* dzU, double mu, double tau,
                                            bool resto, double zeta, double* amax_io, double* az_io, double* dphi_io, double* bad_io) {
  const size_t o = size_t(bi) * D.nv;
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;    // this workgroup's slice (vec_combine)
  double amax = *amax_io, az = *az_io, dphi = *dphi_io, bad = *bad_io;
  #pragma unroll 4
  for (int i = i0; i < D.nv; i += stride) {
    const double l = D.vl[o + i], u = D.vu[o + i], vi = D.v[o + i], dsol = sol[D.pos[i]], zl = D.zL[o + i], zu = D.zU[o + i];
    // every load ahead of the branches (kept in flight by the unrolling)
    const double gri = resto ? zeta * D.dr2[o + i] * (vi - D.vR[o + i]) : (i < D.n ? D.grad[size_t(bi) * D.n + i] : 0.0);
    double d = 0.0, dl = 0.0, du = 0.0;
    if (l != u) {
      d = dsol;
      if (!(fabs(d) < 1e300)) bad = 1;
      double gphi = gri;
      if (l > -IPM_INF) dl = bound_step(vi - l, zl, d, false, mu, tau, &amax, &az, &gphi);
      if (u < IPM_INF) du = bound_step(u - vi, zu, -d, true, mu, tau, &amax, &az, &gphi);
      dphi += gphi * d;
    }
    dv[o + i] = d;
    dzL[o + i] = dl;
    dzU[o + i] = du;
  }
  *amax_io = amax; *az_io = az; *dphi_io = dphi; *bad_io = bad;
}
// step of the regular iteration: the unknowns' part, dlambda, and the totals over the instance (true on its last workgroup only)
__device__ inline bool newton_step(const IpmDev& D, int bi, const double* sol, double* dv, double* dlam, double* dzL, double* dzU,
                                   double mu, double tau, double* sh, double* amax, double* az, double* dphi, double* bad) {
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  *amax = 1.0; *az = 1.0; *dphi = 0.0; *bad = 0.0;
  newton_step_unknowns(D, bi, sol, dv, dzL, dzU, mu, tau, false, 0.0, amax, az, dphi, bad);
  #pragma unroll 4
  for (int r = i0; r < D.m; r += stride) dlam[size_t(bi) * D.m + r] = sol[D.pos[D.nv + r]];
  return reduce_and_combine(D, bi, sh, red_min(*amax), red_min(*az), red_sum(*dphi), red_max(*bad));
}
__device__ inline double alpha_min23(const IpmOpts& op, double theta, double theta_min, double dphi) {   // (23)
  double amin = op.gamma_theta;
  if (dphi < 0) {
    amin = fmin(amin, op.gamma_phi * theta / (-dphi));
    if (theta <= theta_min) amin = fmin(amin, op.delta * pow(theta, op.s_theta) / pow(-dphi, op.s_phi));
  }
  return op.gamma_alpha * amin;
}

__global__ __launch_bounds__(1024) void ipm_direction_kernel(IpmDev D) {
  __shared__ double sh[16];
  const int bi = blockIdx.y, t = threadIdx.x, i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  IpmInst& S = D.inst[bi];
  const int status = S.status, mode = S.mode;
  const double mu = mode == 2 ? S.mu_r : S.mu, tau = S.tau;
  __syncthreads();              // thread 0 (of the last workgroup, vec_combine) rewrites S.mode below: everybody has read it
  if (status != 0) return;
  const size_t o = size_t(bi) * D.nv, om = size_t(bi) * D.m;
  const double* sol = D.rhs + size_t(bi) * D.Nt;
  if (mode == 3) {              // least-squares multipliers on leaving the restoration; lambda = 0 when they are large (section 3.6)
    double mx = 0.0;
    #pragma unroll 4
    for (int r = i0; r < D.m; r += stride) { const double w = fabs(sol[D.pos[D.nv + r]]); mx = (w < 1e300) ? fmax(mx, w) : 1e300; }   // NaN counts as too large
    if (!reduce_and_combine(D, bi, sh, red_max(mx))) return;
    const bool keep = mx <= D.o.mult_reset;
    #pragma unroll 4
    for (int r = t; r < D.m; r += blockDim.x) D.lam[om + r] = keep ? sol[D.pos[D.nv + r]] : 0.0;
    if (t == 0) { S.mode = 0; S.accepted = 1; S.skip_update = S.skip_update == -1 ? 2 : (S.skip_update == -2 ? 3 : 1); S.ls = 0; S.armijo = 0; S.soc_on = 0; S.soc_req = 0; S.use_soc = 0; }
    return;
  }
  if (mode == 2) {              // restoration: step in (v, lambda) from the reduced system, p and n recovered from it
    const double rho = D.o.resto_rho, zeta = S.zeta;
    double amax = 1.0, az = 1.0, dphi = 0.0, bad = 0.0;
    newton_step_unknowns(D, bi, sol, D.dv, D.dzL, D.dzU, mu, tau, true, zeta, &amax, &az, &dphi, &bad);
    #pragma unroll 4
    for (int r = i0; r < D.m; r += stride) {
      const double pp = D.pp[om + r], nn = D.nn[om + r], zp = D.zp[om + r], zn = D.zn[om + r], lam = D.lam[om + r];
      const double sp = zp / pp, sn = zn / nn, dlam = sol[D.pos[D.nv + r]];
      if (!(fabs(dlam) < 1e300)) bad = 1;
      const double rp = rho - lam - mu / pp, rn = rho + lam - mu / nn;
      const double dp = (dlam - rp) / sp, dn = (-dlam - rn) / sn;
      double gp = rho, gn = rho;              // p and n are bounded below by zero, their objective gradient is rho
      const double dzp = bound_step(pp, zp, dp, false, mu, tau, &amax, &az, &gp), dzn = bound_step(nn, zn, dn, false, mu, tau, &amax, &az, &gn);
      dphi += gp * dp + gn * dn;
      D.dlam[om + r] = dlam; D.dpp[om + r] = dp; D.dnn[om + r] = dn; D.dzp[om + r] = dzp; D.dzn[om + r] = dzn;
    }
    if (!reduce_and_combine(D, bi, sh, red_min(amax), red_min(az), red_sum(dphi), red_max(bad))) return;
    if (t != 0) return;
    if (bad != 0) { S.status = 5; return; }
    S.alpha_max = amax; S.alpha_z = az; S.alpha = amax; S.dphi = dphi;
    S.alpha_min = alpha_min23(D.o, S.th_r, S.thr_min, dphi);
    S.ls = 0; S.accepted = 0; S.armijo = 0; S.soc_on = 0; S.soc_req = 0; S.use_soc = 0;
    atomicAdd(&D.cnt[2], 1);
    return;
  }
  double amax, az, dphi, bad;
  if (!newton_step(D, bi, sol, D.dv, D.dlam, D.dzL, D.dzU, mu, tau, sh, &amax, &az, &dphi, &bad)) return;
  if (t != 0) return;
  if (bad != 0) { S.status = 5; return; }
  S.alpha_max = amax; S.alpha_z = az; S.alpha = amax; S.dphi = dphi;
  S.alpha_min = alpha_min23(D.o, S.theta, S.theta_min, dphi);
  S.ls = 0; S.accepted = 0; S.armijo = 0; S.soc_on = 0; S.soc_req = 0; S.use_soc = 0; S.soc_p = 0;
  atomicAdd(&D.cnt[2], 1);
}

// ---- second-order correction (paper section 2.4, A-5.5 .. A-5.9): the same matrix, c replaced by c_soc = alpha c_soc + c(trial)
__global__ void ipm_soc_rhs_kernel(IpmDev D) {
  const int bi = blockIdx.y;
  const IpmInst& S = D.inst[bi];
  if (S.status != 0 || !S.soc_req) return;
  const size_t o = size_t(bi) * D.nv, om = size_t(bi) * D.m;
  const int stride = gridDim.x * blockDim.x, t0 = blockIdx.x * blockDim.x + threadIdx.x;
  double* rhs = D.rhs + size_t(bi) * D.Nt;
  const bool first = S.soc_p == 0;
  const double mix = first ? S.alpha : S.alpha_soc, mu = S.mu;
  for (int r = t0; r < D.m; r += stride) {
    const double cs = mix * (first ? D.c[om + r] : D.csoc[om + r]) + D.ct[om + r];
    D.csoc[om + r] = cs;
    rhs[D.pos[D.nv + r]] = -cs;
  }
  for (int i = t0; i < D.nv; i += stride) {
    const double l = D.vl[o + i], u = D.vu[o + i];
    double r = 0.0;
    if (l != u) {
      r = D.glag[o + i];
      if (l > -IPM_INF) r -= mu / (D.v[o + i] - l);
      if (u < IPM_INF) r += mu / (u - D.v[o + i]);
    }
    rhs[D.pos[i]] = -r;
  }
}
__global__ __launch_bounds__(1024) void ipm_soc_direction_kernel(IpmDev D) {
  __shared__ double sh[16];
  const int bi = blockIdx.y;
  IpmInst& S = D.inst[bi];
  const int go = S.status == 0 && S.soc_req;
  const double mu = S.mu, tau = S.tau;
  __syncthreads();
  if (!go) return;
  double amax, az, dphi, bad;
  if (!newton_step(D, bi, D.rhs + size_t(bi) * D.Nt, D.dv2, D.dlam2, D.dzL2, D.dzU2, mu, tau, sh, &amax, &az, &dphi, &bad)) return;
  if (threadIdx.x != 0) return;
  S.soc_req = 0;
  if (bad != 0) { S.soc_on = 0; S.alpha = 0.5 * S.alpha; S.ls += 1; return; }   // no usable correction: back to the plain backtracking
  S.alpha_soc = amax; S.az_soc = az;
}

// ------------------------------------------------------------------------------------------------ line search
// Does the filter line search take the trial point (th, phit)?  `theta .. dphi`: infeasibility, its filter bounds, barrier objective
// and slope at the current point; a_test: the step length of the switching / Armijo tests; dominated: by a filter entry; bad: NaN /
// Inf met on the way.  *armijo: it was taken by the Armijo test, as a step that decreases the objective (no filter entry follows, (22)).
__device__ inline bool filter_accepts(const IpmOpts& op, double theta, double theta_min, double theta_max, double phi, double dphi, double th,
                                      double phit, double a_test, bool dominated, double bad, bool* armijo) {
  const double slack = 10.0 * 2.220446049250313e-16 * fabs(phi);     // Ipopt's rounding allowance in the phi comparisons
  *armijo = false;
  if (bad != 0 || !(th <= theta_max) || dominated) return false;
  const bool sw = dphi < 0 && a_test * pow(-dphi, op.s_phi) > op.delta * pow(theta, op.s_theta);   // (19)
  if (theta <= theta_min && sw) return *armijo = phit - phi - op.eta_phi * a_test * dphi <= slack;    // (20)
  return th <= (1.0 - op.gamma_theta) * theta || phit - (phi - op.gamma_phi * theta) <= slack;       // (18)
}
__global__ void ipm_trial_kernel(IpmDev D) {
  const int bi = blockIdx.y;
  const IpmInst& S = D.inst[bi];
  if (S.status != 0 || S.accepted || S.enter_resto) return;   // (enter_resto: its line search gave up in an earlier round)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.n) return;
  const size_t o = size_t(bi) * D.nv + i;
  D.xt[size_t(bi) * D.n + i] = S.soc_on ? D.v[o] + S.alpha_soc * D.dv2[o] : D.v[o] + S.alpha * D.dv[o];
}
// (several workgroups per instance when a few large instances run, vec_combine: the logarithms of 74 k unknowns kept one
// workgroup's issue slots busy for 100 us on the metric problem)
__global__ __launch_bounds__(1024) void ipm_accept_kernel(IpmDev D) {
  __shared__ double sh[16];
  const int bi = blockIdx.y, t = threadIdx.x, i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  IpmInst& S = D.inst[bi];
  // An instance whose line search gave up (enter_resto set) waits for the update like an accepted one: judged again in the rounds
  // that other instances of the batch still need, it would go on halving alpha and counting ls.
  const int go = S.status == 0 && !S.accepted && !S.enter_resto, mode = S.mode, soc = S.soc_on;
  const double a = soc ? S.alpha_soc : S.alpha;
  __syncthreads();
  if (!go) return;
  const size_t o = size_t(bi) * D.nv, om = size_t(bi) * D.m;
  const double* dvp = soc ? D.dv2 : D.dv;
  double th = 0.0, ln = 0.0, bad = 0.0, qd = 0.0, spn = 0.0, lnpn = 0.0;
  const bool resto = mode == 2;
  #pragma unroll 4
  for (int i = i0; i < D.nv; i += stride) {
    const double l = D.vl[o + i], u = D.vu[o + i], vi = D.v[o + i], di = dvp[o + i];   // loads ahead of the branch: the unrolled
    if (l == u) continue;                                                                 // iterations keep 16 of them in flight
    const double vt = vi + a * di;
    if (l > -IPM_INF) ln += log(vt - l);
    if (u < IPM_INF) ln += log(u - vt);
    if (resto) { const double dd = vt - D.vR[o + i]; qd += D.dr2[o + i] * dd * dd; }
  }
  #pragma unroll 4
  for (int r = i0; r < D.m; r += stride) {
    const int s = D.row_slack[r];
    const double gr = D.gt[size_t(bi) * D.sg + r];
    const double glr = D.scal_on ? D.sc[om + r] * D.gl[r] : D.gl[r];
    double cr = s < 0 ? gr - glr : gr - (D.v[o + D.n + s] + a * dvp[o + D.n + s]);
    D.ct[om + r] = cr;
    if (resto) {
      const double pt = D.pp[om + r] + a * D.dpp[om + r], nt = D.nn[om + r] + a * D.dnn[om + r];
      cr += nt - pt;
      spn += pt + nt;
      lnpn += log(pt) + log(nt);
    }
    if (!(fabs(cr) < 1e300)) bad = 1;
    th += fabs(cr);
  }
  if (!reduce_and_combine(D, bi, sh, red_sum(th), red_sum(ln), red_max(bad), red_sum(qd, resto), red_sum(spn, resto),
                          red_sum(lnpn, resto))) return;
  const IpmOpts& op = D.o;
  // is the trial point dominated by a filter entry?  (every thread holds the reduced sums; the entries — hundreds on a long
  // Delta-III solve — are dealt to the threads instead of being walked by thread 0)
  const double phit_all = resto ? op.resto_rho * spn + 0.5 * S.zeta * qd - S.mu_r * (ln + lnpn) : D.objt[bi] - S.mu * ln;
  double dom = 0.0;
  {
    const double* F = (resto ? D.rfilt : D.filt) + size_t(bi) * 2 * IPM_FMAX;
    const int nf = resto ? S.nrfilt : S.nfilt;
    for (int k = t; k < nf; k += blockDim.x)
      if (th >= F[2 * k] && phit_all >= F[2 * k + 1]) dom = 1.0;
  }
  const bool dominated = block_red(dom, 1, sh) != 0.0;
  if (t != 0) return;
  S.th_trial = th; S.phi_trial = phit_all;
  if (resto) {                  // the restoration problem's own filter line search
    if (!(fabs(phit_all) < 1e300)) bad = 1;
    bool armijo;
    const bool ok = filter_accepts(op, S.th_r, S.thr_min, S.thr_max, S.phi_r, S.dphi, th, phit_all, a, dominated, bad, &armijo);
    if (armijo) S.armijo = 1;
    if (ok) { S.accepted = 1; return; }
    S.alpha = 0.5 * a;
    S.ls += 1;
    if (S.alpha < S.alpha_min || S.ls > op.max_ls) { S.status = 3; return; }     // the restoration failed
    atomicAdd(&D.cnt[2], 1);
    return;
  }
  const double ft = D.objt[bi];
  if (!(fabs(ft) < 1e300) || !(fabs(ln) < 1e300)) bad = 1;
  bool armijo;                         // the switching / Armijo tests of a corrected step use the uncorrected step length (A-5.7)
  const bool ok = filter_accepts(op, S.theta, S.theta_min, S.theta_max, S.phi, S.dphi, th, phit_all, S.alpha, dominated, bad, &armijo);
  if (armijo) S.armijo = 1;
  if (ok) {
    S.accepted = 1;
    if (soc) { S.use_soc = 1; S.n_soc += 1; }
    return;
  }
  const bool th_ok = fabs(th) < 1e300 && bad == 0;
  if (soc) {
    if (th_ok && S.soc_p + 1 < op.max_soc && th <= op.kappa_soc * S.th_old_soc) {      // A-5.9: next correction
      S.soc_p += 1; S.th_old_soc = th; S.soc_req = 1;
      atomicAdd(&D.cnt[3], 1);
      return;
    }
    S.soc_on = 0;                                                                       // give up: plain backtracking
  } else if (S.ls == 0 && op.max_soc > 0 && th_ok && th >= S.theta) {                   // A-5.5
    S.soc_on = 1; S.soc_p = 0; S.th_old_soc = S.theta; S.soc_req = 1;
    atomicAdd(&D.cnt[3], 1);
    return;
  }
  S.alpha = 0.5 * S.alpha;
  S.ls += 1;
  if (S.alpha < S.alpha_min || S.ls > op.max_ls) {
    if (S.err0 <= op.acceptable_tol) S.status = 6;             // nothing left to gain: Ipopt reports the acceptable level here too
    else if (op.resto && S.theta > op.tol) S.enter_resto = 1;  // Ipopt switches to its restoration phase here
    else if (op.resto && S.n_recalc < 3) S.enter_resto = 2;    // feasible but the multipliers are off: recompute them (recalc_y)
    else S.status = 3;
    return;
  }
  atomicAdd(&D.cnt[2], 1);
}

// ------------------------------------------------------------------------------------------------ step
// filter entry (22) for the point (theta, phi), while there is room
__device__ inline void filter_append(double* F, int* n, double theta, double phi, const IpmOpts& o) {
  if (*n >= IPM_FMAX) return;
  F[2 * *n] = (1.0 - o.gamma_theta) * theta;
  F[2 * *n + 1] = phi - o.gamma_phi * theta;
  *n += 1;
}
// trace record of the iteration that ends (ls: backtracks; -1 marks a restoration step)
__device__ inline void trace_record(const IpmDev& D, int bi, const IpmInst& S, double mu, double a, double az, double delta_w, double ls) {
  if (!D.trace || S.iter >= D.trace_cap) return;
  double* R = D.trace + (size_t(bi) * D.trace_cap + S.iter) * IPM_TRACE;
  R[0] = S.f; R[1] = S.theta; R[2] = mu; R[3] = a; R[4] = az; R[5] = delta_w; R[6] = S.err0; R[7] = ls;
}
// the accepted step: v += a dv, z += az dz with the reset (16) against mu, lambda += a dlambda (this workgroup's slice)
__device__ inline void apply_step(const IpmDev& D, int bi, const double* dv, const double* dlam, const double* dzL, const double* dzU, double a,
                                  double az, double mu) {
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  const size_t o = size_t(bi) * D.nv, om = size_t(bi) * D.m;
  const double ks = D.o.kappa_sigma;
  #pragma unroll 4
  for (int i = i0; i < D.nv; i += stride) {
    const double l = D.vl[o + i], u = D.vu[o + i], v0 = D.v[o + i], di = dv[o + i];
    const double zl = D.zL[o + i], zu = D.zU[o + i], dl = dzL[o + i], du = dzU[o + i];        // loads ahead of the branch
    if (l == u) continue;
    const double vi = v0 + a * di;
    D.v[o + i] = vi;
    if (l > -IPM_INF) D.zL[o + i] = reset16(zl + az * dl, vi - l, mu, ks);   // (16)
    if (u < IPM_INF) D.zU[o + i] = reset16(zu + az * du, u - vi, mu, ks);
  }
  #pragma unroll 4
  for (int r = i0; r < D.m; r += stride) D.lam[om + r] += a * dlam[om + r];
}
__global__ __launch_bounds__(1024) void ipm_update_kernel(IpmDev D) {
  const int bi = blockIdx.y, t = threadIdx.x, i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  IpmInst& S = D.inst[bi];
  // every thread reads the instance's verdicts BEFORE anybody changes any of them (a late wave must not see enter_resto already
  // cleared, or mode already switched, and skip its slice): the record is only written by thread 0 of the LAST workgroup of the
  // instance to get here (vec_last_arrival)
  const int s_status = S.status, s_enter = S.enter_resto, s_accepted = S.accepted, s_mode = S.mode, s_skip = S.skip_update, s_soc = S.use_soc;
  const double s_alpha = s_soc ? S.alpha_soc : S.alpha, s_alpha_z = s_soc ? S.az_soc : S.alpha_z, s_mu = S.mu, s_mu_r = S.mu_r, s_cinf = S.cinf;
  __syncthreads();
  if (s_status != 0) return;
  const size_t o = size_t(bi) * D.nv, om = size_t(bi) * D.m;
  const double ks = D.o.kappa_sigma;
  if (s_skip) {           // this pass only replaced lambda (least-squares multipliers after the restoration, or recalc_y)
    if (!vec_last_arrival(D, bi)) return;
    if (t == 0) { if (s_skip == 1) S.n_resto += 1; else if (s_skip == 2) S.n_recalc += 1; S.skip_update = 0; }
    return;
  }
  if (s_enter == 2) {     // recalc_y: the next pass computes least-squares multipliers at this point, nothing else
    if (!vec_last_arrival(D, bi)) return;
    if (t == 0) { S.mode = 3; S.enter_resto = 0; S.skip_update = -1; }
    return;
  }
  if (s_enter) {          // the line search gave up at an infeasible point: start the restoration phase from it
    const double rho = D.o.resto_rho, mu_r = fmax(s_mu, s_cinf);
    #pragma unroll 4
    for (int i = i0; i < D.nv; i += stride) {
      const double vi = D.v[o + i], sc = fmax(1.0, fabs(vi));
      D.vR[o + i] = vi;
      D.dr2[o + i] = 1.0 / (sc * sc);
      D.zL[o + i] = fmin(rho, D.zL[o + i]);
      D.zU[o + i] = fmin(rho, D.zU[o + i]);
    }
    #pragma unroll 4
    for (int r = i0; r < D.m; r += stride) {        // (33), (34): the p, n that minimise the restoration's barrier objective at v_R
      const double c = D.c[om + r], h2 = (mu_r - rho * c) / (2.0 * rho);
      const double nn = h2 + sqrt(h2 * h2 + mu_r * c / (2.0 * rho)), pp = c + nn;
      D.nn[om + r] = nn; D.pp[om + r] = pp;
      D.zp[om + r] = mu_r / pp; D.zn[om + r] = mu_r / nn;
      D.lam[om + r] = 0.0;
    }
    if (!vec_last_arrival(D, bi)) return;
    if (t == 0) {
      filter_append(D.filt + size_t(bi) * 2 * IPM_FMAX, &S.nfilt, S.theta, S.phi, D.o);
      S.th0 = S.theta; S.mu_r = mu_r; S.zeta = sqrt(mu_r); S.mode = 2; S.resto_it = 0; S.enter_resto = 0; S.nrfilt = 0;
    }
    return;
  }
  if (!s_accepted) return;
  const double a = s_alpha, az = s_alpha_z;
  if (s_mode == 2) {      // (no second-order correction in the restoration phase: s_soc is 0)
    const double mu = s_mu_r;
    apply_step(D, bi, D.dv, D.dlam, D.dzL, D.dzU, a, az, mu);
    #pragma unroll 4
    for (int r = i0; r < D.m; r += stride) {
      const double pp = D.pp[om + r] + a * D.dpp[om + r], nn = D.nn[om + r] + a * D.dnn[om + r];
      D.pp[om + r] = pp; D.nn[om + r] = nn;
      D.zp[om + r] = reset16(D.zp[om + r] + az * D.dzp[om + r], pp, mu, ks);
      D.zn[om + r] = reset16(D.zn[om + r] + az * D.dzn[om + r], nn, mu, ks);
    }
    if (!vec_last_arrival(D, bi)) return;
    if (t == 0) {
      if (!S.armijo) filter_append(D.rfilt + size_t(bi) * 2 * IPM_FMAX, &S.nrfilt, S.th_r, S.phi_r, D.o);
      trace_record(D, bi, S, S.mu_r, a, az, 0.0, -1.0);
      S.resto_it += 1;
      S.iter += 1;
    }
    return;
  }
  apply_step(D, bi, s_soc ? D.dv2 : D.dv, s_soc ? D.dlam2 : D.dlam, s_soc ? D.dzL2 : D.dzL, s_soc ? D.dzU2 : D.dzU, a, az, s_mu);
  if (!vec_last_arrival(D, bi)) return;
  if (t == 0) {
    if (!S.armijo) filter_append(D.filt + size_t(bi) * 2 * IPM_FMAX, &S.nfilt, S.theta, S.phi, D.o);
    trace_record(D, bi, S, S.mu, a, az, S.delta_w, double(S.ls));
    S.iter += 1;
  }
}


// ------------------------------------------------------------------------------------------------ launchers
// threads per instance of the one-workgroup-per-instance vector kernels: a few large instances (the metric problem: n = 41 k)
// get 16 waves each, a sweep of many small ones 4
static unsigned vec_threads(const IpmDev& D) { return D.B <= 32 && D.nv >= 4096 ? 1024u : 256u; }
// workgroups per instance of the vector kernels that can split an instance (ipm_accept_kernel)
static unsigned vec_blocks(const IpmDev& D) {
  return D.B <= 32 && D.nv >= 4096 ? unsigned(std::min(IPM_VEC_BLOCKS, (std::max(D.nv, D.m) + 1023) / 1024)) : 1u;
}
void ipm_launch_set_state0(const IpmDev& D, int x_state0, int M, int nx, const double* d_state0, hipStream_t st) {
  if (D.B * nx == 0) return;
  hipLaunchKernelGGL(ipm_set_state0_kernel, dim3(unsigned((D.B * nx + 255) / 256)), dim3(256), 0, st, D, x_state0, M, nx, d_state0);
}
void ipm_launch_init(const IpmDev& D, const double* d_x0, hipStream_t st, int warm) {
  hipLaunchKernelGGL(ipm_init_kernel, dim3(unsigned(D.B)), dim3(256), 0, st, D, d_x0, warm);
}
void ipm_launch_init_slack(const IpmDev& D, hipStream_t st, int warm) {
  hipLaunchKernelGGL(ipm_init_slack_kernel, dim3(unsigned(D.B)), dim3(256), 0, st, D, warm);
}
void ipm_launch_warm_duals(const IpmDev& D, const double* d_x0, const double* d_lambda, const double* d_zL, const double* d_zU, hipStream_t st) {
  hipLaunchKernelGGL(ipm_warm_duals_kernel, dim3(unsigned(D.B)), dim3(256), 0, st, D, d_x0, d_lambda, d_zL, d_zU);
}
void ipm_launch_bound_multipliers(const IpmDev& D, double* d_zL, double* d_zU, hipStream_t st) {
  hipLaunchKernelGGL(ipm_bound_mult_kernel, dim3(unsigned((D.n + 255) / 256), unsigned(D.B)), dim3(256), 0, st, D, d_zL, d_zU);
}
void ipm_launch_pack_x(const IpmDev& D, hipStream_t st) {
  hipLaunchKernelGGL(ipm_pack_x_kernel, dim3(unsigned((D.n + 255) / 256), unsigned(D.B)), dim3(256), 0, st, D);
}
void ipm_launch_residual(const IpmDev& D, hipStream_t st) {
  const int tb = (D.nv + 255) / 256;
  hipLaunchKernelGGL(ipm_jt_lambda_kernel, dim3(unsigned(tb + D.n_long), unsigned(D.B)), dim3(256), 0, st, D, tb);
  hipLaunchKernelGGL(ipm_residual_kernel, dim3(vec_blocks(D), unsigned(D.B)), dim3(vec_threads(D)), 0, st, D);
}
void ipm_launch_jt_lambda_into(const IpmDev& D, double* out, hipStream_t st) {
  IpmDev D2 = D;
  D2.glag = out;
  const int tb = (D.nv + 255) / 256;
  hipLaunchKernelGGL(ipm_jt_lambda_kernel, dim3(unsigned(tb + D.n_long), unsigned(D.B)), dim3(256), 0, st, D2, tb);
}
void ipm_launch_direction(const IpmDev& D, hipStream_t st) {
  hipLaunchKernelGGL(ipm_direction_kernel, dim3(vec_blocks(D), unsigned(D.B)), dim3(vec_threads(D)), 0, st, D);
}
void ipm_launch_trial(const IpmDev& D, hipStream_t st) {
  hipLaunchKernelGGL(ipm_trial_kernel, dim3(unsigned((D.n + 255) / 256), unsigned(D.B)), dim3(256), 0, st, D);
}
void ipm_launch_accept(const IpmDev& D, hipStream_t st) {
  hipLaunchKernelGGL(ipm_accept_kernel, dim3(vec_blocks(D), unsigned(D.B)), dim3(vec_threads(D)), 0, st, D);
}
void ipm_launch_update(const IpmDev& D, hipStream_t st) {
  hipLaunchKernelGGL(ipm_update_kernel, dim3(vec_blocks(D), unsigned(D.B)), dim3(vec_threads(D)), 0, st, D);
}
void ipm_launch_soc_rhs(const IpmDev& D, hipStream_t st) {
  const int blocks = std::max(1, std::min(64, (std::max(D.nv, D.m) + 255) / 256));
  hipLaunchKernelGGL(ipm_soc_rhs_kernel, dim3(unsigned(blocks), unsigned(D.B)), dim3(256), 0, st, D);
}
void ipm_launch_soc_direction(const IpmDev& D, hipStream_t st) {
  hipLaunchKernelGGL(ipm_soc_direction_kernel, dim3(vec_blocks(D), unsigned(D.B)), dim3(vec_threads(D)), 0, st, D);
}
// ------------------------------------------------------------------------------------------------ NLP scaling
// Ipopt's GradientScaling (nlp_scaling_method = gradient-based, its default; option nlp_scaling here): at the caller's starting
// point, sf = min(1, gmax / |grad f|_inf) and sc_i = min(1, gmax / |grad c_i|_inf) over the free variables (floor scal_min); the
// solver then works on sf f and sc o c — values scaled in place right after every evaluation — and hands back lambda o sc / sf.
__global__ void ipm_scal_max_kernel(IpmDev D) {      // row maxima into sc, gradient maximum into sf (as bit patterns of non-negative doubles)
  const int bi = blockIdx.y;
  unsigned long long* rmax = reinterpret_cast<unsigned long long*>(D.sc + size_t(bi) * D.m);
  const double* jac = D.jac + size_t(bi) * D.sv;
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  for (int k = i0; k < D.nnz_jac; k += stride)
    if (D.jac_dst[k] >= 0) atomicMax(&rmax[D.jac_row[k]], (unsigned long long)__double_as_longlong(fabs(jac[k])));
  double gm = 0.0;
  for (int i = i0; i < D.n; i += stride)
    if (D.vl[size_t(bi) * D.nv + i] != D.vu[size_t(bi) * D.nv + i]) gm = fmax(gm, fabs(D.grad[size_t(bi) * D.n + i]));
  if (gm > 0.0) atomicMax(reinterpret_cast<unsigned long long*>(D.sf + bi), (unsigned long long)__double_as_longlong(gm));
}
__global__ void ipm_scal_finish_kernel(IpmDev D) {
  const int bi = blockIdx.y;
  const double gmax = D.o.scal_gmax, vmin = D.o.scal_min;
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < D.m; r += gridDim.x * blockDim.x) {
    const double v = D.sc[size_t(bi) * D.m + r];
    D.sc[size_t(bi) * D.m + r] = v > gmax ? fmax(gmax / v, vmin) : 1.0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double v = D.sf[bi];
    D.sf[bi] = v > gmax ? fmax(gmax / v, vmin) : 1.0;
  }
}
__global__ void ipm_scal_apply_kernel(IpmDev D, double* g, double* jac, int jac0, int jac1, double* obj, double* grad) {
  const int bi = blockIdx.y;
  if (D.inst[bi].status != 0) return;
  const double* sc = D.sc + size_t(bi) * D.m;
  const double sf = D.sf[bi];
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  if (g) for (int r = i0; r < D.m; r += stride) g[size_t(bi) * D.sg + r] *= sc[r];
  if (jac) for (int k = jac0 + i0; k < jac1; k += stride) jac[size_t(bi) * D.sv + k] *= sc[D.jac_row[k]];
  if (grad) for (int i = i0; i < D.n; i += stride) grad[size_t(bi) * D.n + i] *= sf;
  if (obj && i0 == 0) obj[bi] *= sf;
}
__global__ void ipm_scal_lambda_kernel(IpmDev D, double* out) {   // lambda o sc / sf: the multipliers of the unscaled rows over the objective's factor
  const int bi = blockIdx.y;
  const double sf = D.sf[bi];
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < D.m; r += gridDim.x * blockDim.x)
    out[size_t(bi) * D.m + r] = D.lam[size_t(bi) * D.m + r] * D.sc[size_t(bi) * D.m + r] / sf;
}
__global__ void ipm_scal_hess_kernel(IpmDev D) {
  const int bi = blockIdx.y;
  if (D.inst[bi].status != 0) return;
  const double sf = D.sf[bi];
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < D.nnz_h; k += gridDim.x * blockDim.x) D.hess[size_t(bi) * D.nnz_h + k] *= sf;
}
static dim3 scal_grid(const IpmDev& D, int n) { return dim3(unsigned(std::max(1, std::min(D.B <= 32 ? 256 : 16, (n + 255) / 256))), unsigned(D.B)); }
void ipm_launch_scaling_factors(const IpmDev& D, hipStream_t st) {
  (void)hipMemsetAsync(D.sc, 0, size_t(D.B) * D.m * sizeof(double), st);
  (void)hipMemsetAsync(D.sf, 0, size_t(D.B) * sizeof(double), st);
  hipLaunchKernelGGL(ipm_scal_max_kernel, scal_grid(D, std::max(D.nnz_jac, D.n)), dim3(256), 0, st, D);
  hipLaunchKernelGGL(ipm_scal_finish_kernel, scal_grid(D, D.m), dim3(256), 0, st, D);
}
void ipm_launch_scale(const IpmDev& D, double* g, double* jac, int jac0, int jac1, double* obj, double* grad, hipStream_t st) {
  const int n = std::max(std::max(g ? D.m : 0, jac ? jac1 - jac0 : 0), std::max(grad ? D.n : 0, 1));
  hipLaunchKernelGGL(ipm_scal_apply_kernel, scal_grid(D, n), dim3(256), 0, st, D, g, jac, jac0, jac1, obj, grad);
}
void ipm_launch_scale_lambda(const IpmDev& D, hipStream_t st) {
  hipLaunchKernelGGL(ipm_scal_lambda_kernel, scal_grid(D, D.m), dim3(256), 0, st, D, D.lam_h);
}
void ipm_launch_scale_hessian(const IpmDev& D, hipStream_t st) {
  hipLaunchKernelGGL(ipm_scal_hess_kernel, scal_grid(D, D.nnz_h), dim3(256), 0, st, D);
}
void ipm_launch_unscale_lambda(const IpmDev& D, double* out, hipStream_t st) {
  hipLaunchKernelGGL(ipm_scal_lambda_kernel, scal_grid(D, D.m), dim3(256), 0, st, D, out);
}

}  // namespace rpm
