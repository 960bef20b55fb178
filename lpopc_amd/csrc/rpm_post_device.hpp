// rpm_post_device.hpp — the rules of the steps after the NLP solve, one copy of each: solution extraction
// (Nlp2OpConverter::Nlp2OpControl, Core/Nlp2OPConverter.cpp:13-196) and the mesh-error estimate
// (SolutionErrorChecker::CheckSolutionDiffError, Core/LpSolutionError.cpp:112-169).  The one-instance kernels
// (rpm_post_kernels.hip) and the kernels of a whole sweep (rpm_post_kernels.hip, rpm_extract_kernels.hip, rpm_carry_kernels.hip)
// differ in their base pointers, their work split and their reductions' shape; what they compute per node, per entry and per
// partial sum is below.  Everything is __forceinline__ on plain pointers: with -ffp-contract=off every caller performs the same
// operations in the same order, so the routes agree bit for bit.
#pragma once
#include "rpm_device_internal.hpp"

namespace rpm {

// ---- solution extraction ---------------------------------------------------------------------------------------

// result->time at tau (Nlp2OPConverter.cpp:49; tau = 1 gives its last entry, :58)
__device__ __forceinline__ double post_time(double t0, double tf, double tau) { return (tf - t0) * (tau + 1) / 2 + t0; }

// End-point costate of state s, -trans(D(:,N)) * lambda: only the rows of the last mesh interval reach the last column, summed
// in ascending row order.  lp: this phase's multipliers.
__device__ __forceinline__ double post_end_costate(const KParams& K, const PhaseDev& ph, const double* lp, int s) {
  const int N = ph.N;
  const NodeDev last = K.nodes[ph.node0 + N - 1];
  double acc = 0.0;
  for (int r = last.dcol0; r < N; ++r) {
    const NodeDev nr = K.nodes[ph.node0 + r];
    acc += K.dvals[nr.drow_off + nr.dlen - 1] * lp[s * N + r];
  }
  return -acc;
}

struct PostOut {   // one phase's output columns of one instance, each column-major with N + 1 rows
  double *time, *state, *control, *costate, *pathmult, *ham, *mayer;
};

// Row k (k = N: the end point tau = 1) of Nlp2OpControl's arrays for one phase of one instance.  x / lam / consts: the bases
// of the instance's variables, multipliers and constants; u_end / pm_end: the controls and path multipliers splined to tau = 1;
// end_costate(s): the end-point costate, asked for in row N only; lag_k: where the Lagrangian of the row goes (NULL: nowhere).
template <class Prob, class EndCostate>
__device__ __forceinline__ void post_node(const KParams& K, const PhaseDev& ph, int k, const double* __restrict__ x,
                                          const double* __restrict__ lam, const double* consts, const double* u_end,
                                          const double* pm_end, EndCostate end_costate, const PostOut& o, double* lag_k) {
  constexpr int NX = Prob::NX, NU = Prob::NU, NC = Prob::NC;
  constexpr int NXs = NX > 0 ? NX : 1, NUs = NU > 0 ? NU : 1, NCs = NC > 0 ? NC : 1;
  const int N = ph.N, M = N + 1;
  const double t0 = x[ph.x_t0], tf = x[ph.x_t0 + 1];
  const double t = post_time(t0, tf, k < N ? K.points[ph.node0 + k] : 1.0);
  o.time[k] = t;
  double xs[NXs], us[NUs], cst[NXs];
#pragma unroll
  for (int s = 0; s < NX; ++s) {
    xs[s] = x[ph.x_state0 + s * M + k];
    o.state[s * M + k] = xs[s];
  }
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    us[j] = k < N ? x[ph.x_control0 + j * N + k] : u_end[j];             // :53-64
    o.control[j * M + k] = us[j];
  }
  const double* lp = lam + ph.g0;                                       // this phase's multipliers, :73
#pragma unroll
  for (int s = 0; s < NX; ++s) {
    cst[s] = k < N ? -((1 / K.weights[ph.node0 + k]) * lp[s * N + k]) : end_costate(s);   // -(W^-1 lambda), :75-79
    o.costate[s * M + k] = cst[s];
  }
#pragma unroll
  for (int j = 0; j < NC; ++j)   // lambda WITHOUT the phase offset, exactly as Nlp2OPConverter.cpp:88 reads it
    o.pathmult[j * M + k] = k < N ? 2 * ((1 / K.weights[ph.node0 + k]) * lam[N * NX + j * N + k]) / (tf - t0) : pm_end[j];
  double f[NXs], cp[NCs];
  pf_dae<Prob>(ph.phase_num, t, xs, us, x + ph.x_t0 + 2, consts, f, cp);
  const double L = pf_lagrange<Prob>(ph.phase_num, t, xs, us, x + ph.x_t0 + 2, consts);
  double sum = 0.0;
#pragma unroll
  for (int s = 0; s < NX; ++s) {
    const double term = cst[s] * f[s];
    sum = (s == 0) ? term : sum + term;
  }
  o.ham[k] = L + sum;                                                    // :146
  if (lag_k) *lag_k = L;
  if (k == 0) {
    double x0[NXs], xf[NXs];
#pragma unroll
    for (int s = 0; s < NX; ++s) {
      x0[s] = x[ph.x_state0 + s * M];
      xf[s] = x[ph.x_state0 + s * M + N];
    }
    o.mayer[0] = pf_mayer<Prob>(ph.phase_num, t0, x0, tf, xf, x + ph.x_t0 + 2, consts);
  }
}

// lagrange_cost = (tf - t0) * (w . L[0..N-1]) / 2 (:134) as a fixed tree: partial sum t of 256 over k = t (mod 256) in ascending
// k, the halving tree 128 .. 1 over the partial sums (in the kernels: one instance or a tile of them), then the scaling
__device__ __forceinline__ double post_cost_partial(int N, const double* w, const double* lag, int t) {
  double s = 0.0;
  for (int k = t; k < N; k += 256) s += w[k] * lag[k];
  return s;
}
__device__ __forceinline__ double post_cost_scaled(double t0, double tf, double sum) { return (tf - t0) * sum / 2.0; }

// ---- mesh-error estimate ---------------------------------------------------------------------------------------

// One interpolated value on the finer mesh (SolutionInterpolation, LpSolutionError.cpp:46-108): the node's own value where a
// finer point hits a node, else the weighted sum over the interval's `terms` nodes (n + 1 for a state, n for a control).
// Hq: the point's row of the interpolation table, ld doubles between its entries; scale: the row's divisor.
__device__ __forceinline__ double mesh_interp(int hit, const double* Hq, int ld, int terms, const double* col, const double* scale) {
  if (hit >= 0) return col[hit];
  double acc = 0.0;
  for (int j = 0; j < terms; ++j) acc += Hq[j * ld] * col[j];
  return acc / *scale;
}

// The scaled dynamics at one point of the finer mesh (:120-131).  t0, tf: result->time's first and last entries; tt: the
// point in [-1, 1]; Xq / Uq: the interpolated states and controls there; Fq: the NX results.
template <class Prob>
__device__ __forceinline__ void mesh_dynamics(const PhaseDev& ph, double t0, double tf, double tt, const double* Xq, const double* Uq,
                                              const double* params, const double* consts, double* Fq) {
  constexpr int NX = Prob::NX, NU = Prob::NU, NC = Prob::NC;
  constexpr int NXs = NX > 0 ? NX : 1, NUs = NU > 0 ? NU : 1, NCs = NC > 0 ? NC : 1;
  double xs[NXs], us[NUs], f[NXs], cp[NCs];
#pragma unroll
  for (int s = 0; s < NX; ++s) xs[s] = Xq[s];
#pragma unroll
  for (int j = 0; j < NU; ++j) us[j] = Uq[j];
  const double half = (tf - t0) / 2;
  const double t = half * tt + half;   // t0 is not added, LpSolutionError.cpp:124
  pf_dae<Prob>(ph.phase_num, t, xs, us, params, consts, f, cp);
#pragma unroll
  for (int s = 0; s < NX; ++s) Fq[s] = f[s] * ((tf - t0) / 2.0);
}

// Row r of X(start) + A f for state s (:147).  Ar: the row of the interval's n1 x n1 integration matrix (column-major);
// Fs [c * nx + s]: the scaled dynamics; Xs [s]: the interval's first interpolated point.
__device__ __forceinline__ double mesh_integrate(const double* Ar, int n1, const double* Fs, int nx, int s, const double* Xs) {
  double acc = 0.0;
  for (int c = 0; c < n1; ++c) acc += Ar[c * n1] * Fs[c * nx + s];
  return (0.0 + 1.0 * Xs[s]) + acc;
}

// relative_error = |integrated - interpolated| / (1 + max(interpolated(:, s))) (:148-157); den: the column's denominator
__device__ __forceinline__ double mesh_rel_entry(double integ, double fine, double den) { return fabs(integ - fine) / den; }

}  // namespace rpm
