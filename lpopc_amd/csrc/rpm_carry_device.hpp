// rpm_carry_device.hpp — "the plan at time t", one copy of each rule: the knots of a phase's columns, the natural cubic spline
// through them (LpGuessChecker::spline_interpolation, Core/LpGuessChecker.cpp:208-294, as spline_eval of rpm_setup.cpp writes it)
// and the coordinate a time is evaluated at.  The carry, the shift of a plan, the sampler (rpm_carry_kernels.hip) and the
// roll-out (rpm_rollout_kernels.hip) call what is below; with -ffp-contract=off every caller performs the same operations in the
// same order, so the control the plant sees is the control the shift and the extraction see, bit for bit.
#pragma once
#include "rpm_post_device.hpp"

namespace rpm {

// Dynamic LDS of the spline kernels, offsets in doubles.  Rows are Mp = (N + 1) | 1 doubles apart: the lanes that walk different
// rows in step then sit on different banks (an odd number of doubles is 2 * odd dwords; 32 lanes x 2 dwords cover the 64 banks).
struct CarryLds {
  int Mp;
  int pts;     // [Mp]               the source phase's LGR points
  int tau;     // [TB][Mp]           knots tau_g of every instance
  int mu;      // [TB][Mp]           mu of the forward recurrence: depends on the knots only
  int y;       // [TB * ncols][Mp]   the columns, row = instance * ncols + column
  int c;       // [TB * ncols][Mp]   z of the forward recurrence, overwritten by the second derivatives c
  int total;
  __host__ __device__ constexpr CarryLds(int M, int TB, int ncols)
      : Mp(M | 1), pts(0), tau(Mp), mu(tau + TB * Mp), y(mu + TB * Mp), c(y + TB * ncols * Mp), total(c + TB * ncols * Mp) {}
};
static_assert(CarryLds(65, 8, 16).Mp == 65 && CarryLds(64, 1, 1).Mp == 65 && CarryLds(65, 8, 16).total == 65 * (1 + 16 + 2 * 128),
              "CarryLds: an array overlaps its neighbour or the total changed");

// spline_eval's tail (rpm_setup.cpp): binary search for the knot interval, then A, B as written there.  The search
// halves kr - kl whatever the comparisons say, and its trip count is bounded besides: NaN knots cannot spin it.
struct CarryAt {
  int kl, kr;
  double h, A, B;
};
__device__ __forceinline__ CarryAt carry_locate(double x, const double* xd, int n) {
  int kl = 1, kr = n;
  for (int it = 0; it < 32 && kr - kl > 1; ++it) {
    const int k = (kr + kl) / 2;
    if (xd[k - 1] > x) kr = k; else kl = k;
  }
  const double h = xd[kr - 1] - xd[kl - 1];
  return CarryAt{kl, kr, h, (xd[kr - 1] - x) / h, (x - xd[kl - 1]) / h};
}
// the natural cubic spline there: Cc, Dd as spline_eval writes them
__device__ __forceinline__ double carry_eval(double x, const double* xd, const double* yd, const double* c, int n) {
  const CarryAt p = carry_locate(x, xd, n);
  const double h = p.h, A = p.A, B = p.B;
  const double Cc = (A * A * A - A) * (h * h) / 6.0, Dd = (B * B * B - B) * (h * h) / 6.0;
  return A * yd[p.kl - 1] + B * yd[p.kr - 1] + Cc * c[p.kl - 1] + Dd * c[p.kr - 1];
}
// the same knots and search, the cubic terms dropped: a convex combination, non-negative columns stay non-negative.  A and B
// are rounded separately, so the sum can come out an ulp outside the two knot values (x next to a knot): it is held between
// them, with comparisons a NaN passes through.
__device__ __forceinline__ double carry_eval_linear(double x, const double* xd, const double* yd, int n) {
  const CarryAt p = carry_locate(x, xd, n);
  const double yl = yd[p.kl - 1], yr = yd[p.kr - 1];
  const double lo = yl < yr ? yl : yr, hi = yl < yr ? yr : yl;
  double v = p.A * yl + p.B * yr;
  v = v > hi ? hi : v;
  return v < lo ? lo : v;
}
// into [-1, 1], so that a point past either end of the horizon holds the end value; the comparisons are written so that a NaN
// passes through
__device__ __forceinline__ double carry_clamped(double s) {
  s = s > 1.0 ? 1.0 : s;
  return s < -1.0 ? -1.0 : s;
}
// A shifted evaluation point: tau moved on by dt in the instance's own time, then clamped.
__device__ __forceinline__ double carry_shifted(double tau, double dt, double t0, double tf, double tau_0) {
  const double time_0 = post_time(t0, tf, tau_0), time_N = post_time(t0, tf, 1.0);
  return carry_clamped(tau + 2 * dt / (time_N - time_0));
}
// Knot k of a phase (k == N: the end point tau = 1): 2 (time[k] - time[0]) / (time[N] - time[0]) - 1, fp the phase's LGR points.
__device__ __forceinline__ double carry_knot(double t0, double tf, const double* fp, int N, int k) {
  const double time_k = post_time(t0, tf, k < N ? fp[k] : 1.0);
  const double time_0 = post_time(t0, tf, fp[0]), time_N = post_time(t0, tf, 1.0);
  return 2 * (time_k - time_0) / (time_N - time_0) - 1;
}
// The coordinate of a time t of the problem's clock: the very expression of carry_knot, so t = time[k] gives knot k to the bit;
// then clamped.  tau_0: the phase's first LGR point.
__device__ __forceinline__ double carry_coord(double t, double t0, double tf, double tau_0) {
  const double time_0 = post_time(t0, tf, tau_0), time_N = post_time(t0, tf, 1.0);
  return carry_clamped(2 * (t - time_0) / (time_N - time_0) - 1);
}

// ---- the three stages a workgroup runs between staging its columns and evaluating them.  LDS rows as CarryLds lays them out;
// nb instances, ncols columns each, M = N + 1 knots.  The caller synchronises between the stages. ------------------------------

// 1. every instance's knots; t0tf(bi, &t0, &tf) hands out instance bi's t0 and tf
template <class T0TF>
__device__ __forceinline__ void carry_stage_knots(double* tau, int Mp, const double* fp, int N, int nb, T0TF t0tf) {
  const int M = N + 1;
  for (int idx = threadIdx.x; idx < nb * M; idx += blockDim.x) {
    const int k = idx % M, bi = idx / M;
    double t0, tf;
    t0tf(bi, &t0, &tf);
    tau[bi * Mp + k] = carry_knot(t0, tf, fp, N, k);
  }
}
// 2. wave 0: mu, once per instance.  The other waves: the value at tau = 1 of the rows is_control(r) names, post_spline_end
// through the N points `pts`
template <class IsControl>
__device__ __forceinline__ void carry_stage_mu_and_ends(const double* tau, double* mu, double* ys, const double* pts, int Mp, int N,
                                                         int nb, int ncols, IsControl is_control) {
  const int M = N + 1, tid = threadIdx.x, nt = blockDim.x;
  if (tid < 64) {
    for (int bi = tid; bi < nb; bi += 64) {
      const double* xd = tau + bi * Mp;
      double* m = mu + bi * Mp;
      m[0] = 0.0;
      for (int i = 1; i < M - 1; ++i) {
        const double him1 = xd[i] - xd[i - 1], hi = xd[i + 1] - xd[i];
        const double li = 2 * (xd[i + 1] - xd[i - 1]) - him1 * m[i - 1];
        m[i] = hi / li;
      }
      m[M - 1] = 0.0;
    }
  } else {
    for (int r = tid - 64; r < nb * ncols; r += nt - 64) {
      if (!is_control(r)) continue;
      double* y = ys + r * Mp;
      y[N] = post_spline_end(N, pts, [&](int k) -> double { return y[k]; });
    }
  }
}
// 3. one lane per (instance, column): forward recurrence, back substitution, interior c doubled
__device__ __forceinline__ void carry_stage_second(const double* tau, const double* mu, const double* ys, double* cs, int Mp, int M,
                                                    int rows, int ncols) {
  for (int r = threadIdx.x; r < rows; r += blockDim.x) {
    const double* xd = tau + (r / ncols) * Mp;
    const double* m = mu + (r / ncols) * Mp;
    const double* y = ys + r * Mp;
    double* c = cs + r * Mp;
    double z = 0.0;
    c[0] = 0.0;
    for (int i = 1; i < M - 1; ++i) {
      const double him1 = xd[i] - xd[i - 1], hi = xd[i + 1] - xd[i];
      const double alpha = 3.0 / hi * (y[i + 1] - y[i]) - 3.0 / him1 * (y[i] - y[i - 1]);
      const double li = 2 * (xd[i + 1] - xd[i - 1]) - him1 * m[i - 1];
      z = (alpha - him1 * z) / li;
      c[i] = z;
    }
    c[M - 1] = 0.0;
    double next = 0.0;   // c[j + 1] before its doubling
    for (int j = M - 2; j >= 0; --j) {
      next = c[j] - m[j] * next;
      c[j] = j >= 1 ? 2 * next : next;
    }
  }
}

}  // namespace rpm
