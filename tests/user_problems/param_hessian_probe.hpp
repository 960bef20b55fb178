// Test functor of the parameter Hessian (tests/test_param_hessian*.py; its long-double twin is in
// tests/_param_hessian_reference.py): two phases, one linkage, NX = 2, NU = 1, NQ = 2, NC = 1.  Polynomials of degree <= 3, no
// libm.  Every callback depends explicitly on time (t, or t0 / tf), on both parameters, and bilinearly on states / controls; the
// linkage is nonlinear in xl, xr, pl, pr — so every kind of entry of the Hessian, the (t, t) and the (p, .) scalars included, is
// non-zero on real data, and every pair of states and controls has curvature in a constraint (x1 x1 in f1; x0 x1 and u u in the
// path), so that a draw with sigma = 0 leaves no stored block analytically zero.  The parenthesised products fix the order of the roundings; the twin forms them in the same order.
#pragma once
#include <hip/hip_runtime.h>
#ifndef RPM_DEV
#define RPM_DEV __device__ __forceinline__
#endif
namespace rpm {

struct UserProblem {
  static constexpr int ID = 100;
  static constexpr int NX = 2, NU = 1, NQ = 2, NC = 1, NE_MAX = 2, NLINK_MAX = 2, NCONST = 0;
  static constexpr bool HAS_ANALYTIC = false;
  template <class CP = const double*>
  RPM_DEV static void dae(int, double t, const double* x, const double* u, const double* p, CP, double* f, double* cp) {
    f[0] = x[1] + (p[0] * t) * x[0];
    f[1] = ((-(p[0] * x[0]) + (p[1] * u[0]) * x[1]) + (t * t) * u[0]) + x[1] * x[1];
    cp[0] = ((x[0] * u[0] + x[0] * x[1]) + u[0] * u[0]) + (p[1] * t) * p[0];
  }
  RPM_DEV static void event(int, double t0, const double* x0, double tf, const double* xf, const double* p, const double*, double* ev) {
    ev[0] = x0[0] * p[0] + t0 * p[1];
    ev[1] = xf[1] * tf + (p[0] * p[1]) * xf[0];
  }
  RPM_DEV static void link(int, int, const double* xl, const double* xr, const double* pl, const double* pr, const double*, int, double* lo) {
    lo[0] = xl[0] * pl[0] - xr[0] * pr[1];
    lo[1] = xl[1] * xr[1] + pl[1] * pr[0];
  }
  RPM_DEV static double mayer(int, double t0, const double* x0, double tf, const double* xf, const double* p, const double*) {
    return ((tf * p[0]) * xf[0] + (p[1] * p[1]) * x0[0]) + t0 * tf;
  }
  RPM_DEV static double lagrange(int, double t, const double* x, const double* u, const double* p, const double*) {
    return (u[0] * u[0] + (p[1] * x[0]) * x[0]) + (t * p[0]) * x[1];
  }
};

}  // namespace rpm
