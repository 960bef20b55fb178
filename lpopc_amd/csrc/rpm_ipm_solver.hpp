// rpm_ipm_solver.hpp — private to rpm_ipm_solver.hip (create, options, the loop, the solve entry points) and rpm_ipm_debug.hip
// (the test hooks): the solver object behind the rpm_ipm handle and the few helpers both units use.
#pragma once
#include <string>
#include <vector>

#include "rpm_device_internal.hpp"
#include "rpm_ipm_device.hpp"

struct rpm_ipm {
  rpm_engine* eng = nullptr;
  rpm::IpmPlan plan;
  rpm::IpmDev D{};
  std::vector<void*> allocs;
  int* h_cnt = nullptr;           // page-locked mirror of D.cnt
  size_t factor_lds = 0;
  size_t l1_dense_lds = 0;    // LDS of kkt_factor_dense_kernel when every level-1 sub-problem fits its register tiles, else 0
  size_t l2_dense_lds = 0, last_dense_lds = 0;   // the same for the groups of separators and for the last level
  int factor_mt = rpm::IPM_MT;
  std::string err;
  std::vector<rpm::IpmInst> h_inst;
  int total_factorizations = 0, total_iterations = 0, total_trials = 0, total_soc = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // around the factorisation and the substitution of an iteration
  double factor_ms = 0.0, solve_ms = 0.0;
  bool solve_pending = false;
  bool attached = false;
  bool lbfgs = false;            // hessian-approximation = limited-memory (rpm_ipm_lbfgs.hip)
  int lb_iterations = 0;         // iterations of the running solve: an upper bound of the pairs any instance holds
  bool solved = false;           // a solve has finished: D.zL / D.zU hold its bound multipliers (rpm_ipm_get_bound_multipliers)
  double* d_host_form = nullptr; // the host-pointer entry points' device copies of x, lambda, z_L, z_U (B x (3 n + m)), on first use
  ~rpm_ipm() {
    if (attached && eng && eng->e.ipm_attached > 0) eng->e.ipm_attached -= 1;
    for (void* p : allocs) (void)hipFree(p);
    if (h_cnt) (void)hipHostFree(h_cnt);
    for (hipEvent_t e2 : ev)
      if (e2) (void)hipEventDestroy(e2);
  }
};

#define IPM_TRY(h, call)                                                      \
  do {                                                                        \
    hipError_t _s = (call);                                                   \
    if (_s != hipSuccess) {                                                   \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(_s);          \
      return RPM_E_DEVICE;                                                    \
    }                                                                         \
  } while (0)

namespace rpm {

template <class T>
int ipm_alloc(rpm_ipm* h, T** dst, size_t count, const T* src = nullptr) {
  void* p = nullptr;
  IPM_TRY(h, hipMalloc(&p, (count ? count : 1) * sizeof(T)));
  h->allocs.push_back(p);
  *dst = static_cast<T*>(p);
  if (src && count) IPM_TRY(h, hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
  return RPM_OK;
}

inline int launch_check(rpm_ipm* h, const char* what) {
  hipError_t s = hipGetLastError();
  if (s != hipSuccess) {
    h->err = std::string(what) + ": " + hipGetErrorString(s);
    return RPM_E_DEVICE;
  }
  return RPM_OK;
}
inline int factor_and_solve_launch(rpm_ipm* h, hipStream_t st, bool factor, bool solve, int check_status, int forward_done = 0) {
  if (factor) kkt_launch_factor(h->D, h->factor_mt, h->factor_lds, st);
  if (solve) kkt_launch_solve(h->D, check_status, st, forward_done);
  return launch_check(h, "kkt kernels");
}

// The starting point's arrays: x required, and for a warm start lambda too, z_L and z_U together or both NULL.  RPM_OK, or
// RPM_E_INVALID with h->err = "<who>: <need>" resp. "<who>: z_L and z_U are given together or both NULL".
int ipm_check_start_args(rpm_ipm* h, const char* who, const char* need, bool warm, const void* x, const void* lambda, const void* z_L,
                         const void* z_U);
// The launches that precede the iteration loop: bounds, pushed x, (nlp_scaling) the scaling factors, g at the pushed x, slacks and
// the duals — z = 1, lambda = 0 of the cold start, or (warm) the caller's d_lambda and d_zL / d_zU (both NULL: z from mu_init).
int ipm_start(rpm_ipm* h, bool warm, const double* d_x, const double* d_lambda, const double* d_zL, const double* d_zU, hipStream_t st);
// the host-pointer entry points' device block, allocated once and kept (rpm_ipm_solve, rpm_ipm_solve_warm,
// rpm_ipm_get_bound_multipliers, rpm_ipm_debug_start): x (B n), lambda (B m), z_L, z_U (B n each)
int host_form(rpm_ipm* h, double** d_x, double** d_l, double** d_zL, double** d_zU);

}  // namespace rpm
