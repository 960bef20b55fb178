// rpm_ipm_solver.hpp — private to rpm_ipm_solver.hip (create, options, the loop, the solve entry points), rpm_ipm_debug.hip
// (the test hooks) and rpm_ipm_sens.hip (solution sensitivities): the solver object behind the rpm_ipm handle, the few helpers both units use and the steps of the solve loop
// (IpmLoop), which the hooks rpm_ipm_debug_pass, rpm_ipm_debug_line_search and rpm_ipm_debug_update run one pass of.
#pragma once
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "rpm_device_internal.hpp"
#include "rpm_ipm_device.hpp"
#include "rpm_ipm_hold.hpp"

namespace rpm {
// what a solve counts (rpm_ipm_get_stats, rpm_ipm_get_kernel_times) and what its loop carries from one step to the next; a solve
// and rpm_ipm_debug_pass start from IpmStats{}, the sensitivities keep a copy and put it back
struct IpmStats {
  int total_iterations = 0, total_factorizations = 0, total_trials = 0, total_soc = 0;
  double factor_ms = 0.0, solve_ms = 0.0;   // inside the factorisation / the substitution kernels (HIP events)
  bool solve_pending = false;    // a substitution's time is read once the line search's first fetch_counts has waited for it
  int lb_iterations = 0;         // iterations of the running solve: an upper bound of the pairs any instance holds
};
}  // namespace rpm

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
  rpm::IpmStats stats;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // around the factorisation and the substitution of an iteration
  bool attached = false;
  bool lbfgs = false;            // hessian-approximation = limited-memory (rpm_ipm_lbfgs.hip)
  rpm::IpmHold hold;             // what the arrays of D hold between two calls: what may be called after what (rpm_ipm_hold.hpp)
  double* d_host_form = nullptr; // the host-pointer entry points' device copies of x, lambda, z_L, z_U (B x (3 n + m)), on first use
  // rpm_ipm_sens.hip: its work space (B x n_par x Nt_alloc right-hand sides), the source table of the last parameter list, the
  // plan's fixed pattern and the host-pointer forms' device block; each on first use, kept, grown only
  struct Sens {
    double *ws = nullptr, *block = nullptr;
    int *table = nullptr, *fixed = nullptr;
    size_t ws_cap = 0, block_cap = 0, table_cap = 0;
    int n_groups = 0;
    std::vector<int> var_index;    // the list `table` was built for
    // option "sens_refine" (rounds of iterative refinement of the columns, 0 = none): the rows of the KKT matrix by source
    // (ptr, position, then per entry a source code and the position of its column), a copy of the right-hand sides, the residuals
    int refine = -1;               // -1 automatic: 2 rounds on an exact-parameters engine with static parameters, else none
    int *rows = nullptr;
    int n_rows = 0, n_ent = 0;
    double *rhs0 = nullptr, *res = nullptr;
    size_t rhs0_cap = 0, res_cap = 0;
    // sensitivities to the instances' constants: option "sens_constant_step" (rho of h = rho (1 + |c_k|)), the column table of the
    // plan (IpmConstTable, flat, once per solver), and the scratch of one constant, which serves every constant of a call in
    // turn: the perturbed constants c+ | c- (B x nconst each) and the steps h (B), grad f | g at c+ and at c- (B x (n + sg)
    // each, with a B-long tail the objective values land in), the Jacobian at c+ and at c- (B x sv each)
    double const_step = 1e-5;
    int *ctable = nullptr;
    int c_free = 0, c_ent = 0;
    double *cpm = nullptr, *eval_p = nullptr, *eval_m = nullptr, *jac_p = nullptr, *jac_m = nullptr;
    size_t cpm_cap = 0, eval_p_cap = 0, eval_m_cap = 0, jac_p_cap = 0, jac_m_cap = 0;
  } sens;
  ~rpm_ipm() {
    if (attached && eng && eng->e.ipm_attached > 0) eng->e.ipm_attached -= 1;
    for (void* p : allocs) (void)hipFree(p);
    for (void* p : {static_cast<void*>(sens.ws), static_cast<void*>(sens.block), static_cast<void*>(sens.table), static_cast<void*>(sens.fixed),
                    static_cast<void*>(sens.rows), static_cast<void*>(sens.rhs0), static_cast<void*>(sens.res),
                    static_cast<void*>(sens.ctable), static_cast<void*>(sens.cpm), static_cast<void*>(sens.eval_p),
                    static_cast<void*>(sens.eval_m), static_cast<void*>(sens.jac_p), static_cast<void*>(sens.jac_m)})
      if (p) (void)hipFree(p);
    if (h_cnt) (void)hipHostFree(h_cnt);
    for (hipEvent_t e2 : ev)
      if (e2) (void)hipEventDestroy(e2);
  }
};

#define IPM_TRY(h, call)                                                                             \
  do {                                                                                               \
    hipError_t _s = (call);                                                                          \
    if (_s != hipSuccess) return rpm::ipm_refuse((h), RPM_E_DEVICE, #call, hipGetErrorString(_s)); \
  } while (0)

namespace rpm {

// every refusal and every failure: `code` with h->err = "<who>: <why>" (who empty: the bare <why>)
inline int ipm_refuse(rpm_ipm* h, int code, const std::string& who, const std::string& why) {
  h->err = who.empty() ? why : who + ": " + why;
  return code;
}
// what a call into the engine returned, passed on: its text goes with a failure
inline int ipm_eng_fail(rpm_ipm* h, int rc) {
  if (rc) h->err = h->eng->e.err;
  return rc;
}

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
  const hipError_t s = hipGetLastError();
  return s == hipSuccess ? RPM_OK : ipm_refuse(h, RPM_E_DEVICE, what, hipGetErrorString(s));
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

inline int ipm_abi_status(int device_status) {   // IpmInst::status -> rpm_hip.h: 0 converged, 1 converged to the acceptable level
  return device_status == 1 ? 0 : (device_status == 6 ? 1 : device_status);
}

// ---- reading state back to the host and editing it there (the test hooks, the sensitivities).  Pageable copies on the solver's
// stream, which the caller or the helper synchronises; not the solve's path.
inline hipStream_t ipm_stream(rpm_ipm* h) { return static_cast<hipStream_t>(dev_stream(h->eng->e)); }

// B rows of `width` doubles, `pitch` apart on the device, packed into dst; a NULL dst or an empty row is skipped.  Blocking.
inline hipError_t ipm_rows(const IpmDev& D, double* dst, const double* src, size_t width, size_t pitch) {
  if (!dst || !width) return hipSuccess;
  return hipMemcpy2D(dst, width * sizeof(double), src, pitch * sizeof(double), width * sizeof(double), size_t(D.B), hipMemcpyDeviceToHost);
}

// KKT order -> unknown order through the plan's permutation: out is B x P x Nt, its row (bi, k) is row k B + bi of kkt (rows of
// Nt_alloc) — the layout of the sensitivities' work space; with P = 1 that of D.rhs
inline void ipm_from_kkt_order(const IpmPlan& p, size_t B, size_t P, const double* kkt, double* out) {
  for (size_t r = 0; r < B * P; ++r)
    for (size_t a = 0; a < size_t(p.Nt); ++a) out[r * p.Nt + a] = kkt[((r % P) * B + r / P) * p.Nt_alloc + size_t(p.pos[a])];
}
// the same from the device: d_kkt down on the solver's stream, synchronised, then permuted
inline int ipm_download_unknown_order(rpm_ipm* h, const double* d_kkt, size_t P, double* out) {
  std::vector<double> w(size_t(h->D.B) * P * size_t(h->plan.Nt_alloc));
  IPM_TRY(h, hipMemcpyAsync(w.data(), d_kkt, w.size() * sizeof(double), hipMemcpyDeviceToHost, ipm_stream(h)));
  IPM_TRY(h, hipStreamSynchronize(ipm_stream(h)));
  ipm_from_kkt_order(h->plan, size_t(h->D.B), P, w.data(), out);
  return RPM_OK;
}

// the instance records: down (synchronised), up (queued: `inst` outlives the caller's next synchronise), both around edit(bi, record)
inline int ipm_download_records(rpm_ipm* h, std::vector<IpmInst>& inst) {
  inst.resize(size_t(h->D.B));
  IPM_TRY(h, hipMemcpyAsync(inst.data(), h->D.inst, inst.size() * sizeof(IpmInst), hipMemcpyDeviceToHost, ipm_stream(h)));
  IPM_TRY(h, hipStreamSynchronize(ipm_stream(h)));
  return RPM_OK;
}
inline int ipm_upload_records(rpm_ipm* h, const std::vector<IpmInst>& inst) {
  IPM_TRY(h, hipMemcpyAsync(h->D.inst, inst.data(), inst.size() * sizeof(IpmInst), hipMemcpyHostToDevice, ipm_stream(h)));
  return RPM_OK;
}
template <class F>
int ipm_edit_records(rpm_ipm* h, std::vector<IpmInst>& inst, F edit) {
  if (int rc = ipm_download_records(h, inst)) return rc;
  for (size_t bi = 0; bi < inst.size(); ++bi) edit(bi, inst[bi]);
  return ipm_upload_records(h, inst);
}

// level 1 left to the fill kernel while this lives (IpmDev::df_on off): the launches in its scope work on what is in the storage
struct IpmFusedFillOff {
  IpmDev& D;
  const int keep;
  explicit IpmFusedFillOff(IpmDev& d) : D(d), keep(d.df_on) { D.df_on = 0; }
  ~IpmFusedFillOff() { D.df_on = keep; }
};

// ---- one solve: the steps of an iteration, in the order ipm_solve_dev takes them (rpm_ipm_debug_pass runs the first of them on an
// injected state: the same members, no launch sequence of its own)
struct IpmLoop {
  rpm_ipm* h;
  Engine& e;
  IpmDev& D;
  hipStream_t st;
  bool scal;     // nlp_scaling is on

  int fetch_counts() const {
    IPM_TRY(h, hipMemcpyAsync(h->h_cnt, D.cnt, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    IPM_TRY(h, hipStreamSynchronize(st));
    return RPM_OK;
  }
  // f, grad f, g, the Jacobian and the optimality residual at the current iterate; h_cnt[0]: instances still running
  int evaluate_and_residual() const {
    int rc;
    ipm_launch_pack_x(D, st);
    if ((rc = dev_eval_obj(e, D.xe, D.obj, D.grad, st))) return ipm_eng_fail(h, rc);
    // D.jac is this solver's own array, written by the tile kernel only: its constant Doffdiag block (55 % of the metric
    // problem's Jacobian) is written by the first evaluation of a solve and left alone afterwards (flag 16)
    if ((rc = dev_eval_cons(e, D.xe, D.g, D.jac, 3 | 4 | 16, st))) return ipm_eng_fail(h, rc);
    // (without the scaling's own evaluation the first pass of a solve writes the constant block too: then all of D.jac is scaled)
    if (scal) ipm_launch_scale(D, D.g, D.jac, 0, D.nnz_var, D.obj, D.grad, st);
    IPM_TRY(h, hipMemsetAsync(D.cnt, 0, 4 * sizeof(int), st));
    ipm_launch_residual(D, st);
    if (h->lbfgs) lb_launch_update(D, st);     // the pair of the step just taken (grad_x L at the new point is in D.glag)
    return fetch_counts();
  }
  int exact_hessian() const {
    if (scal) ipm_launch_scale_lambda(D, st);            // sf (H_f + sum (lambda_i sc_i / sf) H_ci)
    if (int rc = dev_eval_h(e, D.xe, 1.0, scal ? D.lam_h : D.lam, D.hess, st)) return ipm_eng_fail(h, rc);
    if (scal) ipm_launch_scale_hessian(D, st);
    return RPM_OK;
  }
  // assemble and factor until no instance asks for another delta_w (Algorithm IC)
  int factor_with_inertia_correction() const {
    int rc;
    for (int tries = 0; tries < 80; ++tries) {
      IPM_TRY(h, hipMemsetAsync(D.cnt + 1, 0, sizeof(int), st));
      ipm_launch_assemble(D, std::max(e.nnz_jac, e.nnz_h), st);
      IPM_TRY(h, hipEventRecord(h->ev[0], st));
      if ((rc = factor_and_solve_launch(h, st, true, false, 1))) return rc;
      IPM_TRY(h, hipEventRecord(h->ev[1], st));
      ipm_launch_inertia(D, st);
      h->stats.total_factorizations += 1;
      if ((rc = fetch_counts())) return rc;
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, h->ev[0], h->ev[1]) == hipSuccess) h->stats.factor_ms += ms;
      if (h->h_cnt[1] == 0) break;
    }
    return RPM_OK;
  }
  int substitute() const {
    IPM_TRY(h, hipEventRecord(h->ev[2], st));
    if (h->lbfgs && h->stats.lb_iterations > 0) {
      // Z = K0^-1 E with the factors in place (all columns of all instances in one pass), then C = M - E'Z
      lb_launch_columns_and_solve(D, st);
      lb_launch_small(D, st);
    }
    if (int rc = factor_and_solve_launch(h, st, false, true, 1, 1)) return rc;   // (the right-hand side the factorisation was given)
    if (h->lbfgs) lb_launch_correct(D, 1, st);
    IPM_TRY(h, hipEventRecord(h->ev[3], st));
    h->stats.solve_pending = true;   // its time is read once the line search's first fetch_counts has waited for it
    return RPM_OK;
  }
  // the step, then rounds: every pending instance evaluates one trial point per round — its next backtracking step, or the next
  // second-order correction (right-hand side, substitution with the factors in place, step lengths) where one was asked for
  int direction() const {
    IPM_TRY(h, hipMemsetAsync(D.cnt + 2, 0, 2 * sizeof(int), st));
    ipm_launch_direction(D, st);
    h->h_cnt[3] = 0;
    return RPM_OK;
  }
  // one round: the corrections that were asked for, the trial points, their evaluation and the verdicts; h_cnt[2] / h_cnt[3] then
  // hold the line searches still pending and the corrections asked for next.  soc_rhs_copy (the test hook's; B x Nt_alloc on the
  // host, KKT order): the corrections' right-hand sides before the substitution overwrites them — a copy, no launch.
  int line_search_round(double* soc_rhs_copy = nullptr) const {
    int rc;
    if (h->h_cnt[3] > 0) {
      ipm_launch_soc_rhs(D, st);
      if (soc_rhs_copy)
        IPM_TRY(h, hipMemcpyAsync(soc_rhs_copy, D.rhs, size_t(D.B) * size_t(h->plan.Nt_alloc) * sizeof(double), hipMemcpyDeviceToHost, st));
      if ((rc = factor_and_solve_launch(h, st, false, true, 2))) return rc;
      if (h->lbfgs) lb_launch_correct(D, 2, st);
      ipm_launch_soc_direction(D, st);
      h->stats.total_soc += 1;
    }
    ipm_launch_trial(D, st);
    if ((rc = dev_eval_obj(e, D.xt, D.objt, nullptr, st))) return ipm_eng_fail(h, rc);
    if ((rc = dev_eval_cons(e, D.xt, D.gt, nullptr, 1 | 4, st))) return ipm_eng_fail(h, rc);
    if (scal) ipm_launch_scale(D, D.gt, nullptr, 0, 0, D.objt, nullptr, st);
    IPM_TRY(h, hipMemsetAsync(D.cnt + 2, 0, 2 * sizeof(int), st));
    ipm_launch_accept(D, st);
    h->stats.total_trials += 1;
    if ((rc = fetch_counts())) return rc;
    if (h->stats.solve_pending) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, h->ev[2], h->ev[3]) == hipSuccess) h->stats.solve_ms += ms;
      h->stats.solve_pending = false;
    }
    return RPM_OK;
  }
  bool line_search_over() const { return h->h_cnt[2] == 0 && h->h_cnt[3] == 0; }
  int line_search() const {
    int rc;
    if ((rc = direction())) return rc;
    for (int ls = 0; ls <= D.o.max_ls + D.o.max_soc + 2; ++ls) {
      if ((rc = line_search_round())) return rc;
      if (line_search_over()) break;
    }
    return RPM_OK;
  }
  int update() const {
    ipm_launch_update(D, st);
    if (h->lbfgs) {
      ipm_launch_jt_lambda_into(D, D.lb_gold, st);   // grad_x L(x_old, lambda_new): D.grad / D.jac still belong to the old iterate
      h->stats.lb_iterations += 1;
    }
    return launch_check(h, "ipm iteration");
  }
  // x back into the caller's array, multipliers, per-instance verdicts
  int collect(double* d_x, double* d_lambda, double* d_zL, double* d_zU, double* obj, int* status, int* iterations, double* kkt_error) const {
    const size_t B = size_t(D.B);
    ipm_launch_pack_x(D, st);
    IPM_TRY(h, hipMemcpyAsync(d_x, D.xe, B * D.n * sizeof(double), hipMemcpyDeviceToDevice, st));
    std::vector<double> sf_host;
    if (d_lambda) {
      if (scal) ipm_launch_unscale_lambda(D, d_lambda, st);     // the multipliers of the caller's (unscaled) rows
      else IPM_TRY(h, hipMemcpyAsync(d_lambda, D.lam, B * D.m * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    if (d_zL && d_zU) ipm_launch_bound_multipliers(D, d_zL, d_zU, st);
    if (scal) {
      sf_host.resize(B);
      IPM_TRY(h, hipMemcpyAsync(sf_host.data(), D.sf, B * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    IPM_TRY(h, hipMemcpyAsync(h->h_inst.data(), D.inst, B * sizeof(IpmInst), hipMemcpyDeviceToHost, st));
    IPM_TRY(h, hipStreamSynchronize(st));
#ifdef IPM_TIMING
    fprintf(stderr, "last factorisation of instance 0, phase clocks [100 MHz ticks]: T %lld  k-loop %lld  diag %lld  panel %lld  corner %lld  tail %lld | dense level 1, diagonal wave: waiting %lld  factoring %lld\n",
            h->h_inst[0].dbg[0], h->h_inst[0].dbg[1], h->h_inst[0].dbg[2], h->h_inst[0].dbg[3], h->h_inst[0].dbg[4], h->h_inst[0].dbg[5], h->h_inst[0].dbg[6], h->h_inst[0].dbg[7]);
#endif
    for (size_t bi = 0; bi < B; ++bi) {
      const IpmInst& S = h->h_inst[bi];
      if (obj) obj[bi] = scal ? S.f / sf_host[bi] : S.f;
      if (status) status[bi] = ipm_abi_status(S.status);
      if (iterations) iterations[bi] = S.iter;
      if (kkt_error) kkt_error[bi] = S.err0;
    }
    h->hold.solve_ends();
    return RPM_OK;
  }
};
inline IpmLoop ipm_loop(rpm_ipm* h) { return IpmLoop{h, h->eng->e, h->D, ipm_stream(h), h->D.scal_on != 0}; }

}  // namespace rpm
