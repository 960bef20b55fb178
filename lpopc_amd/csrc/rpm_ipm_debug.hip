// rpm_ipm_debug.hip — row f-2, the test hooks of the C ABI: the production launchers of the factorisation, the limited-memory
// kernels and the start of a solve on the caller's data (no kernel of their own), and the plan's permutation and slots.
#include <cstring>
#include <vector>

#include "rpm_ipm_solver.hpp"

using namespace rpm;

namespace {
// Factor and solve the caller's matrices: fresh instance records that ask for a factorisation, `store` (B x storage doubles) and
// `rhs` (B x rhs_len, KKT order) up, the kernels on what is in the storage (not on the solver's own matrix: df_on off), the
// solutions back into `rhs` and the instance records into `inst`.  limited_memory: K = K0 - E M^-1 E' the way an iteration solves
// it (Z = K0^-1 E and C = M - E'Z after the factorisation, the Woodbury correction after the substitution, check_status 1);
// otherwise the plain factor + solve of every instance, then the pivot signs summed into the records.
int debug_factor_solve(rpm_ipm* h, const double* store, double* rhs, size_t rhs_len, bool limited_memory, std::vector<IpmInst>& inst) {
  IpmDev& D = h->D;
  hipStream_t st = ipm_stream(h);
  const size_t B = size_t(D.B);
  h->hold.overwritten();
  inst.assign(B, IpmInst{});
  for (IpmInst& s : inst) s.refactor = 1;
  int rc = ipm_upload_records(h, inst);
  if (rc) return rc;
  IPM_TRY(h, hipMemcpyAsync(D.K, store, B * size_t(h->plan.storage()) * sizeof(double), hipMemcpyHostToDevice, st));
  IPM_TRY(h, hipMemcpyAsync(D.rhs, rhs, B * rhs_len * sizeof(double), hipMemcpyHostToDevice, st));
  {
    const IpmFusedFillOff on_the_storage(D);
    if (limited_memory) {
      kkt_launch_factor(D, h->factor_mt, h->factor_lds, st);
      lb_launch_columns_and_solve(D, st);
      lb_launch_small(D, st);
      kkt_launch_solve(D, 1, st);
      lb_launch_correct(D, 1, st);
      rc = launch_check(h, "limited-memory solve");
    } else {
      rc = factor_and_solve_launch(h, st, true, true, 0);
      if (!rc) ipm_launch_inertia(D, st);
    }
  }
  if (rc) return rc;
  IPM_TRY(h, hipMemcpyAsync(rhs, D.rhs, B * rhs_len * sizeof(double), hipMemcpyDeviceToHost, st));
  return ipm_download_records(h, inst);
}

// the same for right-hand sides (B x Nt) and solutions in unknown order: into KKT order (B x Nt_alloc) and back
int debug_factor_solve_unknown_order(rpm_ipm* h, const std::vector<double>& store, const double* rhs, double* sol, bool limited_memory,
                                     std::vector<IpmInst>& inst) {
  const IpmPlan& p = h->plan;
  const size_t B = size_t(h->D.B);
  std::vector<double> r(B * size_t(p.Nt_alloc), 0.0);
  for (size_t bi = 0; bi < B; ++bi)
    for (size_t a = 0; a < size_t(p.Nt); ++a) r[bi * p.Nt_alloc + p.pos[a]] = rhs[bi * p.Nt + a];
  if (int rc = debug_factor_solve(h, store.data(), r.data(), size_t(p.Nt_alloc), limited_memory, inst)) return rc;
  ipm_from_kkt_order(p, B, 1, r.data(), sol);
  return RPM_OK;
}
void pivot_signs(const std::vector<IpmInst>& inst, int* n_pos, int* n_neg) {
  for (size_t bi = 0; bi < inst.size(); ++bi) {
    if (n_pos) n_pos[bi] = inst[bi].npos;
    if (n_neg) n_neg[bi] = inst[bi].nneg;
  }
}
// the instance record as the hooks hand it out: every field up to n_recalc in declaration order, then the trial point's theta and
// phi; ic_hot and dbg left out (the order is documented in rpm_hip.h and named in lpopc_amd/_abi.py: IPM_RECORD_FIELDS)
void flat_record(const IpmInst& S, double* r) {
  const double v[] = {S.mu, S.tau, S.f, S.theta, S.lnsum, S.dinf, S.cinf, S.comp_max, S.comp_min, S.sum_lam, S.sum_z, S.err0,
                      S.delta_w, S.delta_w_last, S.alpha_max, S.alpha_z, S.alpha, S.alpha_min, S.dphi, S.phi, S.theta_max, S.theta_min,
                      double(S.status), double(S.iter), double(S.nfilt), double(S.accepted), double(S.refactor), double(S.npos),
                      double(S.nneg), double(S.nbad), double(S.ls), double(S.armijo), double(S.nzb), double(S.pad),
                      double(S.mode), double(S.resto_it), double(S.enter_resto), double(S.n_resto), double(S.n_acc), double(S.skip_update),
                      S.th0, S.zeta, S.mu_r, S.th_r, S.thr_max, S.thr_min, S.phi_r,
                      double(S.nrfilt), double(S.soc_on), double(S.soc_req), double(S.soc_p), double(S.use_soc), double(S.n_soc),
                      S.alpha_soc, S.az_soc, S.th_old_soc, S.mu_max, S.refs[0], S.refs[1], S.refs[2], S.refs[3],
                      double(S.fixed_mode), double(S.nrefs), double(S.n_recalc), S.th_trial, S.phi_trial};
  static_assert(sizeof(v) / sizeof(v[0]) == RPM_IPM_RECORD_DOUBLES, "RPM_IPM_RECORD_DOUBLES");
  std::memcpy(r, v, sizeof(v));
}
// the instance records down into `inst` and, flattened, into `record` (NULL: not wanted)
int download_flat_records(rpm_ipm* h, std::vector<IpmInst>& inst, double* record) {
  if (int rc = ipm_download_records(h, inst)) return rc;
  for (size_t bi = 0; record && bi < inst.size(); ++bi) flat_record(inst[bi], record + bi * RPM_IPM_RECORD_DOUBLES);
  return RPM_OK;
}
int no_slot(rpm_ipm* h, const char* who, long long a, long long c) {
  return ipm_refuse(h, RPM_E_INVALID, who, "entry (" + std::to_string(a) + ", " + std::to_string(c) + ") has no slot in the layout");
}
}  // namespace

extern "C" {

/* test hook: factor + solve the caller's matrices (B x storage doubles in the band + border layout, lower triangle)
 * against B right-hand sides in KKT order; returns the solutions and the signs of D */
int rpm_ipm_debug_solve(rpm_ipm* h, const double* k_storage, const double* rhs, double* sol, int* n_pos, int* n_neg) {
  if (!h || !k_storage || !rhs || !sol) return RPM_E_INVALID;
  const IpmPlan& p = h->plan;
  if (p.nd) return ipm_refuse(h, RPM_E_UNSUPPORTED, "", "rpm_ipm_debug_solve takes the band + border storage; with nested dissection use rpm_ipm_debug_solve_dense");
  std::vector<IpmInst> inst;
  std::memcpy(sol, rhs, size_t(h->D.B) * p.Nt * sizeof(double));
  int rc = debug_factor_solve(h, k_storage, sol, size_t(p.Nt), false, inst);
  if (rc) return rc;
#ifdef IPM_TIMING
  fprintf(stderr, "factor phases of instance 0 [100 MHz ticks]: T %lld  k-loop %lld  diag %lld  panel %lld  corner %lld  tail %lld\n",
          inst[0].dbg[0], inst[0].dbg[1], inst[0].dbg[2], inst[0].dbg[3], inst[0].dbg[4], inst[0].dbg[5]);
#endif
  pivot_signs(inst, n_pos, n_neg);
  return RPM_OK;
}

/* test hook, layout-independent: factor + solve the caller's DENSE symmetric matrices (B x Nt x Nt, row-major, rows and columns
 * in unknown order: [0,n) variables, slacks, multipliers) against B right-hand sides (unknown order); entries the layout has
 * no slot for must be zero (RPM_E_INVALID otherwise).  Works for the band + border layout and for nested dissection. */
int rpm_ipm_debug_solve_dense(rpm_ipm* h, const double* k_dense, const double* rhs, double* sol, int* n_pos, int* n_neg) {
  if (!h || !k_dense || !rhs || !sol) return RPM_E_INVALID;
  const IpmPlan& p = h->plan;
  const size_t B = size_t(h->D.B), Nt = size_t(p.Nt);
  std::vector<double> store(B * size_t(p.storage()), 0.0);
  for (size_t bi = 0; bi < B; ++bi)
    for (size_t a = 0; a < Nt; ++a)
      for (size_t c = 0; c <= a; ++c) {
        const double v = k_dense[(bi * Nt + a) * Nt + c];
        if (v == 0.0) continue;
        const long long o = ipm_plan_offset(p, int(a), int(c));
        if (o < 0) return no_slot(h, "rpm_ipm_debug_solve_dense", (long long)a, (long long)c);
        store[bi * size_t(p.storage()) + size_t(o)] = v;
      }
  std::vector<IpmInst> inst;
  int rc = debug_factor_solve_unknown_order(h, store, rhs, sol, false, inst);
  if (rc) return rc;
#ifdef IPM_TIMING
  // kkt_factor_dense_kernel (build with -DIPM_TIMING_SUB=<out of range>): tile wave 0 and the diagonal wave of interval block 0
  fprintf(stderr, "level-1 phases of instance 0 [100 MHz ticks]: panel %lld  wait B3 %lld  next diagonal tile + B1 %lld  update %lld  wait B2 %lld  early block columns %lld | diagonal wave: waiting %lld  factoring %lld\n",
          inst[0].dbg[0], inst[0].dbg[1], inst[0].dbg[2], inst[0].dbg[3], inst[0].dbg[4], inst[0].dbg[5], inst[0].dbg[6], inst[0].dbg[7]);
  // kkt_factor_kernel (-DIPM_TIMING_SUB=<sub-problem>): the same record read as the left-looking kernel's phases
  fprintf(stderr, "left-looking phases of instance 0 [100 MHz ticks]: T %lld  k-loop %lld  diag %lld  panel %lld  corner %lld  tail %lld\n",
          inst[0].dbg[0], inst[0].dbg[1], inst[0].dbg[2], inst[0].dbg[3], inst[0].dbg[4], inst[0].dbg[5]);
#endif
  pivot_signs(inst, n_pos, n_neg);
  return RPM_OK;
}

/* storage offset of the entry between unknowns ua and uc (unknown order as above), -1 if the layout has no slot for it */
int rpm_ipm_debug_slot(rpm_ipm* h, int ua, int uc, long long* offset) {
  if (!h || !offset || ua < 0 || uc < 0 || ua >= h->plan.Nt || uc >= h->plan.Nt) return RPM_E_INVALID;
  *offset = ipm_plan_offset(h->plan, ua, uc);
  return RPM_OK;
}

/* test hook, read-only: D.K of every instance as it stands (B x storage doubles) — the factors after the factor hooks or a stage-3
 * pass.  No launch, no change of what the solver holds. */
int rpm_ipm_debug_storage(rpm_ipm* h, double* k_storage) {
  if (!h || !k_storage) return RPM_E_INVALID;
  IPM_TRY(h, hipStreamSynchronize(ipm_stream(h)));
  IPM_TRY(h, hipMemcpy(k_storage, h->D.K, size_t(h->D.B) * size_t(h->plan.storage()) * sizeof(double), hipMemcpyDeviceToHost));
  return RPM_OK;
}

/* KKT position of every unknown ([0,n) variables, then the slacks, then the m multipliers) — for tests and tools */
int rpm_ipm_get_permutation(rpm_ipm* h, int* pos, int capacity) {
  if (!h || !pos || capacity < h->plan.Nt) return RPM_E_INVALID;
  std::memcpy(pos, h->plan.pos.data(), sizeof(int) * h->plan.Nt);
  return RPM_OK;
}

/* test hooks of the limited-memory kernels (rpm_ipm_lbfgs.hip): the production launchers on the caller's data, no kernel of
 * their own.  RPM_E_UNSUPPORTED on a solver created with the exact Hessian. */
/* One pass of the solve loop between ipm_launch_residual and fetch_counts: x (B x n) into the first n entries of every row of
 * D.v, glag_new into D.glag, glag_old into D.lb_gold, mode / status (B ints, NULL = 0) into the instance records, then
 * lb_launch_update.  reset != 0: ipm_launch_init first (vl / vu from the solver's bounds, fresh instance records), then
 * lb_launch_reset; the first call of a sequence has to reset.  x at fixed variables is the caller's to keep at the bound. */
int rpm_ipm_debug_lbfgs_step(rpm_ipm* h, int reset, const double* x, const double* glag_new, const double* glag_old, const int* mode,
                             const int* status) {
  if (!h || !x || !glag_new || !glag_old) return RPM_E_INVALID;
  if (!h->lbfgs) return ipm_refuse(h, RPM_E_UNSUPPORTED, "rpm_ipm_debug_lbfgs_step", "the solver was created with the exact Hessian");
  const IpmPlan& p = h->plan;
  IpmDev& D = h->D;
  hipStream_t st = ipm_stream(h);
  const size_t B = size_t(D.B), row = size_t(p.n) * sizeof(double), pitch = size_t(p.nv) * sizeof(double);
  h->hold.overwritten();
  IPM_TRY(h, hipMemcpyAsync(D.xt, x, B * row, hipMemcpyHostToDevice, st));
  if (reset) {
    ipm_launch_init(D, D.xt, st);
    lb_launch_reset(D, st);
  }
  IPM_TRY(h, hipMemcpy2DAsync(D.v, pitch, x, row, row, B, hipMemcpyHostToDevice, st));
  IPM_TRY(h, hipMemcpy2DAsync(D.glag, pitch, glag_new, row, row, B, hipMemcpyHostToDevice, st));
  IPM_TRY(h, hipMemcpy2DAsync(D.lb_gold, pitch, glag_old, row, row, B, hipMemcpyHostToDevice, st));
  std::vector<IpmInst> inst;
  int rc = ipm_edit_records(h, inst, [&](size_t bi, IpmInst& s) {
    s.mode = mode ? mode[bi] : 0;
    s.status = status ? status[bi] : 0;
  });
  if (rc) return rc;
  lb_launch_update(D, st);
  if ((rc = launch_check(h, "limited-memory update"))) return rc;
  IPM_TRY(h, hipStreamSynchronize(st));
  return RPM_OK;
}

/* what the update left: per instance the first 8 doubles of its record (sigma, pairs held, consecutive skips, previous iterate
 * valid, updates, skips, the two decision words), M (B x 12 x 12) and the pair columns S, Y (B x 6 x n, oldest first); NULL = skip */
int rpm_ipm_debug_lbfgs_state(rpm_ipm* h, double* record, double* M, double* S, double* Y) {
  if (!h) return RPM_E_INVALID;
  if (!h->lbfgs) return ipm_refuse(h, RPM_E_UNSUPPORTED, "rpm_ipm_debug_lbfgs_state", "the solver was created with the exact Hessian");
  IpmDev& D = h->D;
  const size_t B = size_t(D.B), th2 = size_t(2 * IPM_LB_H) * size_t(2 * IPM_LB_H), cols = B * IPM_LB_H * size_t(D.n);
  IPM_TRY(h, hipStreamSynchronize(ipm_stream(h)));
  std::vector<double> small(B * IPM_LB_SMALL);
  IPM_TRY(h, hipMemcpy(small.data(), D.lb_small, small.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t bi = 0; bi < B; ++bi) {
    if (record) std::memcpy(record + bi * 8, small.data() + bi * IPM_LB_SMALL, 8 * sizeof(double));
    if (M) std::memcpy(M + bi * th2, small.data() + bi * IPM_LB_SMALL + 8, th2 * sizeof(double));
  }
  if (S) IPM_TRY(h, hipMemcpy(S, D.lb_S, cols * sizeof(double), hipMemcpyDeviceToHost));
  if (Y) IPM_TRY(h, hipMemcpy(Y, D.lb_Y, cols * sizeof(double), hipMemcpyDeviceToHost));
  return RPM_OK;
}

/* K d = rhs with K = K0 - E M^-1 E' and the memory as it stands, the way an iteration does it: K0 (the matrix of the diagonal
 * Hessian; lower triangle in coordinate form, unknown order, every entry once, one structure for all instances, values B x nnz)
 * is factored, Z = K0^-1 E and C = M - E'Z follow, rhs (B x Nt, unknown order) is substituted and corrected (check_status 1).
 * Every instance is made live first.  An entry the layout has no slot for: RPM_E_INVALID. */
int rpm_ipm_debug_lbfgs_solve(rpm_ipm* h, int nnz, const int* rows, const int* cols, const double* vals, const double* rhs, double* sol) {
  if (!h || nnz < 0 || (nnz && (!rows || !cols || !vals)) || !rhs || !sol) return RPM_E_INVALID;
  if (!h->lbfgs) return ipm_refuse(h, RPM_E_UNSUPPORTED, "rpm_ipm_debug_lbfgs_solve", "the solver was created with the exact Hessian");
  const IpmPlan& p = h->plan;
  const size_t B = size_t(h->D.B);
  std::vector<double> store(B * size_t(p.storage()), 0.0);
  for (int k = 0; k < nnz; ++k) {
    const int a = rows[k], c = cols[k];
    const long long o = (a >= c && c >= 0 && a < p.Nt) ? ipm_plan_offset(p, a, c) : -1;
    if (o < 0) return no_slot(h, "rpm_ipm_debug_lbfgs_solve", a, c);
    for (size_t bi = 0; bi < B; ++bi) store[bi * size_t(p.storage()) + size_t(o)] = vals[bi * size_t(nnz) + size_t(k)];
  }
  std::vector<IpmInst> inst;
  return debug_factor_solve_unknown_order(h, store, rhs, sol, true, inst);
}

/* test hook: exactly the launches that precede the iteration loop (warm = 0: the cold start, lambda / z_L / z_U ignored), then the
 * state: v (B x nv: x, slacks), zL, zU (B x nv), lambda (B x m), mu (B), status (B: 0, or 5 after a non-finite input); outputs may be
 * NULL.  No step is taken. */
int rpm_ipm_debug_start(rpm_ipm* h, int warm, const double* x, const double* lambda, const double* z_L, const double* z_U,
                        double* v_out, double* zL_out, double* zU_out, double* lam_out, double* mu_out, int* status_out) {
  if (!h) return RPM_E_INVALID;
  int rc = ipm_check_start_args(h, "rpm_ipm_debug_start", "x (and, warm, lambda) are required", warm != 0, x, lambda, z_L, z_U);
  if (rc) return rc;
  Engine& e = h->eng->e;
  IpmDev& D = h->D;
  hipStream_t st = static_cast<hipStream_t>(dev_stream(e));
  const size_t B = size_t(D.B), Bn = B * h->plan.n, Bm = B * h->plan.m, Bv = B * h->plan.nv;
  double *d_x, *d_l, *d_zL, *d_zU;
  if ((rc = host_form(h, &d_x, &d_l, &d_zL, &d_zU))) return rc;
  IPM_TRY(h, hipMemcpyAsync(d_x, x, Bn * sizeof(double), hipMemcpyHostToDevice, st));
  if (warm) IPM_TRY(h, hipMemcpyAsync(d_l, lambda, Bm * sizeof(double), hipMemcpyHostToDevice, st));
  if (warm && z_L) {
    IPM_TRY(h, hipMemcpyAsync(d_zL, z_L, Bn * sizeof(double), hipMemcpyHostToDevice, st));
    IPM_TRY(h, hipMemcpyAsync(d_zU, z_U, Bn * sizeof(double), hipMemcpyHostToDevice, st));
  }
  IPM_TRY(h, hipStreamSynchronize(st));
  h->hold.start_begins();   // D.v, D.zL, D.zU and D.lam are about to hold a start state, not a solve's result
  if ((rc = ipm_start(h, warm != 0, d_x, d_l, warm && z_L ? d_zL : nullptr, warm && z_L ? d_zU : nullptr, st))) return rc;
  IPM_TRY(h, hipStreamSynchronize(st));
  if (v_out) IPM_TRY(h, hipMemcpy(v_out, D.v, Bv * sizeof(double), hipMemcpyDeviceToHost));
  if (zL_out) IPM_TRY(h, hipMemcpy(zL_out, D.zL, Bv * sizeof(double), hipMemcpyDeviceToHost));
  if (zU_out) IPM_TRY(h, hipMemcpy(zU_out, D.zU, Bv * sizeof(double), hipMemcpyDeviceToHost));
  if (lam_out) IPM_TRY(h, hipMemcpy(lam_out, D.lam, Bm * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<IpmInst> inst;
  if ((rc = ipm_download_records(h, inst))) return rc;
  for (size_t bi = 0; bi < B; ++bi) {
    if (mu_out) mu_out[bi] = inst[bi].mu;
    if (status_out) status_out[bi] = inst[bi].status;
  }
  h->hold.start_ends();
  return RPM_OK;
}

/* test hook: the loop's own next steps (IpmLoop, rpm_ipm_solver.hpp) on the state rpm_ipm_debug_start has just made, and what they
 * wrote.  stage 1: evaluate_and_residual.  stage 2: then exact_hessian (exact mode) and ipm_launch_assemble with level 1 left to the
 * fill kernel (df_on off for this call), no factorisation.  stage 3: evaluate_and_residual, exact_hessian,
 * factor_with_inertia_correction, substitute, direction — no trial point.  A pass after which no instance runs stops there, as the
 * loop does. */
int rpm_ipm_debug_pass(rpm_ipm* h, int stage, double* obj, double* grad, double* g, double* jac, double* c, double* glag, double* hess,
                       double* k_storage, double* rhs, double* dv, double* dlam, double* dzL, double* dzU, double* record) {
  if (!h) return RPM_E_INVALID;
  const char* who = "rpm_ipm_debug_pass";
  if (stage < 1 || stage > 3) return ipm_refuse(h, RPM_E_INVALID, who, "stage 1, 2 or 3");
  if (!h->hold.pass_allowed()) return ipm_refuse(h, RPM_E_INVALID, who, "valid only directly after rpm_ipm_debug_start on this solver");
  h->hold.pass_begins();
  h->stats = IpmStats{};
  const IpmLoop L = ipm_loop(h);
  const Engine& e = L.e;
  IpmDev& D = L.D;
  const IpmPlan& p = h->plan;
  int rc = L.evaluate_and_residual();
  if (!rc && stage >= 2 && h->h_cnt[0] > 0) {
    if (!h->lbfgs) rc = L.exact_hessian();
    if (!rc && stage == 2) {
      const IpmFusedFillOff by_the_fill_kernel(D);
      ipm_launch_assemble(D, std::max(e.nnz_jac, e.nnz_h), L.st);
      rc = launch_check(h, "ipm_launch_assemble");
    }
    if (!rc && stage == 3) rc = L.factor_with_inertia_correction();
    if (!rc && stage == 3) rc = L.substitute();
    if (!rc && stage == 3) rc = L.direction();
  }
  h->stats.solve_pending = false;
  if (rc) return rc;
  IPM_TRY(h, hipStreamSynchronize(L.st));
  h->hold.pass_ends(stage == 3 && h->h_cnt[0] > 0);   // a direction stands: rpm_ipm_debug_line_search may follow
  const size_t n = size_t(p.n), m = size_t(p.m), nv = size_t(p.nv);
  IPM_TRY(h, ipm_rows(D, obj, D.obj, 1, 1));
  IPM_TRY(h, ipm_rows(D, grad, D.grad, n, n));
  IPM_TRY(h, ipm_rows(D, g, D.g, m, size_t(D.sg)));
  IPM_TRY(h, ipm_rows(D, jac, D.jac, size_t(e.nnz_jac), size_t(D.sv)));
  IPM_TRY(h, ipm_rows(D, c, D.c, m, m));
  IPM_TRY(h, ipm_rows(D, glag, D.glag, nv, nv));
  // what the stage did not write is left alone in the caller's arrays, not filled from stale device memory
  if (stage >= 2 && !h->lbfgs) IPM_TRY(h, ipm_rows(D, hess, D.hess, size_t(e.nnz_h), size_t(e.nnz_h)));   // (limited-memory: there is none)
  if (stage >= 2) IPM_TRY(h, ipm_rows(D, k_storage, D.K, size_t(p.storage()), size_t(p.storage())));
  if (stage >= 3) {
    IPM_TRY(h, ipm_rows(D, dv, D.dv, nv, nv));
    IPM_TRY(h, ipm_rows(D, dlam, D.dlam, m, m));
    IPM_TRY(h, ipm_rows(D, dzL, D.dzL, nv, nv));
    IPM_TRY(h, ipm_rows(D, dzU, D.dzU, nv, nv));
  }
  if (rhs && stage >= 2 && (rc = ipm_download_unknown_order(h, D.rhs, 1, rhs))) return rc;
  std::vector<IpmInst> inst;
  return record ? download_flat_records(h, inst, record) : RPM_OK;
}

/* test hook: rounds of the line search (IpmLoop::line_search_round, what IpmLoop::line_search repeats) on the direction that
 * rpm_ipm_debug_pass(stage 3) has just left, or further rounds after itself; it stops early where the loop does.  filter (B x
 * n_filter pairs theta, phi) with filter_count (B) replaces every instance's filter before the first round. */
int rpm_ipm_debug_line_search(rpm_ipm* h, int rounds, int n_filter, const double* filter, const int* filter_count, double* xt, double* objt,
                              double* gt, double* ct, double* csoc, double* dv2, double* dlam2, double* dzL2, double* dzU2, double* soc_rhs,
                              double* rhs, double* record, int* counts) {
  if (!h) return RPM_E_INVALID;
  const char* who = "rpm_ipm_debug_line_search";
  if (rounds < 1) return ipm_refuse(h, RPM_E_INVALID, who, "rounds >= 1");
  if (n_filter < 0 || n_filter > IPM_FMAX) return ipm_refuse(h, RPM_E_INVALID, who, "at most " + std::to_string(IPM_FMAX) + " filter entries");
  if (n_filter > 0 && (!filter || !filter_count)) return ipm_refuse(h, RPM_E_INVALID, who, "filter entries need filter and filter_count");
  if (!h->hold.line_search_allowed())
    return ipm_refuse(h, RPM_E_INVALID, who, "valid only directly after rpm_ipm_debug_pass(stage 3) that left an instance running, or after itself");
  const IpmLoop L = ipm_loop(h);
  IpmDev& D = L.D;
  const IpmPlan& p = h->plan;
  const size_t B = size_t(D.B), d8 = sizeof(double);
  int rc;
  if (filter_count) {
    for (size_t bi = 0; bi < B; ++bi)
      if (filter_count[bi] < 0 || filter_count[bi] > n_filter) return ipm_refuse(h, RPM_E_INVALID, who, "filter_count outside 0 .. n_filter");
    std::vector<IpmInst> inst;
    if ((rc = ipm_edit_records(h, inst, [&](size_t bi, IpmInst& s) { s.nfilt = filter_count[bi]; }))) return rc;
    if (n_filter > 0)
      IPM_TRY(h, hipMemcpy2D(D.filt, 2 * IPM_FMAX * d8, filter, 2 * size_t(n_filter) * d8, 2 * size_t(n_filter) * d8, B, hipMemcpyHostToDevice));
    IPM_TRY(h, hipStreamSynchronize(L.st));   // (the records are up before `inst` goes)
  }
  const bool first = h->hold.line_search_begins();   // trial points and, next, the update: no longer the state of a start or a pass
  std::vector<double> rk(soc_rhs ? B * size_t(p.Nt_alloc) : 0);
  bool corrected = false;
  for (int r = 0; r < rounds; ++r) {
    if (!(first && r == 0) && L.line_search_over()) break;      // (before the first round ever the counts are not on the host yet)
    corrected = h->h_cnt[3] > 0;
    if ((rc = L.line_search_round(soc_rhs ? rk.data() : nullptr))) return rc;
  }
  if (soc_rhs && corrected) ipm_from_kkt_order(p, B, 1, rk.data(), soc_rhs);
  h->hold.line_search_ends();
  const size_t n = size_t(p.n), m = size_t(p.m), nv = size_t(p.nv);
  IPM_TRY(h, ipm_rows(D, xt, D.xt, n, n));
  IPM_TRY(h, ipm_rows(D, objt, D.objt, 1, 1));
  IPM_TRY(h, ipm_rows(D, gt, D.gt, m, size_t(D.sg)));
  IPM_TRY(h, ipm_rows(D, ct, D.ct, m, m));
  IPM_TRY(h, ipm_rows(D, csoc, D.csoc, m, m));
  IPM_TRY(h, ipm_rows(D, dv2, D.dv2, nv, nv));
  IPM_TRY(h, ipm_rows(D, dlam2, D.dlam2, m, m));
  IPM_TRY(h, ipm_rows(D, dzL2, D.dzL2, nv, nv));
  IPM_TRY(h, ipm_rows(D, dzU2, D.dzU2, nv, nv));
  if (rhs && (rc = ipm_download_unknown_order(h, D.rhs, 1, rhs))) return rc;
  if (counts) { counts[0] = h->h_cnt[2]; counts[1] = h->h_cnt[3]; }
  std::vector<IpmInst> inst;
  return record ? download_flat_records(h, inst, record) : RPM_OK;
}

/* test hook: IpmLoop::update on what rpm_ipm_debug_line_search has just left, and what it wrote.  filter: B x n_filter pairs, the
 * first min(nfilt, n_filter) of every instance. */
int rpm_ipm_debug_update(rpm_ipm* h, double* v, double* zL, double* zU, double* lambda, int n_filter, double* filter, double* vR, double* dr2,
                         double* pp, double* nn, double* zp, double* zn, double* lb_gold, double* record) {
  if (!h) return RPM_E_INVALID;
  const char* who = "rpm_ipm_debug_update";
  if (n_filter < 0 || n_filter > IPM_FMAX || (n_filter > 0 && !filter))
    return ipm_refuse(h, RPM_E_INVALID, who, "0 .. " + std::to_string(IPM_FMAX) + " filter entries into filter");
  if (!h->hold.update_allowed()) return ipm_refuse(h, RPM_E_INVALID, who, "valid only directly after rpm_ipm_debug_line_search on this solver");
  h->hold.updated();
  const IpmLoop L = ipm_loop(h);
  IpmDev& D = L.D;
  const IpmPlan& p = h->plan;
  if (int rc = L.update()) return rc;
  IPM_TRY(h, hipStreamSynchronize(L.st));
  const size_t n = size_t(p.n), m = size_t(p.m), nv = size_t(p.nv);
  IPM_TRY(h, ipm_rows(D, v, D.v, nv, nv));
  IPM_TRY(h, ipm_rows(D, zL, D.zL, nv, nv));
  IPM_TRY(h, ipm_rows(D, zU, D.zU, nv, nv));
  IPM_TRY(h, ipm_rows(D, lambda, D.lam, m, m));
  IPM_TRY(h, ipm_rows(D, filter, D.filt, 2 * size_t(n_filter), 2 * size_t(IPM_FMAX)));
  IPM_TRY(h, ipm_rows(D, vR, D.vR, nv, nv));
  IPM_TRY(h, ipm_rows(D, dr2, D.dr2, nv, nv));
  IPM_TRY(h, ipm_rows(D, pp, D.pp, m, m));
  IPM_TRY(h, ipm_rows(D, nn, D.nn, m, m));
  IPM_TRY(h, ipm_rows(D, zp, D.zp, m, m));
  IPM_TRY(h, ipm_rows(D, zn, D.zn, m, m));
  if (h->lbfgs) IPM_TRY(h, ipm_rows(D, lb_gold, D.lb_gold, n, nv));
  return download_flat_records(h, h->h_inst, record);   // (always: rpm_ipm_get_trace reads the iteration counts from h_inst)
}

}  // extern "C"
