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
  hipStream_t st = static_cast<hipStream_t>(dev_stream(h->eng->e));
  const size_t B = size_t(D.B);
  h->debug_started = false;
  h->state_held = false;
  h->debug_ls = 0;
  inst.assign(B, IpmInst{});
  for (IpmInst& s : inst) s.refactor = 1;
  IPM_TRY(h, hipMemcpyAsync(D.inst, inst.data(), B * sizeof(IpmInst), hipMemcpyHostToDevice, st));
  IPM_TRY(h, hipMemcpyAsync(D.K, store, B * size_t(h->plan.storage()) * sizeof(double), hipMemcpyHostToDevice, st));
  IPM_TRY(h, hipMemcpyAsync(D.rhs, rhs, B * rhs_len * sizeof(double), hipMemcpyHostToDevice, st));
  const int df_keep = D.df_on;
  D.df_on = 0;
  int rc;
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
  D.df_on = df_keep;
  if (rc) return rc;
  IPM_TRY(h, hipStreamSynchronize(st));
  IPM_TRY(h, hipMemcpy(rhs, D.rhs, B * rhs_len * sizeof(double), hipMemcpyDeviceToHost));
  IPM_TRY(h, hipMemcpy(inst.data(), D.inst, B * sizeof(IpmInst), hipMemcpyDeviceToHost));
  return RPM_OK;
}

// right-hand sides in unknown order (B x Nt) <-> vectors in KKT order (B x Nt_alloc)
std::vector<double> to_kkt_order(const IpmPlan& p, size_t B, const double* rhs) {
  std::vector<double> r(B * size_t(p.Nt_alloc), 0.0);
  for (size_t bi = 0; bi < B; ++bi)
    for (size_t a = 0; a < size_t(p.Nt); ++a) r[bi * p.Nt_alloc + p.pos[a]] = rhs[bi * p.Nt + a];
  return r;
}
void from_kkt_order(const IpmPlan& p, size_t B, const std::vector<double>& r, double* sol) {
  for (size_t bi = 0; bi < B; ++bi)
    for (size_t a = 0; a < size_t(p.Nt); ++a) sol[bi * p.Nt + a] = r[bi * p.Nt_alloc + p.pos[a]];
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
int no_slot(rpm_ipm* h, const char* who, long long a, long long c) {
  h->err = std::string(who) + ": entry (" + std::to_string(a) + ", " + std::to_string(c) + ") has no slot in the layout";
  return RPM_E_INVALID;
}
}  // namespace

extern "C" {

/* test hook: factor + solve the caller's matrices (B x storage doubles in the band + border layout, lower triangle)
 * against B right-hand sides in KKT order; returns the solutions and the signs of D */
int rpm_ipm_debug_solve(rpm_ipm* h, const double* k_storage, const double* rhs, double* sol, int* n_pos, int* n_neg) {
  if (!h || !k_storage || !rhs || !sol) return RPM_E_INVALID;
  const IpmPlan& p = h->plan;
  if (p.nd) { h->err = "rpm_ipm_debug_solve takes the band + border storage; with nested dissection use rpm_ipm_debug_solve_dense"; return RPM_E_UNSUPPORTED; }
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
  std::vector<double> r = to_kkt_order(p, B, rhs);
  std::vector<IpmInst> inst;
  int rc = debug_factor_solve(h, store.data(), r.data(), size_t(p.Nt_alloc), false, inst);
  if (rc) return rc;
#ifdef IPM_TIMING
  // kkt_factor_dense_kernel (build with -DIPM_TIMING_SUB=<out of range>): tile wave 0 and the diagonal wave of interval block 0
  fprintf(stderr, "level-1 phases of instance 0 [100 MHz ticks]: panel %lld  wait B3 %lld  next diagonal tile + B1 %lld  update %lld  wait B2 %lld  early block columns %lld | diagonal wave: waiting %lld  factoring %lld\n",
          inst[0].dbg[0], inst[0].dbg[1], inst[0].dbg[2], inst[0].dbg[3], inst[0].dbg[4], inst[0].dbg[5], inst[0].dbg[6], inst[0].dbg[7]);
  // kkt_factor_kernel (-DIPM_TIMING_SUB=<sub-problem>): the same record read as the left-looking kernel's phases
  fprintf(stderr, "left-looking phases of instance 0 [100 MHz ticks]: T %lld  k-loop %lld  diag %lld  panel %lld  corner %lld  tail %lld\n",
          inst[0].dbg[0], inst[0].dbg[1], inst[0].dbg[2], inst[0].dbg[3], inst[0].dbg[4], inst[0].dbg[5]);
#endif
  from_kkt_order(p, B, r, sol);
  pivot_signs(inst, n_pos, n_neg);
  return RPM_OK;
}

/* storage offset of the entry between unknowns ua and uc (unknown order as above), -1 if the layout has no slot for it */
int rpm_ipm_debug_slot(rpm_ipm* h, int ua, int uc, long long* offset) {
  if (!h || !offset || ua < 0 || uc < 0 || ua >= h->plan.Nt || uc >= h->plan.Nt) return RPM_E_INVALID;
  *offset = ipm_plan_offset(h->plan, ua, uc);
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
  if (!h->lbfgs) { h->err = "rpm_ipm_debug_lbfgs_step: the solver was created with the exact Hessian"; return RPM_E_UNSUPPORTED; }
  const IpmPlan& p = h->plan;
  IpmDev& D = h->D;
  hipStream_t st = static_cast<hipStream_t>(dev_stream(h->eng->e));
  const size_t B = size_t(D.B), row = size_t(p.n) * sizeof(double), pitch = size_t(p.nv) * sizeof(double);
  h->debug_started = false;
  h->state_held = false;
  h->debug_ls = 0;
  IPM_TRY(h, hipMemcpyAsync(D.xt, x, B * row, hipMemcpyHostToDevice, st));
  if (reset) {
    ipm_launch_init(D, D.xt, st);
    lb_launch_reset(D, st);
  }
  IPM_TRY(h, hipMemcpy2DAsync(D.v, pitch, x, row, row, B, hipMemcpyHostToDevice, st));
  IPM_TRY(h, hipMemcpy2DAsync(D.glag, pitch, glag_new, row, row, B, hipMemcpyHostToDevice, st));
  IPM_TRY(h, hipMemcpy2DAsync(D.lb_gold, pitch, glag_old, row, row, B, hipMemcpyHostToDevice, st));
  std::vector<IpmInst> inst(B);
  IPM_TRY(h, hipMemcpyAsync(inst.data(), D.inst, B * sizeof(IpmInst), hipMemcpyDeviceToHost, st));
  IPM_TRY(h, hipStreamSynchronize(st));
  for (size_t bi = 0; bi < B; ++bi) {
    inst[bi].mode = mode ? mode[bi] : 0;
    inst[bi].status = status ? status[bi] : 0;
  }
  IPM_TRY(h, hipMemcpyAsync(D.inst, inst.data(), B * sizeof(IpmInst), hipMemcpyHostToDevice, st));
  lb_launch_update(D, st);
  int rc = launch_check(h, "limited-memory update");
  if (rc) return rc;
  IPM_TRY(h, hipStreamSynchronize(st));
  return RPM_OK;
}

/* what the update left: per instance the first 8 doubles of its record (sigma, pairs held, consecutive skips, previous iterate
 * valid, updates, skips, the two decision words), M (B x 12 x 12) and the pair columns S, Y (B x 6 x n, oldest first); NULL = skip */
int rpm_ipm_debug_lbfgs_state(rpm_ipm* h, double* record, double* M, double* S, double* Y) {
  if (!h) return RPM_E_INVALID;
  if (!h->lbfgs) { h->err = "rpm_ipm_debug_lbfgs_state: the solver was created with the exact Hessian"; return RPM_E_UNSUPPORTED; }
  IpmDev& D = h->D;
  hipStream_t st = static_cast<hipStream_t>(dev_stream(h->eng->e));
  const size_t B = size_t(D.B), th2 = size_t(2 * IPM_LB_H) * size_t(2 * IPM_LB_H), cols = B * IPM_LB_H * size_t(D.n);
  IPM_TRY(h, hipStreamSynchronize(st));
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
  if (!h->lbfgs) { h->err = "rpm_ipm_debug_lbfgs_solve: the solver was created with the exact Hessian"; return RPM_E_UNSUPPORTED; }
  const IpmPlan& p = h->plan;
  const size_t B = size_t(h->D.B);
  std::vector<double> store(B * size_t(p.storage()), 0.0);
  for (int k = 0; k < nnz; ++k) {
    const int a = rows[k], c = cols[k];
    const long long o = (a >= c && c >= 0 && a < p.Nt) ? ipm_plan_offset(p, a, c) : -1;
    if (o < 0) return no_slot(h, "rpm_ipm_debug_lbfgs_solve", a, c);
    for (size_t bi = 0; bi < B; ++bi) store[bi * size_t(p.storage()) + size_t(o)] = vals[bi * size_t(nnz) + size_t(k)];
  }
  std::vector<double> r = to_kkt_order(p, B, rhs);
  std::vector<IpmInst> inst;
  int rc = debug_factor_solve(h, store.data(), r.data(), size_t(p.Nt_alloc), true, inst);
  if (rc) return rc;
  from_kkt_order(p, B, r, sol);
  return RPM_OK;
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
  h->solved = false;   // D.v, D.zL, D.zU and D.lam are about to hold a start state, not a solve's result
  h->state_held = false;
  if ((rc = ipm_start(h, warm != 0, d_x, d_l, warm && z_L ? d_zL : nullptr, warm && z_L ? d_zU : nullptr, st))) return rc;
  IPM_TRY(h, hipStreamSynchronize(st));
  if (v_out) IPM_TRY(h, hipMemcpy(v_out, D.v, Bv * sizeof(double), hipMemcpyDeviceToHost));
  if (zL_out) IPM_TRY(h, hipMemcpy(zL_out, D.zL, Bv * sizeof(double), hipMemcpyDeviceToHost));
  if (zU_out) IPM_TRY(h, hipMemcpy(zU_out, D.zU, Bv * sizeof(double), hipMemcpyDeviceToHost));
  if (lam_out) IPM_TRY(h, hipMemcpy(lam_out, D.lam, Bm * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<IpmInst> inst(B);
  IPM_TRY(h, hipMemcpy(inst.data(), D.inst, B * sizeof(IpmInst), hipMemcpyDeviceToHost));
  for (size_t bi = 0; bi < B; ++bi) {
    if (mu_out) mu_out[bi] = inst[bi].mu;
    if (status_out) status_out[bi] = inst[bi].status;
  }
  h->debug_started = true;
  h->state_held = true;
  h->debug_ls = 0;
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
  if (stage < 1 || stage > 3) { h->err = "rpm_ipm_debug_pass: stage 1, 2 or 3"; return RPM_E_INVALID; }
  if (!h->debug_started) { h->err = "rpm_ipm_debug_pass: valid only directly after rpm_ipm_debug_start on this solver"; return RPM_E_INVALID; }
  h->debug_started = false;
  h->debug_ls = 0;
  Engine& e = h->eng->e;
  IpmDev& D = h->D;
  const IpmPlan& p = h->plan;
  hipStream_t st = static_cast<hipStream_t>(dev_stream(e));
  h->lb_iterations = 0;
  h->total_factorizations = h->total_iterations = h->total_trials = h->total_soc = 0;
  h->factor_ms = h->solve_ms = 0.0;
  h->solve_pending = false;
  const IpmLoop L{h, e, D, st, D.scal_on != 0};
  int rc = L.evaluate_and_residual();
  if (!rc && stage >= 2 && h->h_cnt[0] > 0) {
    if (!h->lbfgs) rc = L.exact_hessian();
    if (!rc && stage == 2) {
      const int df_keep = D.df_on;
      D.df_on = 0;
      ipm_launch_assemble(D, std::max(e.nnz_jac, e.nnz_h), st);
      D.df_on = df_keep;
      rc = launch_check(h, "ipm_launch_assemble");
    }
    if (!rc && stage == 3) rc = L.factor_with_inertia_correction();
    if (!rc && stage == 3) rc = L.substitute();
    if (!rc && stage == 3) rc = L.direction();
  }
  h->solve_pending = false;
  if (rc) return rc;
  IPM_TRY(h, hipStreamSynchronize(st));
  h->debug_ls = stage == 3 && h->h_cnt[0] > 0 ? 1 : 0;   // a direction stands: rpm_ipm_debug_line_search may follow
  const size_t B = size_t(D.B), d8 = sizeof(double);
  auto rows = [&](double* dst, const double* src, size_t width, size_t pitch) -> hipError_t {   // B rows of `width` doubles, `pitch` apart
    if (!dst || !width) return hipSuccess;
    return hipMemcpy2D(dst, width * d8, src, pitch * d8, width * d8, B, hipMemcpyDeviceToHost);
  };
  IPM_TRY(h, rows(obj, D.obj, 1, 1));
  IPM_TRY(h, rows(grad, D.grad, size_t(p.n), size_t(p.n)));
  IPM_TRY(h, rows(g, D.g, size_t(p.m), size_t(D.sg)));
  IPM_TRY(h, rows(jac, D.jac, size_t(e.nnz_jac), size_t(D.sv)));
  IPM_TRY(h, rows(c, D.c, size_t(p.m), size_t(p.m)));
  IPM_TRY(h, rows(glag, D.glag, size_t(p.nv), size_t(p.nv)));
  // what the stage did not write is left alone in the caller's arrays, not filled from stale device memory
  if (stage >= 2 && !h->lbfgs) IPM_TRY(h, rows(hess, D.hess, size_t(e.nnz_h), size_t(e.nnz_h)));   // (limited-memory: there is none)
  if (stage >= 2) IPM_TRY(h, rows(k_storage, D.K, size_t(p.storage()), size_t(p.storage())));
  if (stage >= 3) {
    IPM_TRY(h, rows(dv, D.dv, size_t(p.nv), size_t(p.nv)));
    IPM_TRY(h, rows(dlam, D.dlam, size_t(p.m), size_t(p.m)));
    IPM_TRY(h, rows(dzL, D.dzL, size_t(p.nv), size_t(p.nv)));
    IPM_TRY(h, rows(dzU, D.dzU, size_t(p.nv), size_t(p.nv)));
  }
  if (rhs && stage >= 2) {
    std::vector<double> r(B * size_t(p.Nt_alloc));
    IPM_TRY(h, hipMemcpy(r.data(), D.rhs, r.size() * d8, hipMemcpyDeviceToHost));
    from_kkt_order(p, B, r, rhs);
  }
  if (record) {
    std::vector<IpmInst> inst(B);
    IPM_TRY(h, hipMemcpy(inst.data(), D.inst, B * sizeof(IpmInst), hipMemcpyDeviceToHost));
    for (size_t bi = 0; bi < B; ++bi) flat_record(inst[bi], record + bi * RPM_IPM_RECORD_DOUBLES);
  }
  return RPM_OK;
}

/* test hook: rounds of the line search (IpmLoop::line_search_round, what IpmLoop::line_search repeats) on the direction that
 * rpm_ipm_debug_pass(stage 3) has just left, or further rounds after itself; it stops early where the loop does.  filter (B x
 * n_filter pairs theta, phi) with filter_count (B) replaces every instance's filter before the first round. */
int rpm_ipm_debug_line_search(rpm_ipm* h, int rounds, int n_filter, const double* filter, const int* filter_count, double* xt, double* objt,
                              double* gt, double* ct, double* csoc, double* dv2, double* dlam2, double* dzL2, double* dzU2, double* soc_rhs,
                              double* rhs, double* record, int* counts) {
  if (!h) return RPM_E_INVALID;
  const char* who = "rpm_ipm_debug_line_search";
  if (rounds < 1) { h->err = std::string(who) + ": rounds >= 1"; return RPM_E_INVALID; }
  if (n_filter < 0 || n_filter > IPM_FMAX) { h->err = std::string(who) + ": at most " + std::to_string(IPM_FMAX) + " filter entries"; return RPM_E_INVALID; }
  if (n_filter > 0 && (!filter || !filter_count)) { h->err = std::string(who) + ": filter entries need filter and filter_count"; return RPM_E_INVALID; }
  if (h->debug_ls == 0) {
    h->err = std::string(who) + ": valid only directly after rpm_ipm_debug_pass(stage 3) that left an instance running, or after itself";
    return RPM_E_INVALID;
  }
  Engine& e = h->eng->e;
  IpmDev& D = h->D;
  const IpmPlan& p = h->plan;
  hipStream_t st = static_cast<hipStream_t>(dev_stream(e));
  const size_t B = size_t(D.B), d8 = sizeof(double);
  std::vector<IpmInst> inst(B);
  if (filter_count) {
    for (size_t bi = 0; bi < B; ++bi)
      if (filter_count[bi] < 0 || filter_count[bi] > n_filter) { h->err = std::string(who) + ": filter_count outside 0 .. n_filter"; return RPM_E_INVALID; }
    IPM_TRY(h, hipStreamSynchronize(st));
    IPM_TRY(h, hipMemcpy(inst.data(), D.inst, B * sizeof(IpmInst), hipMemcpyDeviceToHost));
    for (size_t bi = 0; bi < B; ++bi) inst[bi].nfilt = filter_count[bi];
    IPM_TRY(h, hipMemcpy(D.inst, inst.data(), B * sizeof(IpmInst), hipMemcpyHostToDevice));
    if (n_filter > 0)
      IPM_TRY(h, hipMemcpy2D(D.filt, 2 * IPM_FMAX * d8, filter, 2 * size_t(n_filter) * d8, 2 * size_t(n_filter) * d8, B, hipMemcpyHostToDevice));
  }
  const bool first = h->debug_ls == 1;
  h->debug_ls = 0;
  h->state_held = false;   // trial points and, next, the update: no longer the state of a start or a pass
  const IpmLoop L{h, e, D, st, D.scal_on != 0};
  std::vector<double> rk(soc_rhs ? B * size_t(p.Nt_alloc) : 0);
  bool corrected = false;
  for (int r = 0; r < rounds; ++r) {
    if (!(first && r == 0) && L.line_search_over()) break;      // (before the first round ever the counts are not on the host yet)
    corrected = h->h_cnt[3] > 0;
    if (int rc = L.line_search_round(soc_rhs ? rk.data() : nullptr)) return rc;
  }
  if (soc_rhs && corrected) from_kkt_order(p, B, rk, soc_rhs);
  h->debug_ls = 2;
  auto rows = [&](double* dst, const double* src, size_t width, size_t pitch) -> hipError_t {
    if (!dst || !width) return hipSuccess;
    return hipMemcpy2D(dst, width * d8, src, pitch * d8, width * d8, B, hipMemcpyDeviceToHost);
  };
  const size_t n = size_t(p.n), m = size_t(p.m), nv = size_t(p.nv);
  IPM_TRY(h, rows(xt, D.xt, n, n));
  IPM_TRY(h, rows(objt, D.objt, 1, 1));
  IPM_TRY(h, rows(gt, D.gt, m, size_t(D.sg)));
  IPM_TRY(h, rows(ct, D.ct, m, m));
  IPM_TRY(h, rows(csoc, D.csoc, m, m));
  IPM_TRY(h, rows(dv2, D.dv2, nv, nv));
  IPM_TRY(h, rows(dlam2, D.dlam2, m, m));
  IPM_TRY(h, rows(dzL2, D.dzL2, nv, nv));
  IPM_TRY(h, rows(dzU2, D.dzU2, nv, nv));
  if (rhs) {
    std::vector<double> r(B * size_t(p.Nt_alloc));
    IPM_TRY(h, hipMemcpy(r.data(), D.rhs, r.size() * d8, hipMemcpyDeviceToHost));
    from_kkt_order(p, B, r, rhs);
  }
  if (record) {
    IPM_TRY(h, hipMemcpy(inst.data(), D.inst, B * sizeof(IpmInst), hipMemcpyDeviceToHost));
    for (size_t bi = 0; bi < B; ++bi) flat_record(inst[bi], record + bi * RPM_IPM_RECORD_DOUBLES);
  }
  if (counts) { counts[0] = h->h_cnt[2]; counts[1] = h->h_cnt[3]; }
  return RPM_OK;
}

/* test hook: IpmLoop::update on what rpm_ipm_debug_line_search has just left, and what it wrote.  filter: B x n_filter pairs, the
 * first min(nfilt, n_filter) of every instance. */
int rpm_ipm_debug_update(rpm_ipm* h, double* v, double* zL, double* zU, double* lambda, int n_filter, double* filter, double* vR, double* dr2,
                         double* pp, double* nn, double* zp, double* zn, double* lb_gold, double* record) {
  if (!h) return RPM_E_INVALID;
  if (n_filter < 0 || n_filter > IPM_FMAX || (n_filter > 0 && !filter)) { h->err = "rpm_ipm_debug_update: 0 .. " + std::to_string(IPM_FMAX) + " filter entries into filter"; return RPM_E_INVALID; }
  if (h->debug_ls != 2) { h->err = "rpm_ipm_debug_update: valid only directly after rpm_ipm_debug_line_search on this solver"; return RPM_E_INVALID; }
  h->debug_ls = 0;
  Engine& e = h->eng->e;
  IpmDev& D = h->D;
  const IpmPlan& p = h->plan;
  hipStream_t st = static_cast<hipStream_t>(dev_stream(e));
  const IpmLoop L{h, e, D, st, D.scal_on != 0};
  if (int rc = L.update()) return rc;
  IPM_TRY(h, hipStreamSynchronize(st));
  const size_t B = size_t(D.B), d8 = sizeof(double);
  auto rows = [&](double* dst, const double* src, size_t width, size_t pitch) -> hipError_t {
    if (!dst || !width) return hipSuccess;
    return hipMemcpy2D(dst, width * d8, src, pitch * d8, width * d8, B, hipMemcpyDeviceToHost);
  };
  const size_t n = size_t(p.n), m = size_t(p.m), nv = size_t(p.nv);
  IPM_TRY(h, rows(v, D.v, nv, nv));
  IPM_TRY(h, rows(zL, D.zL, nv, nv));
  IPM_TRY(h, rows(zU, D.zU, nv, nv));
  IPM_TRY(h, rows(lambda, D.lam, m, m));
  IPM_TRY(h, rows(filter, D.filt, 2 * size_t(n_filter), 2 * size_t(IPM_FMAX)));
  IPM_TRY(h, rows(vR, D.vR, nv, nv));
  IPM_TRY(h, rows(dr2, D.dr2, nv, nv));
  IPM_TRY(h, rows(pp, D.pp, m, m));
  IPM_TRY(h, rows(nn, D.nn, m, m));
  IPM_TRY(h, rows(zp, D.zp, m, m));
  IPM_TRY(h, rows(zn, D.zn, m, m));
  if (h->lbfgs) IPM_TRY(h, rows(lb_gold, D.lb_gold, n, nv));
  h->h_inst.resize(B);                     // (rpm_ipm_get_trace reads the iteration counts from here)
  IPM_TRY(h, hipMemcpy(h->h_inst.data(), D.inst, B * sizeof(IpmInst), hipMemcpyDeviceToHost));
  if (record)
    for (size_t bi = 0; bi < B; ++bi) flat_record(h->h_inst[bi], record + bi * RPM_IPM_RECORD_DOUBLES);
  return RPM_OK;
}

}  // extern "C"
