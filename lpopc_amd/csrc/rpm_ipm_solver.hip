// rpm_ipm_solver.hip — row f-2, host side: the interior-point loop over the batched kernels of rpm_ipm_step_kernels.hip, rpm_kkt_factor.hip and rpm_kkt_solve.hip (per
// iteration three counters come back from the device, nothing else) and the rpm_ipm_* entry points of the C ABI (the test hooks: rpm_ipm_debug.hip).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>

#include "rpm_ipm_solver.hpp"

// =================================================================================================== host side + ABI
using namespace rpm;

namespace {
// a run of device allocations: the first failure is kept (code here, text in h->err), the calls after it do nothing
struct IpmAllocs {
  rpm_ipm* h;
  int rc = RPM_OK;
  template <class T>
  void room(T** dst, size_t count) { if (!rc) rc = ipm_alloc(h, dst, count); }
  template <class T>
  void table(const T** dst, const std::vector<T>& src) {
    T* p = nullptr;
    if (!rc) rc = ipm_alloc(h, &p, src.size(), src.data());
    *dst = p;
  }
};

bool env_is_zero(const char* name) {   // the "set and equal to 0" switches of rpm_ipm_create
  const char* v = std::getenv(name);
  return v && std::atoi(v) == 0;
}

// the plan's scatter maps and the fill list, resident
int upload_plan_tables(rpm_ipm* h, const IpmFillList& fill, bool one_pass) {
  const Engine& e = h->eng->e;
  const IpmPlan& p = h->plan;
  IpmDev& D = h->D;
  IpmAllocs a{h};
  a.table(&D.pos, p.pos); a.table(&D.row_slack, p.row_slack); a.table(&D.slack_row, p.slack_row);
  a.table(&D.jac_dst, p.jac_dst); a.table(&D.hes_dst, p.hes_dst);
  a.table(&D.diag_dst, p.diag_dst); a.table(&D.slk_dst, p.slk_dst); a.table(&D.jt_ptr, p.jt_ptr);
  a.table(&D.jt_ent, p.jt_ent); a.table(&D.jt_row, p.jt_row);
  a.table(&D.hg_ptr, p.hg_ptr); a.table(&D.hg_src, p.hg_src); a.table(&D.hg_dst, p.hg_dst);
  D.n_hg = int(p.hg_dst.size());
  if (one_pass) {   // the one-pass fill (ipm_fill_kernel); as_nchunk 0: the two-kernel path
    a.table(&D.as_dst, fill.dst); a.table(&D.as_ki, fill.ki); a.table(&D.as_hg, fill.hg); a.table(&D.as_ptr, fill.ptr);
    D.as_nchunk = fill.n_chunks();
  }
  const std::vector<int> long_cols = ipm_long_columns(p);
  D.n_long = int(long_cols.size());
  a.table(&D.long_cols, long_cols);
  a.table(&D.gl, e.gl); a.table(&D.gu, e.gu);
  return a.rc;
}

// the factorisation's sub-problems and what moves data between their levels, resident
int upload_factor_tables(rpm_ipm* h, const IpmSubList& s, const IpmFusedFill& fused) {
  const IpmPlan& p = h->plan;
  IpmDev& D = h->D;
  IpmAllocs a{h};
  // level 1 assembled by kkt_factor_dense_kernel itself (IpmDev::df_on); the fill then leaves out the chunks inside such a block
  D.df_tiles = fused.tiles;
  D.df_on = fused.built ? 1 : 0;
  if (fused.built) {
    a.table(&D.df_ptr, fused.ptr); a.table(&D.df_ki, fused.ki); a.table(&D.df_hg, fused.hg);
    a.table(&D.as_live, fused.live); a.table(&D.df_map, fused.map);
    D.as_nlive = int(fused.live.size());
  }
  // factorisation sub-problems: the whole band + border matrix, or the interval blocks followed by the separator system
  a.table(&D.subs, s.subs);
  D.n_sub = int(s.subs.size()); D.n_l1 = s.n_l1; D.n_l2 = s.n_l2; D.max_sub_nt = s.max_sub_nt;
  a.room(&D.piv, size_t(D.B) * s.subs.size() * 3);
  a.table(&D.cg_ptr, p.cg_ptr); a.table(&D.cg_src, p.cg_src); a.table(&D.cg_dst, p.cg_dst);
  a.table(&D.rg_ptr, p.rg_ptr); a.table(&D.rg_src, p.rg_src); a.table(&D.rg_dst, p.rg_dst);
  a.table(&D.rs_dst, p.rs_dst); a.table(&D.rs_src, p.rs_src); a.table(&D.gap_pos, p.gap_pos);
  D.n_cg = int(p.cg_dst.size()); D.n_rg = int(p.rg_dst.size()); D.n_rs = int(p.rs_dst.size()); D.n_gap = int(p.gap_pos.size());
  a.table(&D.cg2_ptr, p.cg2_ptr); a.table(&D.cg2_src, p.cg2_src); a.table(&D.cg2_dst, p.cg2_dst);
  a.table(&D.rg2_ptr, p.rg2_ptr); a.table(&D.rg2_src, p.rg2_src); a.table(&D.rg2_dst, p.rg2_dst);
  a.table(&D.rs2_dst, p.rs2_dst); a.table(&D.rs2_src, p.rs2_src);
  D.n_cg2 = int(p.cg2_dst.size()); D.n_rg2 = int(p.rg2_dst.size()); D.n_rs2 = int(p.rs2_dst.size());
  D.n_cg_long = p.n_cg_long; D.n_cg2_long = p.n_cg2_long;
  return a.rc;
}

// per-instance state and work space; the variable bounds of every instance default to the engine's
int alloc_state(rpm_ipm* h) {
  Engine& e = h->eng->e;
  const IpmPlan& p = h->plan;
  IpmDev& D = h->D;
  const size_t B = size_t(D.B), Bm = B * size_t(std::max(p.m, 1));   // (m >= 1 keeps the allocations non-empty)
  IpmAllocs a{h};
  a.room(&D.v, B * p.nv); a.room(&D.vl, B * p.nv); a.room(&D.vu, B * p.nv);
  a.room(&D.zL, B * p.nv); a.room(&D.zU, B * p.nv); a.room(&D.lam, B * p.m);
  a.room(&D.dv, B * p.nv); a.room(&D.dlam, B * p.m); a.room(&D.dzL, B * p.nv);
  a.room(&D.dzU, B * p.nv); a.room(&D.glag, B * p.nv); a.room(&D.c, B * p.m);
  a.room(&D.rhs, B * size_t(p.Nt_alloc)); a.room(&D.K, B * size_t(p.storage())); a.room(&D.filt, B * 2 * IPM_FMAX);
  a.room(&D.xe, B * p.n); a.room(&D.xt, B * p.n); a.room(&D.grad, B * p.n);
  a.room(&D.g, B * size_t(D.sg)); a.room(&D.jac, B * size_t(D.sv)); a.room(&D.hess, B * size_t(e.nnz_h));
  a.room(&D.obj, B); a.room(&D.gt, B * size_t(D.sg)); a.room(&D.objt, B);
  a.room(&D.inst, B); a.room(&D.cnt, size_t(4));
  a.room(&D.vR, B * p.nv); a.room(&D.dr2, B * p.nv);
  a.room(&D.vl0, B * p.nv); a.room(&D.vu0, B * p.nv);
  if (h->lbfgs) {
    a.room(&D.lb_S, B * IPM_LB_H * p.n); a.room(&D.lb_Y, B * IPM_LB_H * p.n);
    a.room(&D.lb_xprev, B * p.n); a.room(&D.lb_gold, B * p.nv);
    a.room(&D.lb_small, B * IPM_LB_SMALL); a.room(&D.lb_part, B * IPM_LB_PART);
    a.room(&D.lb_Z, size_t(2 * IPM_LB_H) * B * size_t(p.Nt_alloc));
  }
  a.room(&D.sc, Bm); a.room(&D.sf, B); a.room(&D.lam_h, Bm);   // nlp_scaling (off until the option asks for it; the arrays are small)
  a.table(&D.jac_row, e.jac_i);                                 // ... the row of every Jacobian entry
  D.nnz_var = e.nnz_nl + e.nnz_lin;
  // restoration phase and second-order correction work space
  a.room(&D.pp, Bm); a.room(&D.nn, Bm); a.room(&D.zp, Bm); a.room(&D.zn, Bm);
  a.room(&D.dpp, Bm); a.room(&D.dnn, Bm); a.room(&D.dzp, Bm); a.room(&D.dzn, Bm);
  a.room(&D.dlam2, Bm); a.room(&D.csoc, Bm); a.room(&D.ct, Bm);
  a.room(&D.dv2, B * p.nv); a.room(&D.dzL2, B * p.nv); a.room(&D.dzU2, B * p.nv);
  a.room(&D.rfilt, B * 2 * IPM_FMAX);
  a.room(&D.part, B * IPM_VEC_BLOCKS * IPM_VEC_PART); a.room(&D.tick, B);
  if (a.rc) return a.rc;
  // on the engine's (non-blocking) stream, where the kernels that take tickets run: a null-stream fill is not ordered against it
  if (hipMemsetAsync(D.tick, 0, B * sizeof(int), static_cast<hipStream_t>(dev_stream(e))) != hipSuccess) return ipm_refuse(h, RPM_E_DEVICE, "", "hipMemset");
  if (hipHostMalloc(reinterpret_cast<void**>(&h->h_cnt), 4 * sizeof(int)) != hipSuccess) return ipm_refuse(h, RPM_E_DEVICE, "", "hipHostMalloc");
  std::vector<double> l(B * p.nv, 0.0), u(B * p.nv, 0.0);
  for (size_t bi = 0; bi < B; ++bi)
    for (int i = 0; i < p.n; ++i) { l[bi * p.nv + i] = e.xl[i]; u[bi * p.nv + i] = e.xu[i]; }
  if (hipMemcpy(D.vl0, l.data(), l.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(D.vu0, u.data(), u.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return ipm_refuse(h, RPM_E_DEVICE, "", "hipMemcpy");
  h->h_inst.resize(B);
  return RPM_OK;
}

// why kkt_factor_kernel cannot hold the plan's sub-problems — rows per block column, LDS —; empty: it can
std::string factor_kernel_refusal(const IpmPlan& p) {
  if (p.max_rows > 4 * IPM_MT * 16)
    return "band + border of " + std::to_string(p.max_rows - IPM_W) + " rows exceeds the factorisation's 512 rows per block column";
  if (kkt_factor_lds_bytes(p) > 150 * 1024)
    return "band of " + std::to_string(p.b) + " and border of " + std::to_string(p.nb) + " rows do not fit the factorisation's LDS";
  return "";
}

// which factorisation kernel runs each level, with how much LDS and how many tiles per wave; refuses what no kernel holds
int choose_kernels(rpm_ipm* h, const IpmSubList& s) {
  const IpmPlan& p = h->plan;
  IpmDev& D = h->D;
  const size_t B = size_t(D.B);
  D.last_dense_corner = 1;
  if (s.n_l1 > 0) {
    auto dense_lds_of = [&](int first, int count) -> size_t {   // LDS of kkt_factor_dense_kernel for these sub-problems, 0: one does not fit
      int rows = 0;   // most 16-row blocks (band + border)
      for (int i = first; i < first + count; ++i) rows = std::max(rows, s.subs[size_t(i)].g.block_rows());
      return count > 0 && rows <= kkt_factor_dense_max_block_rows() ? kkt_factor_dense_lds_bytes(rows) : 0;
    };
    h->l1_dense_lds = dense_lds_of(0, s.n_l1);
    h->l2_dense_lds = dense_lds_of(s.n_l1, s.n_l2);
    for (int i = s.n_l1; i < s.n_l1 + s.n_l2; ++i)     // groups of a narrow band stay on kkt_factor_kernel, which skips what lies outside the band
      if (2 * s.subs[size_t(i)].g.b < s.subs[size_t(i)].g.Nb) h->l2_dense_lds = 0;
    h->last_dense_lds = dense_lds_of(s.n_l1 + s.n_l2, 1);
    // (one workgroup per CU: a sweep of many small last levels is better off on kkt_factor_kernel, several workgroups per CU —
    // 1024 quadrotor instances 0.12 against 0.30 ms)
    if (B > 256) h->last_dense_lds = 0;
    const size_t most = std::max(h->l1_dense_lds, std::max(h->l2_dense_lds, h->last_dense_lds));
    if (most && kkt_factor_dense_prepare(most) != hipSuccess) return ipm_refuse(h, RPM_E_DEVICE, "", "hipFuncSetAttribute");
    if (!env_is_zero("RPM_IPM_DENSE")) D.l1_dense_lds = h->l1_dense_lds;   // option "level1_dense"
    if (!env_is_zero("RPM_IPM_UPPER_DENSE")) {                             // option "upper_dense"
      D.l2_dense_lds = h->l2_dense_lds;
      D.last_dense_lds = h->last_dense_lds;
    }
  }
  h->factor_mt = p.max_rows <= 256 ? 4 : (p.max_rows <= 384 ? 6 : IPM_MT);
  // a few large instances: fewer sub-problems than two per CU -> 8 waves per workgroup, 3 tiles each (code 38: <3, 8>)
  if (p.nd && p.max_rows > 256 && p.max_rows <= 384 && B * p.subs.size() <= 512) h->factor_mt = 38;
  if (const char* fm = std::getenv("RPM_IPM_FACTOR_VARIANT")) h->factor_mt = std::atoi(fm);   // experiments: 4, 6, 8, 28 (<2,8>), 38 (<3,8>)
  if (const std::string why = factor_kernel_refusal(p); !why.empty()) return ipm_refuse(h, RPM_E_UNSUPPORTED, "", why);
  h->factor_lds = kkt_factor_lds_bytes(p);
  if (kkt_factor_prepare(h->factor_mt, h->factor_lds) != hipSuccess) return ipm_refuse(h, RPM_E_DEVICE, "", "hipFuncSetAttribute");
  return RPM_OK;
}
}  // namespace

extern "C" {

int rpm_ipm_create(rpm_engine* eng, rpm_ipm** out) {
  if (!eng || !out) return RPM_E_INVALID;
  *out = nullptr;
  Engine& e = eng->e;
  // hessian-approximation: exact = lpopc's finite-difference Hessian (rpm_eval_h); limited-memory = the reference's default
  // (Core/LpNLPWrapper.hpp:71): Ipopt's limited-memory BFGS, restated in rpm_ipm_lbfgs.hip
  const bool lbfgs = e.hessian_mode != RPM_HESSIAN_EXACT;
  if (e.shard_world > 1) {
    e.err = "rpm_ipm_create: interval-sharded engines are not supported (shard instances across ranks instead)";
    return RPM_E_UNSUPPORTED;
  }
  if (!e.dev) {
    int rc = device_init(e, 0);
    if (rc) return rc;
  }
  int rc = lbfgs ? RPM_OK : ensure_hessian(e);
  if (rc) return rc;
  std::unique_ptr<rpm_ipm> h(new (std::nothrow) rpm_ipm);   // a failure below destroys it: allocations freed, the engine released
  if (!h) return RPM_E_INVALID;
  h->eng = eng;
  h->lbfgs = lbfgs;
  e.ipm_attached += 1;   // freezes the engine's instance strides (rpm_set_option "instance_align"); released by ~rpm_ipm
  h->attached = true;
  auto fail = [&e](int code, const std::string& why) { e.err = "rpm_ipm_create: " + why; return code; };

  // ---- the plan
  std::string why;
  rc = build_ipm_plan(e, h->plan, &why, e.opt_ipm_nested != 0);
  // automatic: no interval structure to dissect, or sub-problems the factorisation kernel cannot hold (rows per block column, LDS:
  // e.g. a border grown by promoted unknowns on top of the intervals' separators) -> one band
  if (e.opt_ipm_nested == -1 && (rc || !factor_kernel_refusal(h->plan).empty()))
    rc = build_ipm_plan(e, h->plan, &why, 0);
  if (rc) return fail(rc, why);
  const IpmPlan& p = h->plan;

  // ---- the tables derived from it (rpm_ipm_tables.cpp)
  const IpmSubList subs = ipm_sub_list(p);
  const IpmFillList fill = ipm_fill_list(p);
  const bool one_pass = fill.one_pass && !std::getenv("RPM_IPM_TWO_PASS_FILL");
  const IpmFusedFill fused = one_pass && !env_is_zero("RPM_IPM_FUSED_FILL") ? ipm_fused_fill(subs, fill) : IpmFusedFill{};

  // ---- allocate and upload
  IpmDev& D = h->D;
  D.B = e.n_instances; D.n = p.n; D.m = p.m; D.ns = p.ns; D.nv = p.nv; D.Nt = p.Nt_alloc; D.Nb = p.Nb; D.nb = p.nb; D.b = p.b; D.CS = p.CS;
  D.nnz_jac = e.nnz_jac; D.nnz_h = e.nnz_h;
  D.sg = e.stride_g(); D.sv = e.stride_values(); D.kstride = p.storage();
  D.rhs_mult = 1;
  D.lb_on = lbfgs ? 1 : 0;
  if ((rc = upload_plan_tables(h.get(), fill, one_pass)) || (rc = alloc_state(h.get())) || (rc = upload_factor_tables(h.get(), subs, fused)))
    return fail(rc, h->err);

  // ---- kernel choice, events
  if ((rc = choose_kernels(h.get(), subs))) return fail(rc, h->err);
  for (hipEvent_t& e2 : h->ev)
    if (hipEventCreate(&e2) != hipSuccess) return fail(RPM_E_DEVICE, "hipEventCreate");
  *out = h.release();
  return RPM_OK;
}

void rpm_ipm_destroy(rpm_ipm* h) { delete h; }
const char* rpm_ipm_last_error(const rpm_ipm* h) { return h ? h->err.c_str() : "null solver"; }

int rpm_ipm_set_option(rpm_ipm* h, const char* key, double value) {
  if (!h || !key) return RPM_E_INVALID;
  IpmOpts& o = h->D.o;
  const std::string k(key);
  if (k == "tol") o.tol = value;
  else if (k == "max_iter") o.max_iter = int(value);
  else if (k == "mu_init") o.mu_init = value;
  else if (k == "bound_push") o.bound_push = value;
  else if (k == "bound_frac") o.bound_frac = value;
  else if (k == "warm_start_bound_push") o.ws_bound_push = value;
  else if (k == "warm_start_bound_frac") o.ws_bound_frac = value;
  else if (k == "warm_start_slack_bound_push") o.ws_slack_bound_push = value;
  else if (k == "warm_start_slack_bound_frac") o.ws_slack_bound_frac = value;
  else if (k == "warm_start_mult_bound_push") o.ws_mult_bound_push = value;
  else if (k == "warm_start_mult_init_max") o.ws_mult_init_max = value;
  else if (k == "delta_c") o.delta_c = value;
  else if (k == "max_line_search") o.max_ls = int(value);
  else if (k == "restoration") o.resto = value != 0.0;
  else if (k == "acceptable_tol") o.acceptable_tol = value;
  else if (k == "acceptable_iter") o.acceptable_iter = int(value);
  else if (k == "restoration_max_iter") o.resto_max = int(value);
  else if (k == "bound_relax_factor") { if (!(value >= 0.0)) return ipm_refuse(h, RPM_E_INVALID, "", "bound_relax_factor must be >= 0"); o.bound_relax = value; }
  else if (k == "max_soc") o.max_soc = std::max(0, int(value));
  else if (k == "sens_refine") { if (!(value >= -1.0 && value <= 8.0)) return ipm_refuse(h, RPM_E_INVALID, "", "sens_refine: 0 .. 8 rounds, or -1 (automatic)"); h->sens.refine = int(value); }
  else if (k == "sens_constant_step") { if (!(value > 0.0 && value <= 0.1)) return ipm_refuse(h, RPM_E_INVALID, "", "sens_constant_step: a relative step in (0, 0.1]"); h->sens.const_step = value; }
  else if (k == "sigma_cap") o.sigma_cap = value;      // experiment
  else if (k == "init_ls_multipliers") o.init_ls_mult = value != 0.0;
  else if (k == "nlp_scaling") { o.nlp_scaling = value != 0.0; h->D.scal_on = o.nlp_scaling; }
  else if (k == "nlp_scaling_max_gradient") { if (!(value > 0.0)) return ipm_refuse(h, RPM_E_INVALID, "", "nlp_scaling_max_gradient must be > 0"); o.scal_gmax = value; }
  else if (k == "ic_hot_start") o.ic_hot = value != 0.0;
  else if (k == "ic_hot_min") o.ic_hot_min = value;
  else if (k == "mu_strategy") {       // 0 monotone (default), 1 adaptive: LOQO oracle + kkt-error globalisation
    if (value != 0.0 && value != 1.0) return ipm_refuse(h, RPM_E_INVALID, "", "mu_strategy: 0 (monotone) or 1 (adaptive)");
    o.mu_adaptive = int(value);
  }
  else if (k == "restoration_penalty") o.resto_rho = value;
  else if (k == "level1_dense") {   // level 1 of the nested dissection on kkt_factor_dense_kernel (default where the interval blocks fit it)
    if (value != 0.0 && !h->l1_dense_lds) return ipm_refuse(h, RPM_E_UNSUPPORTED, "", "level1_dense: no nested dissection, or an interval block of more than 21 block rows");
    h->D.l1_dense_lds = value != 0.0 ? h->l1_dense_lds : 0;
  }
  else if (k == "upper_dense") {    // the levels above the interval blocks on kkt_factor_dense_kernel too (default where their sub-problems fit it)
    h->D.l2_dense_lds = value != 0.0 ? h->l2_dense_lds : 0;
    h->D.last_dense_lds = value != 0.0 ? h->last_dense_lds : 0;
    h->D.last_dense_corner = value == 2.0 ? 0 : 1;   // 2: the last level's corner by kkt_factor_kernel's unblocked elimination
  }
  else if (k == "fused_fill") {     // level-1 blocks assembled inside kkt_factor_dense_kernel (default where that kernel runs and the tables exist)
    if (value != 0.0 && !h->D.df_map) return ipm_refuse(h, RPM_E_UNSUPPORTED, "", "fused_fill: level 1 does not run on kkt_factor_dense_kernel");
    h->D.df_on = value != 0.0;
  }
  else if (k == "trace") {          // keep the first `value` iterations of every instance (rpm_ipm_get_trace)
    const int cap = int(value);
    if (cap < 0 || cap > 100000) return ipm_refuse(h, RPM_E_INVALID, "", "trace: 0 ... 100000 records");
    h->D.trace = nullptr;
    h->D.trace_cap = 0;
    if (cap > 0) {
      int rc = ipm_alloc(h, &h->D.trace, size_t(h->D.B) * cap * IPM_TRACE);
      if (rc) return rc;
      h->D.trace_cap = cap;
    }
  }
  else return ipm_refuse(h, RPM_E_INVALID, "", "unknown option " + k);
  return RPM_OK;
}

int rpm_ipm_get_info(rpm_ipm* h, int* kkt_order, int* band_order, int* half_bandwidth, int* border, long long* storage_doubles,
                     int* n_slacks) {
  if (!h) return RPM_E_INVALID;
  if (kkt_order) *kkt_order = h->plan.Nt;
  if (band_order) *band_order = h->plan.Nb;
  if (half_bandwidth) *half_bandwidth = h->plan.b;
  if (border) *border = h->plan.nb;
  if (storage_doubles) *storage_doubles = h->plan.storage();
  if (n_slacks) *n_slacks = h->plan.ns;
  return RPM_OK;
}

/* the factorisation's sub-problems (one without nested dissection; the interval blocks followed by the separator system
 * with it): 5 ints each — order, banded part, border, half bandwidth, doubles per stored column */
int rpm_ipm_get_subproblems(rpm_ipm* h, int capacity, int* geom, int* n_sub) {
  if (!h || !n_sub) return RPM_E_INVALID;
  const std::vector<KktSub> subs = ipm_sub_list(h->plan).subs;
  const int n = int(subs.size());
  *n_sub = n;
  if (!geom) return RPM_OK;
  if (capacity < n) return RPM_E_INVALID;
  for (int i = 0; i < n; ++i) {
    const KktGeom& s = subs[size_t(i)].g;
    int* g = geom + 5 * i;
    g[0] = s.Nt; g[1] = s.Nb; g[2] = s.nb; g[3] = s.b; g[4] = s.CS;
  }
  return RPM_OK;
}

int rpm_ipm_get_stats(rpm_ipm* h, int* iterations, int* factorizations, int* trial_points) {
  if (!h) return RPM_E_INVALID;
  if (iterations) *iterations = h->stats.total_iterations;
  if (factorizations) *factorizations = h->stats.total_factorizations;
  if (trial_points) *trial_points = h->stats.total_trials;
  return RPM_OK;
}

int rpm_ipm_get_kernel_times(rpm_ipm* h, double* factor_ms, double* substitution_ms) {
  if (!h) return RPM_E_INVALID;
  if (factor_ms) *factor_ms = h->stats.factor_ms;
  if (substitution_ms) *substitution_ms = h->stats.solve_ms;
  return RPM_OK;
}

int rpm_ipm_get_restorations(rpm_ipm* h, int* per_instance) {
  if (!h || !per_instance || h->h_inst.empty()) return RPM_E_INVALID;
  for (int bi = 0; bi < h->D.B; ++bi) per_instance[bi] = h->h_inst[bi].n_resto;
  return RPM_OK;
}

int rpm_ipm_get_trace(rpm_ipm* h, int instance, int capacity, double* records, int* n_records) {
  if (!h || instance < 0 || instance >= h->D.B || !records || !n_records) return RPM_E_INVALID;
  if (!h->D.trace || h->h_inst.empty()) { *n_records = 0; return RPM_OK; }
  const int n = std::min(std::min(h->h_inst[instance].iter, h->D.trace_cap), capacity);
  IPM_TRY(h, hipMemcpy(records, h->D.trace + size_t(instance) * h->D.trace_cap * IPM_TRACE, size_t(n) * IPM_TRACE * sizeof(double),
                       hipMemcpyDeviceToHost));
  *n_records = n;
  return RPM_OK;
}

// the KKT layout is shared by all instances: the first variable of x_l / x_u (one instance, n) that is fixed where the plan has it
// free or the other way round, -1 if none
static const char* const FIXED_FREE_CHANGE = " changes between fixed and free (the KKT layout is shared by all instances)";
static int fixed_free_change(const IpmPlan& p, const double* x_l, const double* x_u) {
  for (int i = 0; i < p.n; ++i)
    if ((x_l[i] == x_u[i]) != (p.fixed[i] != 0)) return i;
  return -1;
}

int rpm_ipm_set_bounds(rpm_ipm* h, int instance, const double* x_l, const double* x_u) {
  if (!h || !x_l || !x_u || instance < 0 || instance >= h->D.B) return RPM_E_INVALID;
  const IpmPlan& p = h->plan;
  if (const int i = fixed_free_change(p, x_l, x_u); i >= 0)
    return ipm_refuse(h, RPM_E_INVALID, "rpm_ipm_set_bounds", "variable " + std::to_string(i) + FIXED_FREE_CHANGE);
  // caller arrays go through the engine's staging slots (rpm_device.hip), not the runtime's pageable-copy path
  Engine& e = h->eng->e;
  int rc = dev_upload(e, h->D.vl0 + size_t(instance) * p.nv, x_l, size_t(p.n), STAGE_X);
  if (!rc) rc = dev_upload(e, h->D.vu0 + size_t(instance) * p.nv, x_u, size_t(p.n), STAGE_G);
  if (!rc) rc = dev_sync(e);
  return ipm_eng_fail(h, rc);
}

/* variable bounds of all instances at once: x_l, x_u are n_instances x n (host), e.g. the measured initial states of a
 * receding-horizon sweep; two copies instead of 2 n_instances */
int rpm_ipm_set_all_bounds(rpm_ipm* h, const double* x_l, const double* x_u) {
  if (!h || !x_l || !x_u) return RPM_E_INVALID;
  const IpmPlan& p = h->plan;
  const size_t B = size_t(h->D.B);
  for (size_t bi = 0; bi < B; ++bi)
    if (const int i = fixed_free_change(p, x_l + bi * p.n, x_u + bi * p.n); i >= 0)
      return ipm_refuse(h, RPM_E_INVALID, "rpm_ipm_set_all_bounds",
                        "instance " + std::to_string(bi) + ", variable " + std::to_string(i) + FIXED_FREE_CHANGE);
  Engine& e = h->eng->e;
  hipStream_t st = static_cast<hipStream_t>(dev_stream(e));
  double *sl = nullptr, *su = nullptr;
  int rc = dev_stage_reserve(e, STAGE_X, B * p.n, &sl, nullptr);
  if (!rc) rc = dev_stage_reserve(e, STAGE_G, B * p.n, &su, nullptr);
  if (rc) return ipm_eng_fail(h, rc);
  std::memcpy(sl, x_l, B * p.n * sizeof(double));
  std::memcpy(su, x_u, B * p.n * sizeof(double));
  IPM_TRY(h, hipMemcpy2DAsync(h->D.vl0, size_t(p.nv) * sizeof(double), sl, size_t(p.n) * sizeof(double), size_t(p.n) * sizeof(double), B,
                              hipMemcpyHostToDevice, st));
  IPM_TRY(h, hipMemcpy2DAsync(h->D.vu0, size_t(p.nv) * sizeof(double), su, size_t(p.n) * sizeof(double), size_t(p.n) * sizeof(double), B,
                              hipMemcpyHostToDevice, st));
  IPM_TRY(h, hipStreamSynchronize(st));
  return RPM_OK;
}

}  // extern "C"

namespace {
// the measured initial states of a phase: every argument error, decided on the host.  All nx initial states must be fixed in the
// plan, because the KKT layout is shared by all instances.
int initial_states_check(rpm_ipm* h, const char* who, int phase, const void* state0) {
  const Engine& e = h->eng->e;
  if (phase < 0 || phase >= e.P) return ipm_refuse(h, RPM_E_INVALID, who, "phase " + std::to_string(phase) + " is out of range");
  if (!state0) return ipm_refuse(h, RPM_E_INVALID, who, "state0 is NULL");
  const PhaseHost& p = e.ph[size_t(phase)];
  for (int j = 0; j < p.nx; ++j) {
    const int i = p.var0 + j * (p.N + 1);
    if (!h->plan.fixed[size_t(i)])
      return ipm_refuse(h, RPM_E_INVALID, who, "variable " + std::to_string(i) + " (initial state " + std::to_string(j) +
                                                   ") is free in the solver's plan (the KKT layout is shared by all instances)");
  }
  return RPM_OK;
}
}  // namespace

extern "C" {

/* vl0 = vu0 = state0[b][j] at variable x_state0 + j (N + 1) of every instance: one small launch on `stream`, no copy, no
 * synchronisation */
int rpm_ipm_set_initial_states_dev(rpm_ipm* h, int phase, const double* d_state0, void* stream) {
  if (!h) return RPM_E_INVALID;
  int rc = initial_states_check(h, "rpm_ipm_set_initial_states_dev", phase, d_state0);
  if (rc) return rc;
  const PhaseHost& p = h->eng->e.ph[size_t(phase)];
  ipm_launch_set_state0(h->D, p.var0, p.N + 1, p.nx, d_state0, static_cast<hipStream_t>(stream));
  return launch_check(h, "ipm_set_state0_kernel");
}

/* the same from a host array (n_instances x nx) through the engine's staging slot; blocking */
int rpm_ipm_set_initial_states(rpm_ipm* h, int phase, const double* state0) {
  if (!h) return RPM_E_INVALID;
  int rc = initial_states_check(h, "rpm_ipm_set_initial_states", phase, state0);
  if (rc) return rc;
  Engine& e = h->eng->e;
  const PhaseHost& p = e.ph[size_t(phase)];
  double *d_x, *d_l, *d_zL, *d_zU;
  if ((rc = host_form(h, &d_x, &d_l, &d_zL, &d_zU))) return rc;
  if ((rc = dev_upload(e, d_x, state0, size_t(h->D.B) * p.nx, STAGE_X))) return ipm_eng_fail(h, rc);
  ipm_launch_set_state0(h->D, p.var0, p.N + 1, p.nx, d_x, static_cast<hipStream_t>(dev_stream(e)));
  if ((rc = launch_check(h, "ipm_set_state0_kernel"))) return rc;
  return ipm_eng_fail(h, dev_sync(e));
}

}  // extern "C"

namespace rpm {
int ipm_check_start_args(rpm_ipm* h, const char* who, const char* need, bool warm, const void* x, const void* lambda, const void* z_L,
                         const void* z_U) {
  if (!x || (warm && !lambda)) return ipm_refuse(h, RPM_E_INVALID, who, need);
  if (warm && (!z_L != !z_U)) return ipm_refuse(h, RPM_E_INVALID, who, "z_L and z_U are given together or both NULL");
  return RPM_OK;
}

int ipm_start(rpm_ipm* h, bool warm, const double* d_x, const double* d_lambda, const double* d_zL, const double* d_zU, hipStream_t st) {
  Engine& e = h->eng->e;
  IpmDev& D = h->D;
  const IpmPlan& p = h->plan;
  const unsigned B = unsigned(D.B);
  dev_forget_persistent(e);   // the first Jacobian evaluation of this solve writes the constant block of D.jac, the later ones skip it
  if (h->lbfgs) lb_launch_reset(D, st);
  IPM_TRY(h, hipMemcpyAsync(D.xt, d_x, size_t(B) * p.n * sizeof(double), hipMemcpyDeviceToDevice, st));
  ipm_launch_init(D, d_x, st, warm ? 1 : 0);
  int rc;
  const bool scal = D.scal_on != 0;
  if (scal) {   // Ipopt's gradient-based scaling: factors from the gradients at the caller's starting point (before it is pushed inside its bounds)
    if ((rc = dev_eval_obj(e, D.xt, D.objt, D.grad, st))) return ipm_eng_fail(h, rc);
    if ((rc = dev_eval_cons(e, D.xt, D.gt, D.jac, 3 | 4 | 16, st))) return ipm_eng_fail(h, rc);
    ipm_launch_scaling_factors(D, st);
    // this evaluation has written D.jac's constant block, which the later ones leave alone: it is scaled here, once
    if (e.nnz_jac > D.nnz_var) ipm_launch_scale(D, nullptr, D.jac, D.nnz_var, e.nnz_jac, nullptr, nullptr, st);
  }
  ipm_launch_pack_x(D, st);
  rc = dev_eval_cons(e, D.xe, D.g, nullptr, 1 | 4, st);
  if (rc) return ipm_eng_fail(h, rc);
  if (scal) ipm_launch_scale(D, D.g, nullptr, 0, 0, nullptr, nullptr, st);
  ipm_launch_init_slack(D, st, warm ? 1 : 0);
  if (warm) ipm_launch_warm_duals(D, D.xt, d_lambda, d_zL, d_zU, st);   // (D.xt: the caller's x as it came)
  return launch_check(h, "ipm_init");
}

int host_form(rpm_ipm* h, double** d_x, double** d_l, double** d_zL, double** d_zU) {
  const size_t Bn = size_t(h->D.B) * h->plan.n, Bm = size_t(h->D.B) * std::max(h->plan.m, 1);
  if (!h->d_host_form) {
    int rc = ipm_alloc(h, &h->d_host_form, 3 * Bn + Bm);
    if (rc) return rc;
  }
  *d_x = h->d_host_form;
  *d_l = *d_x + Bn;
  *d_zL = *d_l + Bm;
  *d_zU = *d_zL + Bn;
  return RPM_OK;
}
}  // namespace rpm

namespace {
int ipm_solve_dev(rpm_ipm* h, bool warm, double* d_x, double* d_lambda, double* d_zL, double* d_zU, double* obj, int* status,
                  int* iterations, double* kkt_error, void* stream) {
  Engine& e = h->eng->e;
  IpmDev& D = h->D;
  hipStream_t st = static_cast<hipStream_t>(dev_stream(e));
  h->hold.solve_begins();
  h->stats = IpmStats{};
  if (D.sg != e.stride_g() || D.sv != e.stride_values())   // rpm_set_option refuses this while a solver is attached; belt and braces
    return ipm_refuse(h, RPM_E_INVALID, "rpm_ipm_solve_dev", "the engine's instance strides changed after rpm_ipm_create");
  // Ordering contract (rpm_hip.h): the loop runs on the engine's private stream.  Its first read of d_x / its first write of
  // d_lambda wait for everything the caller queued on `stream` before this call; the call returns after the solver's stream
  // has drained, so the results are complete for every stream and for the host.
  IPM_TRY(h, hipEventRecord(h->ev[0], static_cast<hipStream_t>(stream)));
  IPM_TRY(h, hipStreamWaitEvent(st, h->ev[0], 0));

  int rc = ipm_start(h, warm, d_x, d_lambda, d_zL, d_zU, st);
  if (rc) return rc;
  const IpmLoop L = ipm_loop(h);
  for (;;) {
    if ((rc = L.evaluate_and_residual())) return rc;
    if (h->h_cnt[0] == 0) break;
    h->stats.total_iterations += 1;
    if (!h->lbfgs && (rc = L.exact_hessian())) return rc;
    if ((rc = L.factor_with_inertia_correction())) return rc;
    if ((rc = L.substitute())) return rc;
    if ((rc = L.line_search())) return rc;
    if ((rc = L.update())) return rc;
  }
  return L.collect(d_x, d_lambda, d_zL, d_zU, obj, status, iterations, kkt_error);
}

// The host-pointer solves: the caller's arrays through the engine's staging slots (or its page-lock registrations) into the solver's
// device block, the solve, the results back the same way.  Cold start: only x goes up, lambda comes back where it is not NULL.
int solve_from_host(rpm_ipm* h, bool warm, double* x, double* lambda, double* z_L, double* z_U, double* obj, int* status,
                    int* iterations, double* kkt_error) {
  Engine& e = h->eng->e;
  const size_t Bn = size_t(h->D.B) * h->plan.n, Bm = size_t(h->D.B) * h->plan.m;
  const bool with_z = warm && z_L;
  double *d_x, *d_l, *d_zL, *d_zU;
  int rc = host_form(h, &d_x, &d_l, &d_zL, &d_zU);
  if (rc) return rc;
  rc = dev_upload(e, d_x, x, Bn, STAGE_X);
  if (!rc && warm) rc = dev_upload(e, d_l, lambda, Bm, STAGE_LAMBDA);
  if (!rc && with_z) rc = dev_upload(e, d_zL, z_L, Bn, STAGE_G);
  if (!rc && with_z) rc = dev_upload(e, d_zU, z_U, Bn, STAGE_GRAD);
  if (!rc) rc = dev_sync(e);                                                                   // nothing in flight when the solve starts
  if (rc) return ipm_eng_fail(h, rc);
  rc = ipm_solve_dev(h, warm, d_x, d_l, with_z ? d_zL : nullptr, with_z ? d_zU : nullptr, obj, status, iterations, kkt_error, nullptr);
  if (rc) return rc;
  rc = dev_download(e, x, d_x, Bn, STAGE_X);
  if (!rc && lambda) rc = dev_download(e, lambda, d_l, Bm, STAGE_LAMBDA);
  if (!rc && with_z) rc = dev_download(e, z_L, d_zL, Bn, STAGE_G);
  if (!rc && with_z) rc = dev_download(e, z_U, d_zU, Bn, STAGE_GRAD);
  return ipm_eng_fail(h, rc);
}

int bound_multipliers_ready(rpm_ipm* h, const double* z_L, const double* z_U) {
  if (!z_L || !z_U) return ipm_refuse(h, RPM_E_INVALID, "rpm_ipm_get_bound_multipliers", "z_L or z_U is NULL");
  if (!h->hold.multipliers_ready()) return ipm_refuse(h, RPM_E_INVALID, "rpm_ipm_get_bound_multipliers", "no solve has finished");
  return RPM_OK;
}
}  // namespace

extern "C" {

int rpm_ipm_solve_dev(rpm_ipm* h, double* d_x, double* d_lambda, double* obj, int* status, int* iterations, double* kkt_error,
                      void* stream) {
  if (!h || !d_x) return RPM_E_INVALID;
  return ipm_solve_dev(h, false, d_x, d_lambda, nullptr, nullptr, obj, status, iterations, kkt_error, stream);
}

int rpm_ipm_solve_warm_dev(rpm_ipm* h, double* d_x, double* d_lambda, double* d_z_L, double* d_z_U, double* obj, int* status,
                           int* iterations, double* kkt_error, void* stream) {
  if (!h) return RPM_E_INVALID;
  int rc = ipm_check_start_args(h, "rpm_ipm_solve_warm", "x and lambda are required", true, d_x, d_lambda, d_z_L, d_z_U);
  if (rc) return rc;
  return ipm_solve_dev(h, true, d_x, d_lambda, d_z_L, d_z_U, obj, status, iterations, kkt_error, stream);
}

int rpm_ipm_get_bound_multipliers_dev(rpm_ipm* h, double* d_z_L, double* d_z_U, void* stream) {
  if (!h) return RPM_E_INVALID;
  int rc = bound_multipliers_ready(h, d_z_L, d_z_U);
  if (rc) return rc;
  ipm_launch_bound_multipliers(h->D, d_z_L, d_z_U, static_cast<hipStream_t>(stream));
  return launch_check(h, "ipm_bound_mult_kernel");
}

int rpm_ipm_get_bound_multipliers(rpm_ipm* h, double* z_L, double* z_U) {
  if (!h) return RPM_E_INVALID;
  int rc = bound_multipliers_ready(h, z_L, z_U);
  if (rc) return rc;
  Engine& e = h->eng->e;
  hipStream_t st = static_cast<hipStream_t>(dev_stream(e));
  double *d_x, *d_l, *d_zL, *d_zU;
  if ((rc = host_form(h, &d_x, &d_l, &d_zL, &d_zU))) return rc;
  const size_t Bn = size_t(h->D.B) * h->plan.n;
  ipm_launch_bound_multipliers(h->D, d_zL, d_zU, st);
  if ((rc = launch_check(h, "ipm_bound_mult_kernel"))) return rc;
  rc = dev_download(e, z_L, d_zL, Bn, STAGE_X);
  if (!rc) rc = dev_download(e, z_U, d_zU, Bn, STAGE_G);
  return ipm_eng_fail(h, rc);
}

int rpm_ipm_solve(rpm_ipm* h, double* x, double* lambda, double* obj, int* status, int* iterations, double* kkt_error) {
  if (!h || !x) return RPM_E_INVALID;
  return solve_from_host(h, false, x, lambda, nullptr, nullptr, obj, status, iterations, kkt_error);
}

int rpm_ipm_solve_warm(rpm_ipm* h, double* x, double* lambda, double* z_L, double* z_U, double* obj, int* status, int* iterations,
                       double* kkt_error) {
  if (!h) return RPM_E_INVALID;
  int rc = ipm_check_start_args(h, "rpm_ipm_solve_warm", "x and lambda are required", true, x, lambda, z_L, z_U);
  if (rc) return rc;
  return solve_from_host(h, true, x, lambda, z_L, z_U, obj, status, iterations, kkt_error);
}

}  // extern "C"
