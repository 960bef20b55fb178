// rpm_ipm_sens.hip — row f-2: first-order sensitivities of a solution to variables that are fixed in the solver's plan (the measured
// initial states of a receding-horizon sweep, t0, tf), and the predictor that applies them.  Column k solves the solver's own
// reduced system (13) — assembled and factored at the state the solver holds by the launchers of an iteration — against minus
// column var_index[k] of the matrix's off-diagonal blocks; all columns of all instances go through ONE pass of the substitution
// kernels (IpmDev::rhs_mult).  Three kernels of its own: the right-hand-side gather, the unpack and the predictor.  DESIGN.md f-2.
// The same for the instances' constants (rpm_ipm_constant_sensitivities): the right-hand side of a constant is minus a central
// difference of the engine's own evaluations at perturbed constants — two more kernels, the perturbed constants and their gather.
#include <cstdint>
#include <limits>
#include <vector>

#include "rpm_device_restore.hpp"
#include "rpm_ipm_solver.hpp"

using namespace rpm;

namespace rpm {

// Option "sens_refine": the factorisation starts at this delta_w instead of 0 — the pivot-free LDL^T is stable on a quasi-definite
// matrix, and W + Sigma of a plan without curvature in some unknowns is only semi-definite to working precision —, and the
// refinement's residual is taken against the matrix WITHOUT it, so the rounds remove what it adds.  sqrt(2^-52) rounded down.
constexpr double SENS_REFINE_DELTA_W = 1e-8;

struct SensPars {   // the parameter list, by value
  int n_par;
  int idx[IPM_SENS_MAX_PAR];
};

// One thread per group of the source table (IpmSensTable, rpm_ipm.hpp): ws[par][instance][dst] = -(sum of the group's sources in list
// order, one IEEE addition after the other).  Groups ascend by (parameter, position), so a wave writes ascending positions of
// one right-hand side; what no group writes stays at the zero the work space was filled with.
__global__ __launch_bounds__(256) void ipm_sens_rhs_kernel(IpmDev D, const int* __restrict__ ptr, const int* __restrict__ par,
                                                          const int* __restrict__ dst, const int* __restrict__ src, int n_groups,
                                                          double* __restrict__ ws) {
  const int bi = blockIdx.y, g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  const double *hess = D.hess + size_t(bi) * D.nnz_h, *jac = D.jac + size_t(bi) * D.sv;
  auto value = [&](int s) { return (s >> 28) ? jac[s & 0x0fffffff] : hess[s & 0x0fffffff]; };
  const int j0 = ptr[g], j1 = ptr[g + 1];
  double acc = value(src[j0]);
  for (int j = j0 + 1; j < j1; ++j) acc += value(src[j]);
  ws[(size_t(par[g]) * D.B + bi) * D.Nt + dst[g]] = -acc;
}

// ---- sensitivities to the instances' constants (rpm_ipm_constant_sensitivities): the right-hand side of constant k is minus the
// central difference, over each instance's own step h = rho (1 + |c_k|), of grad f + J' lambda (free variables) and of g (rows).
// The perturbed constants of every instance: cp / cm (B x nconst) are the constants the kernels read (consts, `stride` doubles
// between instances, 0: shared) with entry k replaced by c_k + h / c_k - h; hbuf[b] = h.
__global__ __launch_bounds__(256) void ipm_sens_perturb_kernel(int nconst, const double* __restrict__ consts, int stride, int k, double rho,
                                                              double* __restrict__ cp, double* __restrict__ cm, double* __restrict__ hbuf) {
  const int bi = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nconst) return;
  const double* c = consts + size_t(bi) * stride;
  const double h = rho * (1.0 + fabs(c[k]));
  const double v = c[j];
  cp[size_t(bi) * nconst + j] = j == k ? v + h : v;
  cm[size_t(bi) * nconst + j] = j == k ? v - h : v;
  if (j == k) hbuf[bi] = h;
}

// One thread per entry of the column table (IpmConstTable, rpm_ipm.hpp; tab: var, var_pos (n_free each), ptr (n_free + 1), ent,
// ent_row (n_ent each), row_pos (m)), grid y = instance.  Free variable i: acc = grad+[i] - grad-[i], then for the [NL] triplets t of
// column i in ascending order acc = acc + (J+[t] - J-[t]) * lambda[row(t)] (product, then sum), and ws = -(acc / (h + h)); row r:
// ws = -((g+[r] - g-[r]) / (h + h)).  Written at (k, instance, position) of the zero-filled work space, as ipm_sens_rhs_kernel does.
__global__ __launch_bounds__(256) void ipm_sens_const_rhs_kernel(IpmDev D, const int* __restrict__ tab, int n_free, int n_ent, int k,
                                                                const double* __restrict__ grad_p, const double* __restrict__ grad_m,
                                                                const double* __restrict__ g_p, const double* __restrict__ g_m,
                                                                const double* __restrict__ jac_p, const double* __restrict__ jac_m,
                                                                const double* __restrict__ hbuf, double* __restrict__ ws) {
  const int bi = blockIdx.y, u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_free + D.m) return;
  const int *var = tab, *var_pos = var + n_free, *ptr = var_pos + n_free, *ent = ptr + n_free + 1, *ent_row = ent + n_ent, *row_pos = ent_row + n_ent;
  const double h = hbuf[bi], h2 = h + h;
  double* w = ws + (size_t(k) * D.B + bi) * D.Nt;
  if (u < n_free) {
    const int i = var[u];
    const double *jp = jac_p + size_t(bi) * D.sv, *jm = jac_m + size_t(bi) * D.sv, *lam = D.lam + size_t(bi) * D.m;
    double acc = grad_p[size_t(bi) * D.n + i] - grad_m[size_t(bi) * D.n + i];
    for (int q = ptr[u]; q < ptr[u + 1]; ++q) {
      const int t = ent[q];
      acc = acc + (jp[t] - jm[t]) * lam[ent_row[q]];
    }
    w[var_pos[u]] = -(acc / h2);
  } else {
    const int r = u - n_free;
    w[row_pos[r]] = -((g_p[size_t(bi) * D.sg + r] - g_m[size_t(bi) * D.sg + r]) / h2);
  }
}

// KKT order -> dx (B x n_par x n) and dlambda (B x n_par x m, or NULL): free variables and rows through pos, 1 at the column's own
// variable (a column of a constant has none: idx -1), 0 at every other fixed one; an instance whose record says it was left out
// (status != 0) gets NaN.
__global__ __launch_bounds__(256) void ipm_sens_unpack_kernel(IpmDev D, SensPars P, const int* __restrict__ fixed,
                                                             const double* __restrict__ ws, double* __restrict__ dx,
                                                             double* __restrict__ dlam) {
  const int bi = blockIdx.y, k = blockIdx.z, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.n + D.m) return;
  const bool left_out = D.inst[bi].status != 0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double* w = ws + (size_t(k) * D.B + bi) * D.Nt;
  const size_t col = size_t(bi) * P.n_par + k;
  if (i < D.n) {
    const double v = fixed[i] ? (i == P.idx[k] ? 1.0 : 0.0) : w[D.pos[i]];
    dx[col * D.n + i] = left_out ? nan : v;
  } else if (dlam) {
    const int r = i - D.n;
    dlam[col * D.m + r] = left_out ? nan : w[D.pos[D.nv + r]];
  }
}

// Iterative refinement of the columns (option "sens_refine"): res = rhs0 - K sol, row by row from the SOURCES of the matrix —
// the Hessian and Jacobian triplets, -1 at the slacks, the diagonal terms as ipm_assemble_kernel forms them — in the fixed order of
// the row table, one thread per row: deterministic, and independent of what the factorisation left in the storage.
// rows: ptr (n_rows + 1), position of every row (n_rows), then per entry its code (kind << 28 | index: 0 Hessian triplet, 1 Jacobian
// triplet, 2 the slack's -1, 3 diagonal of variable or slack i, 4 diagonal of constraint r) and the position of its column.
__global__ __launch_bounds__(256) void ipm_sens_residual_kernel(IpmDev D, const int* __restrict__ rows, int n_rows, int n_ent,
                                                               const double* __restrict__ rhs0, const double* __restrict__ sol,
                                                               double* __restrict__ res, double dw_floor) {
  const int bi = blockIdx.y, k = blockIdx.z, u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_rows) return;
  const IpmInst& S = D.inst[bi];
  const int *ptr = rows, *rpos = rows + n_rows + 1, *code = rpos + n_rows, *col = code + n_ent;
  const size_t off = (size_t(k) * D.B + bi) * D.Nt;
  const double *hess = D.hess + size_t(bi) * D.nnz_h, *jac = D.jac + size_t(bi) * D.sv;
  const double *v = D.v + size_t(bi) * D.nv, *vl = D.vl + size_t(bi) * D.nv, *vu = D.vu + size_t(bi) * D.nv;
  const double *zL = D.zL + size_t(bi) * D.nv, *zU = D.zU + size_t(bi) * D.nv;
  double acc = rhs0[off + rpos[u]];
  for (int j = ptr[u]; j < ptr[u + 1]; ++j) {
    const int kind = code[j] >> 28, i = code[j] & 0x0fffffff;
    double a;
    if (kind == 0) a = hess[i];
    else if (kind == 1) a = jac[i];
    else if (kind == 2) a = -1.0;
    else if (kind == 4) a = -D.o.delta_c;
    else {
      const double l = vl[i], up = vu[i];
      a = 1.0;
      if (l != up) {
        a = S.delta_w > dw_floor ? S.delta_w : 0.0;   // (the floor the refined call factors with is not part of the matrix)
        const double cap = D.o.sigma_cap > 0 ? D.o.sigma_cap : 1e300;
        if (l > -IPM_INF) a += fmin(zL[i] / (v[i] - l), cap);
        if (up < IPM_INF) a += fmin(zU[i] / (up - v[i]), cap);
      }
    }
    acc -= a * sol[off + col[j]];
  }
  res[off + rpos[u]] = acc;
}

__global__ __launch_bounds__(256) void ipm_sens_correct_kernel(long long len, const double* __restrict__ d, double* __restrict__ sol) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < len) sol[i] += d[i];
}

// The predictor: out[b] = in[b], then for k ascending out[b] = out[b] + S[b][k] * delta[b][k] (product, then sum: the build keeps
// them separate roundings), for x (blocks [0, xblocks) of the grid's x) and, when given, for lambda (the blocks after them).
// Bandwidth bound — n_par rows of S are read per row written —: a thread takes two neighbouring entries and reads a row's pair
// with one 16-byte load wherever the pair is 16-byte aligned (every row when the length is even; every other row otherwise).
__global__ __launch_bounds__(256) void ipm_sens_apply_kernel(int n, int m, int n_par, int xblocks, const double* __restrict__ dx,
                                                            const double* __restrict__ dlam, const double* __restrict__ delta,
                                                            const double* __restrict__ x, double* __restrict__ x_out,
                                                            const double* __restrict__ lam, double* __restrict__ lam_out) {
  const int bi = blockIdx.y;
  const bool is_x = int(blockIdx.x) < xblocks;
  const int len = is_x ? n : m, blk = is_x ? int(blockIdx.x) : int(blockIdx.x) - xblocks;
  const int i0 = (blk * int(blockDim.x) + int(threadIdx.x)) * 2;
  if (i0 >= len) return;
  const bool two = i0 + 1 < len;
  const double* S = (is_x ? dx : dlam) + size_t(bi) * n_par * len + i0;
  const double* in = (is_x ? x : lam) + size_t(bi) * len + i0;
  double* out = (is_x ? x_out : lam_out) + size_t(bi) * len + i0;
  const double* dl = delta + size_t(bi) * n_par;
  double a0 = in[0], a1 = two ? in[1] : 0.0;
  for (int k = 0; k < n_par; ++k) {
    const double* row = S + size_t(k) * len;
    const double d = dl[k];
    if (two && (reinterpret_cast<uintptr_t>(row) & 15) == 0) {
      const double2 s2 = *reinterpret_cast<const double2*>(row);
      a0 = a0 + s2.x * d;
      a1 = a1 + s2.y * d;
    } else {
      a0 = a0 + row[0] * d;
      if (two) a1 = a1 + row[1] * d;
    }
  }
  out[0] = a0;
  if (two) out[1] = a1;
}

}  // namespace rpm

namespace {

template <class T>
int sens_room(rpm_ipm* h, T** p, size_t* cap, size_t count) {   // grown only; what growing replaces is freed (the stream is idle between calls)
  if (*p && count <= *cap) return RPM_OK;
  if (*p) {
    IPM_TRY(h, hipFree(*p));
    *p = nullptr;
    *cap = 0;
  }
  IPM_TRY(h, hipMalloc(reinterpret_cast<void**>(p), (count ? count : 1) * sizeof(T)));
  *cap = count;
  return RPM_OK;
}

int sens_check_solver(rpm_ipm* h, const std::string& who, bool need_state);   // what does not depend on the list

// every refusal of rpm_ipm_sensitivities[_dev] / rpm_ipm_debug_sensitivity_rhs, on the host, before anything is queued; *table: the
// source table of the list (NULL: only checked)
int sens_check(rpm_ipm* h, const std::string& who, int n_par, const int* var_index, bool need_state, IpmSensTable* table) {
  const Engine& e = h->eng->e;
  std::string why;
  if (int rc = ipm_sens_table(h->plan, h->lbfgs ? 0 : e.nnz_h, e.hes_i.data(), e.hes_j.data(), n_par, var_index, table, &why))
    return ipm_refuse(h, rc, who, why);
  return sens_check_solver(h, who, need_state);
}
// the same for a list of constants (rpm_ipm_constant_sensitivities[_dev], rpm_ipm_debug_constant_sensitivity_rhs, the predictor)
int const_check(rpm_ipm* h, const std::string& who, int n_par, const int* const_index, bool need_state) {
  std::string why;
  if (int rc = ipm_const_list_check(int(h->eng->e.consts.size()), n_par, const_index, &why)) return ipm_refuse(h, rc, who, why);
  return sens_check_solver(h, who, need_state);
}
int sens_check_solver(rpm_ipm* h, const std::string& who, bool need_state) {
  if (h->lbfgs) return ipm_refuse(h, RPM_E_UNSUPPORTED, who, "hessian-approximation = limited-memory: a quasi-Newton Hessian gives no sensitivities");
  if (h->D.scal_on) return ipm_refuse(h, RPM_E_UNSUPPORTED, who, "not with nlp_scaling = 1");
  if (need_state && !h->hold.holds_state())
    return ipm_refuse(h, RPM_E_INVALID, who, "valid after a finished solve, or directly after rpm_ipm_debug_start / rpm_ipm_debug_pass on this solver");
  return RPM_OK;
}

// the source table of the list on the device (kept while the list stays the same), the fixed pattern, the work space
int sens_fixed_room(rpm_ipm* h) {
  rpm_ipm::Sens& s = h->sens;
  const IpmPlan& p = h->plan;
  if (s.fixed) return RPM_OK;
  size_t cap = 0;
  if (int rc = sens_room(h, &s.fixed, &cap, size_t(p.n))) return rc;
  IPM_TRY(h, hipMemcpy(s.fixed, p.fixed.data(), size_t(p.n) * sizeof(int), hipMemcpyHostToDevice));
  return RPM_OK;
}
int sens_upload(rpm_ipm* h, int n_par, const int* var_index, const IpmSensTable& t) {
  rpm_ipm::Sens& s = h->sens;
  const IpmPlan& p = h->plan;
  int rc;
  if ((rc = sens_fixed_room(h))) return rc;
  const std::vector<int> list(var_index, var_index + n_par);
  if (list != s.var_index || !s.table) {
    const size_t G = size_t(t.n_groups());
    std::vector<int> flat;   // ptr (G + 1), par (G), dst (G), src
    flat.reserve(3 * G + 1 + t.src.size());
    flat.insert(flat.end(), t.ptr.begin(), t.ptr.end());
    flat.insert(flat.end(), t.par.begin(), t.par.end());
    flat.insert(flat.end(), t.dst.begin(), t.dst.end());
    flat.insert(flat.end(), t.src.begin(), t.src.end());
    s.var_index.clear();
    if ((rc = sens_room(h, &s.table, &s.table_cap, flat.size()))) return rc;
    IPM_TRY(h, hipMemcpy(s.table, flat.data(), flat.size() * sizeof(int), hipMemcpyHostToDevice));
    s.n_groups = int(G);
    s.var_index = list;
  }
  return sens_room(h, &s.ws, &s.ws_cap, size_t(h->D.B) * size_t(n_par) * size_t(p.Nt_alloc));
}

// What rpm_ipm_sensitivities[_dev] and rpm_ipm_debug_sensitivity_rhs begin with, under the caller's DeviceRestore: every refusal
// (out_ptr: the output that must not be NULL, named out_name), the engine's device bound, table and work space on the device.
int sens_enter(rpm_ipm* h, const std::string& who, int n_par, const int* var_index, const void* out_ptr, const char* out_name) {
  if (!out_ptr) return ipm_refuse(h, RPM_E_INVALID, who, var_index ? std::string(out_name) + " is NULL" : "var_index is NULL");
  IpmSensTable t;
  int rc = sens_check(h, who, n_par, var_index, true, &t);
  if (rc) return rc;
  if ((rc = dev_bind(h->eng->e))) return ipm_eng_fail(h, rc);
  return sens_upload(h, n_par, var_index, t);
}

// steps 1 and 3: g, the Jacobian and the exact Hessian at the state, then the n_par right-hand sides of every instance into the
// (zeroed) work space
int sens_evaluate(rpm_ipm* h, const IpmLoop& L) {   // step 1: what the matrix is assembled from
  Engine& e = L.e;
  IpmDev& D = L.D;
  int rc;
  dev_forget_persistent(e);   // this evaluation writes all of D.jac, the constant block included (as the first one of a solve does)
  ipm_launch_pack_x(D, L.st);
  if ((rc = dev_eval_cons(e, D.xe, D.g, D.jac, 3 | 4 | 16, L.st))) return ipm_eng_fail(h, rc);
  return L.exact_hessian();
}
int sens_evaluate_and_gather(rpm_ipm* h, const IpmLoop& L, int n_par) {
  IpmDev& D = L.D;
  const rpm_ipm::Sens& s = h->sens;
  int rc;
  if ((rc = sens_evaluate(h, L))) return rc;
  IPM_TRY(h, hipMemsetAsync(s.ws, 0, size_t(D.B) * size_t(n_par) * size_t(D.Nt) * sizeof(double), L.st));
  const int G = s.n_groups;
  if (G > 0) {
    const int *ptr = s.table, *par = ptr + G + 1, *dst = par + G, *src = dst + G;
    hipLaunchKernelGGL(ipm_sens_rhs_kernel, dim3(unsigned((G + 255) / 256), unsigned(D.B)), dim3(256), 0, L.st, D, ptr, par, dst, src, G, s.ws);
  }
  return launch_check(h, "ipm_sens_rhs_kernel");
}

// ---- the constants' route: the column table of the plan on the device (once per solver), the fixed pattern, the scratch of one
// constant (grown only) and the work space
int const_upload(rpm_ipm* h, int n_par) {
  rpm_ipm::Sens& s = h->sens;
  const IpmPlan& p = h->plan;
  const Engine& e = h->eng->e;
  const IpmDev& D = h->D;
  int rc;
  if ((rc = sens_fixed_room(h))) return rc;
  if (!s.ctable) {
    const IpmConstTable t = ipm_const_table(p, e.nnz_nl);
    std::vector<int> flat;   // var, var_pos (n_free each), ptr (n_free + 1), ent, ent_row, row_pos (m)
    for (const std::vector<int>* v : {&t.var, &t.var_pos, &t.ptr, &t.ent, &t.ent_row, &t.row_pos}) flat.insert(flat.end(), v->begin(), v->end());
    size_t cap = 0;
    if ((rc = sens_room(h, &s.ctable, &cap, flat.size()))) return rc;
    IPM_TRY(h, hipMemcpy(s.ctable, flat.data(), flat.size() * sizeof(int), hipMemcpyHostToDevice));
    s.c_free = t.n_free();
    s.c_ent = int(t.ent.size());
  }
  const size_t B = size_t(D.B), nconst = e.consts.size(), ev = B * (size_t(D.n) + size_t(D.sg) + 1);
  if ((rc = sens_room(h, &s.cpm, &s.cpm_cap, B * (2 * nconst + 1)))) return rc;
  if ((rc = sens_room(h, &s.eval_p, &s.eval_p_cap, ev)) || (rc = sens_room(h, &s.eval_m, &s.eval_m_cap, ev))) return rc;
  if ((rc = sens_room(h, &s.jac_p, &s.jac_p_cap, B * size_t(D.sv))) || (rc = sens_room(h, &s.jac_m, &s.jac_m_cap, B * size_t(D.sv)))) return rc;
  return sens_room(h, &s.ws, &s.ws_cap, B * size_t(n_par) * size_t(p.Nt_alloc));
}

// What the entry points of the constants' route begin with, under the caller's DeviceRestore (sens_enter for a list of constants).
int const_enter(rpm_ipm* h, const std::string& who, int n_par, const int* const_index, const void* out_ptr, const char* out_name) {
  if (!out_ptr) return ipm_refuse(h, RPM_E_INVALID, who, const_index ? std::string(out_name) + " is NULL" : "const_index is NULL");
  int rc = const_check(h, who, n_par, const_index, true);
  if (rc) return rc;
  if ((rc = dev_bind(h->eng->e))) return ipm_eng_fail(h, rc);
  return const_upload(h, n_par);
}

// The engine's kernels read the constants through Device::kp, which every launcher copies into its launch: pointed at a scratch
// copy while this lives, and put back — the pointer and its stride, by copy — when it goes, on every path.  The engine's own
// constants are never written, and no launch reads a pointer that has been replaced since it was queued.
struct ConstantsAt {
  KParams& kp;
  const double* const keep;
  const int keep_stride;
  explicit ConstantsAt(Engine& e) : kp(e.dev->kp), keep(e.dev->kp.consts), keep_stride(e.dev->kp.consts_stride) {}
  void point(const double* c, int stride) { kp.consts = c; kp.consts_stride = stride; }
  ~ConstantsAt() { point(keep, keep_stride); }
};

// The n_par right-hand sides of every instance into the (zeroed) work space, constant by constant: c+ and c-, the objective
// gradient, g and the Jacobian at each through the engine's batched launchers, then the gather.
int const_evaluate_and_gather(rpm_ipm* h, const IpmLoop& L, int n_par, const int* const_index) {
  Engine& e = L.e;
  IpmDev& D = L.D;
  const rpm_ipm::Sens& s = h->sens;
  hipStream_t st = L.st;
  const size_t B = size_t(D.B), n = size_t(D.n);
  const int nconst = int(e.consts.size());
  double *cp = s.cpm, *cm = cp + B * size_t(nconst), *hbuf = cm + B * size_t(nconst);
  double *grad[2] = {s.eval_p, s.eval_m}, *jac[2] = {s.jac_p, s.jac_m}, *g[2], *obj[2];
  for (int side = 0; side < 2; ++side) {
    g[side] = grad[side] + B * n;
    obj[side] = g[side] + B * size_t(D.sg);
    IPM_TRY(h, hipMemsetAsync(grad[side], 0, B * n * sizeof(double), st));   // (as the engine's own gradient array starts)
  }
  IPM_TRY(h, hipMemsetAsync(s.ws, 0, B * size_t(n_par) * size_t(D.Nt) * sizeof(double), st));
  ipm_launch_pack_x(D, st);
  ConstantsAt at(e);
  const int entries = s.c_free + D.m;
  int rc;
  for (int k = 0; k < n_par; ++k) {
    hipLaunchKernelGGL(ipm_sens_perturb_kernel, dim3(unsigned((nconst + 255) / 256), unsigned(D.B)), dim3(256), 0, st, nconst, at.keep,
                       at.keep_stride, const_index[k], s.const_step, cp, cm, hbuf);
    for (int side = 0; side < 2; ++side) {
      at.point(side ? cm : cp, nconst);
      if ((rc = dev_eval_obj(e, D.xe, obj[side], grad[side], st))) return ipm_eng_fail(h, rc);
      if ((rc = dev_eval_cons(e, D.xe, g[side], jac[side], 3 | 4, st))) return ipm_eng_fail(h, rc);
    }
    hipLaunchKernelGGL(ipm_sens_const_rhs_kernel, dim3(unsigned((entries + 255) / 256), unsigned(D.B)), dim3(256), 0, st, D, s.ctable, s.c_free,
                       s.c_ent, k, grad[0], grad[1], g[0], g[1], jac[0], jac[1], hbuf, s.ws);
  }
  return launch_check(h, "ipm_sens_const_rhs_kernel");
}

// rounds of refinement of a call: the option, or automatically 2 where the engine carries the exact Hessian of a problem with
// static parameters (hessian-approximation = exact-parameters, nq > 0) — the plans whose sensitivities to a fixed parameter the
// plain columns lose — and none elsewhere, where every bit stays what it was
int sens_rounds(const rpm_ipm* h) {
  if (h->sens.refine >= 0) return h->sens.refine;
  const Engine& e = h->eng->e;
  if (!e.hess_parameters) return 0;
  for (const PhaseHost& p : e.ph)
    if (p.nq > 0) return 2;
  return 0;
}

// the row table of ipm_sens_residual_kernel (once per solver) and the two further work spaces
int sens_refine_room(rpm_ipm* h, int n_par) {
  rpm_ipm::Sens& s = h->sens;
  const IpmPlan& p = h->plan;
  const Engine& e = h->eng->e;
  int rc;
  if (!s.rows) {
    const int nv = h->D.nv, n = p.n, m = p.m, NU = nv + m;
    std::vector<std::vector<std::pair<int, int>>> R;
    R.resize(size_t(NU));
    for (int k = 0; k < e.nnz_h; ++k)
      if (p.hes_dst[size_t(k)] >= 0) {
        const int i = e.hes_i[size_t(k)], j = e.hes_j[size_t(k)];
        R[size_t(i)].emplace_back(k, p.pos[size_t(j)]);
        if (i != j) R[size_t(j)].emplace_back(k, p.pos[size_t(i)]);
      }
    for (int k = 0; k < e.nnz_jac; ++k)
      if (p.jac_dst[size_t(k)] >= 0) {
        const int r = nv + e.jac_i[size_t(k)], c = e.jac_j[size_t(k)];
        R[size_t(r)].emplace_back((1 << 28) | k, p.pos[size_t(c)]);
        R[size_t(c)].emplace_back((1 << 28) | k, p.pos[size_t(r)]);
      }
    for (int q = 0; q < int(p.slack_row.size()); ++q) {
      const int r = nv + p.slack_row[size_t(q)], c = n + q;
      R[size_t(r)].emplace_back(2 << 28, p.pos[size_t(c)]);
      R[size_t(c)].emplace_back(2 << 28, p.pos[size_t(r)]);
    }
    for (int i = 0; i < nv; ++i) R[size_t(i)].emplace_back((3 << 28) | i, p.pos[size_t(i)]);
    for (int r = 0; r < m; ++r) R[size_t(nv + r)].emplace_back((4 << 28) | r, p.pos[size_t(nv + r)]);
    std::vector<int> ptr, rpos, code, col;
    ptr.assign(size_t(NU) + 1, 0);
    rpos.assign(size_t(NU), 0);
    for (int u = 0; u < NU; ++u) {
      rpos[size_t(u)] = p.pos[size_t(u)];
      for (const auto& en : R[size_t(u)]) { code.push_back(en.first); col.push_back(en.second); }
      ptr[size_t(u) + 1] = int(code.size());
    }
    std::vector<int> flat;
    flat.insert(flat.end(), ptr.begin(), ptr.end());
    flat.insert(flat.end(), rpos.begin(), rpos.end());
    flat.insert(flat.end(), code.begin(), code.end());
    flat.insert(flat.end(), col.begin(), col.end());
    size_t cap = 0;
    if ((rc = sens_room(h, &s.rows, &cap, flat.size()))) return rc;
    IPM_TRY(h, hipMemcpy(s.rows, flat.data(), flat.size() * sizeof(int), hipMemcpyHostToDevice));
    s.n_rows = NU;
    s.n_ent = int(code.size());
  }
  const size_t len = size_t(h->D.B) * size_t(n_par) * size_t(p.Nt_alloc);
  if ((rc = sens_room(h, &s.rhs0, &s.rhs0_cap, len))) return rc;
  return sens_room(h, &s.res, &s.res_cap, len);
}

SensPars pars_of(int n_par, const int* var_index) {
  SensPars P{};
  P.n_par = n_par;
  for (int k = 0; k < n_par; ++k) P.idx[k] = var_index ? var_index[k] : -1;   // (NULL: columns of constants, no variable their own)
  return P;
}

// The whole of rpm_ipm_sensitivities_dev after its checks — and, `constants`: of rpm_ipm_constant_sensitivities_dev, `var_index`
// then being the list of constants: the perturbed evaluations and their gather come first, the evaluation the matrix is assembled
// from after them, and no fixed variable is a column's own.  The solver's stream is idle on return, the instance records, the
// counters and the statistics of the last solve are what they were.
int sens_run(rpm_ipm* h, int n_par, const int* var_index, double* d_dx, double* d_dlambda, double* delta_w, int* info, void* stream,
             bool constants = false) {
  const IpmLoop L = ipm_loop(h);   // (nlp_scaling is off: sens_check)
  const int rounds = sens_rounds(h);
  IpmDev& D = L.D;
  hipStream_t st = L.st;
  const size_t B = size_t(D.B);
  // ordering contract of rpm_ipm_solve_dev: after what the caller queued on `stream`, drained on return
  IPM_TRY(h, hipEventRecord(h->ev[0], static_cast<hipStream_t>(stream)));
  IPM_TRY(h, hipStreamWaitEvent(st, h->ev[0], 0));
  // the records of the last solve (or of the hooks) are saved; live ones take their place around the factorisation: mode 0,
  // delta_w = 0, asking for a factorisation — and status 5 kept, so that an instance with a non-finite state is left out
  std::vector<IpmInst> saved, live(B, IpmInst{});
  if (int rc = ipm_download_records(h, saved)) return rc;
  for (size_t bi = 0; bi < B; ++bi) {
    live[bi].mu = saved[bi].mu;
    live[bi].refactor = 1;
    if (rounds > 0) live[bi].delta_w = SENS_REFINE_DELTA_W;
    live[bi].status = saved[bi].status == 5 ? 5 : 0;
  }
  const IpmStats keep_stats = h->stats;
  const int keep_cnt[4] = {h->h_cnt[0], h->h_cnt[1], h->h_cnt[2], h->h_cnt[3]};
  h->hold.sensitivities_taken();   // (a direction rpm_ipm_debug_pass(3) left does not survive: D.K and D.rhs are rewritten)
  auto body = [&]() -> int {
    int rc;
    if ((rc = ipm_upload_records(h, live))) return rc;
    if (constants) {
      if ((rc = const_evaluate_and_gather(h, L, n_par, var_index)) || (rc = sens_evaluate(h, L))) return rc;
    } else if ((rc = sens_evaluate_and_gather(h, L, n_par))) return rc;
    if ((rc = L.factor_with_inertia_correction())) return rc;
    IpmDev Ds = D;   // the substitution kernels on the work space: n_par right-hand sides per instance, same factors
    Ds.rhs = h->sens.ws;
    Ds.rhs_mult = n_par;
    const rpm_ipm::Sens& sn = h->sens;
    const size_t len = B * size_t(n_par) * size_t(D.Nt);
    if (rounds > 0) {
      if ((rc = sens_refine_room(h, n_par))) return rc;
      IPM_TRY(h, hipMemcpyAsync(sn.rhs0, sn.ws, len * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    kkt_launch_solve(Ds, 1, st);
    // option "sens_refine": sol += K^-1 (rhs0 - K sol) with the same factors — what a pivot-free LDL^T needs where W + Sigma is
    // nearly singular (a bang-bang plan: no curvature in the states, inactive bounds) and the columns lose digits
    for (int round = 0; round < rounds; ++round) {
      IPM_TRY(h, hipMemsetAsync(sn.res, 0, len * sizeof(double), st));
      hipLaunchKernelGGL(ipm_sens_residual_kernel, dim3(unsigned((sn.n_rows + 255) / 256), unsigned(D.B), unsigned(n_par)), dim3(256), 0, st, D,
                         sn.rows, sn.n_rows, sn.n_ent, sn.rhs0, sn.ws, sn.res, SENS_REFINE_DELTA_W);
      IpmDev Dr = Ds;
      Dr.rhs = sn.res;
      kkt_launch_solve(Dr, 1, st);
      hipLaunchKernelGGL(ipm_sens_correct_kernel, dim3(unsigned((len + 255) / 256)), dim3(256), 0, st, (long long)len, sn.res, sn.ws);
    }
    hipLaunchKernelGGL(ipm_sens_unpack_kernel, dim3(unsigned((D.n + D.m + 255) / 256), unsigned(D.B), unsigned(n_par)), dim3(256), 0, st, D,
                       pars_of(n_par, constants ? nullptr : var_index), h->sens.fixed, h->sens.ws, d_dx, d_dlambda);
    if ((rc = launch_check(h, "sensitivity substitution"))) return rc;
    IPM_TRY(h, hipMemcpyAsync(live.data(), D.inst, B * sizeof(IpmInst), hipMemcpyDeviceToHost, st));
    return RPM_OK;
  };
  const int rc = body();
  // put back, whatever happened (plain runtime calls: a failure's text in h->err stays)
  hipError_t s1 = hipMemcpyAsync(D.inst, saved.data(), B * sizeof(IpmInst), hipMemcpyHostToDevice, st);
  hipError_t s2 = hipMemcpyAsync(D.cnt, keep_cnt, 4 * sizeof(int), hipMemcpyHostToDevice, st);
  hipError_t s3 = hipStreamSynchronize(st);
  for (int i = 0; i < 4; ++i) h->h_cnt[i] = keep_cnt[i];
  h->stats = keep_stats;
  if (rc) return rc;
  IPM_TRY(h, s1);
  IPM_TRY(h, s2);
  IPM_TRY(h, s3);
  for (size_t bi = 0; bi < B; ++bi) {
    const bool ok = live[bi].status == 0;
    if (delta_w) delta_w[bi] = ok ? live[bi].delta_w : std::numeric_limits<double>::quiet_NaN();
    if (info) info[bi] = ok ? (live[bi].delta_w > (rounds > 0 ? SENS_REFINE_DELTA_W : 0.0) ? 1 : 0) : 2;
  }
  return RPM_OK;
}

struct ApplyArrays {
  const double *dx, *dlambda, *delta, *x;
  double* x_out;
  const double* lambda;
  double* lambda_out;
  bool with_lambda() const { return dlambda && lambda && lambda_out; }
};

int apply_check(rpm_ipm* h, const std::string& who, int n_par, const int* var_index, const ApplyArrays& a, bool constants = false) {
  if (int rc = constants ? const_check(h, who, n_par, var_index, false) : sens_check(h, who, n_par, var_index, false, nullptr)) return rc;
  if (!a.dx || !a.delta || !a.x || !a.x_out) return ipm_refuse(h, RPM_E_INVALID, who, "dx, delta, x or x_out is NULL");
  const size_t B = size_t(h->D.B), d8 = sizeof(double), P = size_t(n_par), n = size_t(h->plan.n), m = size_t(h->plan.m);
  const bool lam = a.with_lambda();
  const ByteRange in[5] = {{"dx", a.dx, B * P * n * d8}, {"delta", a.delta, B * P * d8}, {"x", a.x, B * n * d8},
                           {"dlambda", lam ? a.dlambda : nullptr, B * P * m * d8}, {"lambda", lam ? a.lambda : nullptr, B * m * d8}};
  const ByteRange out[2] = {{"x_out", a.x_out, B * n * d8}, {"lambda_out", lam ? a.lambda_out : nullptr, B * m * d8}};
  Engine& e = h->eng->e;
  return ipm_eng_fail(h, step_overlap(e, who + ": ", out, 2, in, 5));   // every output against every input and the other output
}

int apply_launch(rpm_ipm* h, int n_par, const ApplyArrays& a, hipStream_t stream) {
  const IpmDev& D = h->D;
  const bool lam = a.with_lambda() && D.m > 0;
  const int xblocks = (D.n + 511) / 512, lblocks = lam ? (D.m + 511) / 512 : 0;   // two entries per thread
  hipLaunchKernelGGL(ipm_sens_apply_kernel, dim3(unsigned(xblocks + lblocks), unsigned(D.B)), dim3(256), 0, stream, D.n, D.m, n_par, xblocks,
                     a.dx, a.dlambda, a.delta, a.x, a.x_out, a.lambda, a.lambda_out);
  return launch_check(h, "ipm_sens_apply_kernel");
}

int apply_host_form(rpm_ipm* h, int n_par, const ApplyArrays& a);   // (below the entry points)

}  // namespace

extern "C" {

int rpm_ipm_initial_state_variables(rpm_ipm* h, int phase, int* var_index) {
  if (!h) return RPM_E_INVALID;
  const Engine& e = h->eng->e;
  const std::string who = "rpm_ipm_initial_state_variables";
  if (phase < 0 || phase >= e.P) return ipm_refuse(h, RPM_E_INVALID, who, "phase " + std::to_string(phase) + " is out of range");
  if (!var_index) return ipm_refuse(h, RPM_E_INVALID, who, "var_index is NULL");
  const PhaseHost& p = e.ph[size_t(phase)];
  for (int j = 0; j < p.nx; ++j) var_index[j] = p.var0 + j * (p.N + 1);
  return RPM_OK;
}

int rpm_ipm_parameter_variables(rpm_ipm* h, int phase, int* var_index) {
  if (!h) return RPM_E_INVALID;
  const Engine& e = h->eng->e;
  const std::string who = "rpm_ipm_parameter_variables";
  if (phase < 0 || phase >= e.P) return ipm_refuse(h, RPM_E_INVALID, who, "phase " + std::to_string(phase) + " is out of range");
  if (!var_index) return ipm_refuse(h, RPM_E_INVALID, who, "var_index is NULL");
  const PhaseHost& p = e.ph[size_t(phase)];
  for (int j = 0; j < p.nq; ++j) var_index[j] = p.var0 + p.nx * (p.N + 1) + p.nu * p.N + 2 + j;
  return RPM_OK;
}

int rpm_ipm_sensitivities_dev(rpm_ipm* h, int n_par, const int* var_index, double* d_dx, double* d_dlambda, double* delta_w, int* info,
                              void* stream) {
  if (!h) return RPM_E_INVALID;
  DeviceRestore restore;
  if (int rc = sens_enter(h, "rpm_ipm_sensitivities", n_par, var_index, d_dx, "dx")) return rc;
  return sens_run(h, n_par, var_index, d_dx, d_dlambda, delta_w, info, stream);
}

int rpm_ipm_sensitivities(rpm_ipm* h, int n_par, const int* var_index, double* dx, double* dlambda, double* delta_w, int* info) {
  if (!h) return RPM_E_INVALID;
  DeviceRestore restore;
  int rc = sens_enter(h, "rpm_ipm_sensitivities", n_par, var_index, dx, "dx");
  if (rc) return rc;
  const size_t B = size_t(h->D.B), Pn = size_t(n_par) * h->plan.n, Pm = size_t(n_par) * h->plan.m;
  if ((rc = sens_room(h, &h->sens.block, &h->sens.block_cap, B * (Pn + Pm)))) return rc;
  double *d_dx = h->sens.block, *d_dl = dlambda ? d_dx + B * Pn : nullptr;
  if ((rc = sens_run(h, n_par, var_index, d_dx, d_dl, delta_w, info, dev_stream(h->eng->e)))) return rc;
  IPM_TRY(h, hipMemcpy(dx, d_dx, B * Pn * sizeof(double), hipMemcpyDeviceToHost));
  if (dlambda && Pm) IPM_TRY(h, hipMemcpy(dlambda, d_dl, B * Pm * sizeof(double), hipMemcpyDeviceToHost));
  return RPM_OK;
}

int rpm_ipm_debug_sensitivity_rhs(rpm_ipm* h, int n_par, const int* var_index, double* rhs) {
  if (!h) return RPM_E_INVALID;
  DeviceRestore restore;
  int rc = sens_enter(h, "rpm_ipm_debug_sensitivity_rhs", n_par, var_index, rhs, "rhs");
  if (rc) return rc;
  if ((rc = sens_evaluate_and_gather(h, ipm_loop(h), n_par))) return rc;
  return ipm_download_unknown_order(h, h->sens.ws, size_t(n_par), rhs);
}

int rpm_ipm_apply_sensitivities_dev(rpm_ipm* h, int n_par, const int* var_index, const double* d_dx, const double* d_dlambda,
                                    const double* d_delta, const double* d_x, double* d_x_out, const double* d_lambda, double* d_lambda_out,
                                    void* stream) {
  if (!h) return RPM_E_INVALID;
  const ApplyArrays a{d_dx, d_dlambda, d_delta, d_x, d_x_out, d_lambda, d_lambda_out};
  if (int rc = apply_check(h, "rpm_ipm_apply_sensitivities_dev", n_par, var_index, a)) return rc;
  return apply_launch(h, n_par, a, static_cast<hipStream_t>(stream));
}

int rpm_ipm_apply_sensitivities(rpm_ipm* h, int n_par, const int* var_index, const double* dx, const double* dlambda, const double* delta,
                                const double* x, double* x_out, const double* lambda, double* lambda_out) {
  if (!h) return RPM_E_INVALID;
  const ApplyArrays a{dx, dlambda, delta, x, x_out, lambda, lambda_out};
  if (int rc = apply_check(h, "rpm_ipm_apply_sensitivities", n_par, var_index, a)) return rc;
  return apply_host_form(h, n_par, a);
}

int rpm_ipm_constant_sensitivities_dev(rpm_ipm* h, int n_par, const int* const_index, double* d_dx, double* d_dlambda, double* delta_w,
                                       int* info, void* stream) {
  if (!h) return RPM_E_INVALID;
  DeviceRestore restore;
  if (int rc = const_enter(h, "rpm_ipm_constant_sensitivities", n_par, const_index, d_dx, "dx")) return rc;
  return sens_run(h, n_par, const_index, d_dx, d_dlambda, delta_w, info, stream, true);
}

int rpm_ipm_constant_sensitivities(rpm_ipm* h, int n_par, const int* const_index, double* dx, double* dlambda, double* delta_w, int* info) {
  if (!h) return RPM_E_INVALID;
  DeviceRestore restore;
  int rc = const_enter(h, "rpm_ipm_constant_sensitivities", n_par, const_index, dx, "dx");
  if (rc) return rc;
  const size_t B = size_t(h->D.B), Pn = size_t(n_par) * h->plan.n, Pm = size_t(n_par) * h->plan.m;
  if ((rc = sens_room(h, &h->sens.block, &h->sens.block_cap, B * (Pn + Pm)))) return rc;
  double *d_dx = h->sens.block, *d_dl = dlambda ? d_dx + B * Pn : nullptr;
  if ((rc = sens_run(h, n_par, const_index, d_dx, d_dl, delta_w, info, dev_stream(h->eng->e), true))) return rc;
  IPM_TRY(h, hipMemcpy(dx, d_dx, B * Pn * sizeof(double), hipMemcpyDeviceToHost));
  if (dlambda && Pm) IPM_TRY(h, hipMemcpy(dlambda, d_dl, B * Pm * sizeof(double), hipMemcpyDeviceToHost));
  return RPM_OK;
}

int rpm_ipm_debug_constant_sensitivity_rhs(rpm_ipm* h, int n_par, const int* const_index, double* rhs) {
  if (!h) return RPM_E_INVALID;
  DeviceRestore restore;
  int rc = const_enter(h, "rpm_ipm_debug_constant_sensitivity_rhs", n_par, const_index, rhs, "rhs");
  if (rc) return rc;
  if ((rc = const_evaluate_and_gather(h, ipm_loop(h), n_par, const_index))) return rc;
  return ipm_download_unknown_order(h, h->sens.ws, size_t(n_par), rhs);
}

int rpm_ipm_apply_constant_sensitivities_dev(rpm_ipm* h, int n_par, const int* const_index, const double* d_dx, const double* d_dlambda,
                                             const double* d_delta, const double* d_x, double* d_x_out, const double* d_lambda,
                                             double* d_lambda_out, void* stream) {
  if (!h) return RPM_E_INVALID;
  const ApplyArrays a{d_dx, d_dlambda, d_delta, d_x, d_x_out, d_lambda, d_lambda_out};
  if (int rc = apply_check(h, "rpm_ipm_apply_constant_sensitivities_dev", n_par, const_index, a, true)) return rc;
  return apply_launch(h, n_par, a, static_cast<hipStream_t>(stream));
}

int rpm_ipm_apply_constant_sensitivities(rpm_ipm* h, int n_par, const int* const_index, const double* dx, const double* dlambda,
                                         const double* delta, const double* x, double* x_out, const double* lambda, double* lambda_out) {
  if (!h) return RPM_E_INVALID;
  const ApplyArrays a{dx, dlambda, delta, x, x_out, lambda, lambda_out};
  if (int rc = apply_check(h, "rpm_ipm_apply_constant_sensitivities", n_par, const_index, a, true)) return rc;
  return apply_host_form(h, n_par, a);
}

}  // extern "C"

namespace {

// the host-pointer form of the predictor after its checks: arrays up, one launch, results down
int apply_host_form(rpm_ipm* h, int n_par, const ApplyArrays& a) {
  const double *dx = a.dx, *dlambda = a.dlambda, *delta = a.delta, *x = a.x, *lambda = a.lambda;
  double *x_out = a.x_out, *lambda_out = a.lambda_out;
  int rc;
  DeviceRestore restore;
  Engine& e = h->eng->e;
  if ((rc = dev_bind(e))) return ipm_eng_fail(h, rc);
  hipStream_t st = static_cast<hipStream_t>(dev_stream(e));
  const bool lam = a.with_lambda();
  const size_t B = size_t(h->D.B), P = size_t(n_par), n = size_t(h->plan.n), m = size_t(h->plan.m), d8 = sizeof(double);
  // the block: dx, delta, x, x_out, then dlambda, lambda, lambda_out (every piece an even number of doubles from the start,
  // padded, so that each keeps the base's 16-byte alignment)
  auto even = [](size_t c) { return (c + 1) & ~size_t(1); };
  const size_t o_delta = even(B * P * n), o_x = o_delta + even(B * P), o_xo = o_x + even(B * n), o_dl = o_xo + even(B * n);
  const size_t o_l = o_dl + even(B * P * m), o_lo = o_l + even(B * m), total = o_lo + even(B * m);
  if ((rc = sens_room(h, &h->sens.block, &h->sens.block_cap, total))) return rc;
  double* b = h->sens.block;
  IPM_TRY(h, hipMemcpyAsync(b, dx, B * P * n * d8, hipMemcpyHostToDevice, st));
  IPM_TRY(h, hipMemcpyAsync(b + o_delta, delta, B * P * d8, hipMemcpyHostToDevice, st));
  IPM_TRY(h, hipMemcpyAsync(b + o_x, x, B * n * d8, hipMemcpyHostToDevice, st));
  if (lam && m) {
    IPM_TRY(h, hipMemcpyAsync(b + o_dl, dlambda, B * P * m * d8, hipMemcpyHostToDevice, st));
    IPM_TRY(h, hipMemcpyAsync(b + o_l, lambda, B * m * d8, hipMemcpyHostToDevice, st));
  }
  const ApplyArrays dv{b, lam ? b + o_dl : nullptr, b + o_delta, b + o_x, b + o_xo, lam ? b + o_l : nullptr, lam ? b + o_lo : nullptr};
  if ((rc = apply_launch(h, n_par, dv, st))) return rc;
  IPM_TRY(h, hipMemcpyAsync(x_out, b + o_xo, B * n * d8, hipMemcpyDeviceToHost, st));
  if (lam && m) IPM_TRY(h, hipMemcpyAsync(lambda_out, b + o_lo, B * m * d8, hipMemcpyDeviceToHost, st));
  IPM_TRY(h, hipStreamSynchronize(st));
  return RPM_OK;
}

}  // namespace
