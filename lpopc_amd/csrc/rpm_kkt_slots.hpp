// rpm_kkt_slots.hpp — device only: the value of every structural slot of the KKT matrix and of the right-hand side entry that
// goes with a diagonal slot, by destination: for ipm_fill_kernel (rpm_kkt_assemble.hip) and the assembling prologue of
// kkt_factor_dense_kernel (rpm_kkt_factor.hip).  The rule is written out in two more places, whose results must agree with these
// bit for bit — a change to it is made in all three: ipm_assemble_kernel (rpm_kkt_assemble.hip; by source, every term), and the
// Hessian duplicate sum of the dense kernel's prologue.  A fourth reader restates the mode-0 matrix entries (no right-hand side):
// ipm_sens_residual_kernel (rpm_ipm_sens.hip), whose refined columns tests/test_gpu_param_solver.py holds against a dense numpy solve
// of the matrix built from independent sources — a rule that drifts apart there moves the refined columns.  (Sharing one copy through member functions changes the code generated
// for ipm_fill_kernel and the dense factor kernels, which are tuned as they stand.)
#pragma once
#include "rpm_ipm_device.hpp"

namespace rpm {

// The value of a structural slot of instance bi's KKT matrix in its present mode (ki / hg coded as IpmDev::as_ki / as_hg) and, for
// a diagonal slot, the right-hand side entry that goes with it (written on the way).  Same values as ipm_assemble_kernel's, bit
// for bit: a slot that took two atomic adds onto zero there (Hessian sum, diagonal term) gets their sum.
struct SlotValue {
  const IpmDev& D;
  int bi, mode;
  double mu, delta_w, zeta;
  const double *v, *vl, *vu, *zL, *zU;
  double* rhs;
  __device__ SlotValue(const IpmDev& D_, int bi_) : D(D_), bi(bi_) {
    const IpmInst& S = D.inst[bi];
    mode = S.mode;
    mu = mode == 2 ? S.mu_r : S.mu;
    delta_w = S.delta_w;
    zeta = S.zeta;
    v = D.v + size_t(bi) * D.nv; vl = D.vl + size_t(bi) * D.nv; vu = D.vu + size_t(bi) * D.nv;
    zL = D.zL + size_t(bi) * D.nv; zU = D.zU + size_t(bi) * D.nv;
    rhs = D.rhs + size_t(bi) * D.Nt;
  }
  // entry e of the tables ki_tab / hg_tab (the Hessian slot that shares a diagonal is looked up only for a diagonal)
  __device__ double operator()(const int* ki_tab, const int* hg_tab, int e) const {
    const int ki = ki_tab[e], kind = ki >> 28, idx = ki & 0x0fffffff;
    if (kind == 1) return D.jac[size_t(bi) * D.sv + idx];
    if (kind == 2) return -1.0;
    if (kind == 4) {   // diagonal of constraint row idx
      double k22 = -D.o.delta_c, rr = 0.0;
      if (mode == 0) rr = -D.c[size_t(bi) * D.m + idx];
      else if (mode == 2) {
        const size_t q = size_t(bi) * D.m + idx;
        const double pp = D.pp[q], nn = D.nn[q], sp = D.zp[q] / pp, sn = D.zn[q] / nn, lam = D.lam[q];
        const double rp = D.o.resto_rho - lam - mu / pp, rn = D.o.resto_rho + lam - mu / nn;
        k22 = -(1.0 / sp + 1.0 / sn);
        rr = -(D.c[q] - pp + nn) - rp / sp + rn / sn;
      }
      rhs[D.pos[D.nv + idx]] = rr;
      return k22;
    }
    // 0: a Hessian slot; 3: the diagonal of variable idx (with the Hessian slot that shares it)
    const int hgi = kind == 0 ? idx : hg_tab[e];
    double acc = 0.0;
    if (mode == 0 && hgi >= 0 && !D.lb_on)
      for (int j = D.hg_ptr[hgi]; j < D.hg_ptr[hgi + 1]; ++j) acc += D.hess[size_t(bi) * D.nnz_h + D.hg_src[j]];
    if (kind == 0) return 0.0 + acc;   // as the add onto the zeroed slot gave it (a sum of -0.0 becomes +0.0)
    const int i = idx;
    const double l = vl[i], u = vu[i];
    double diag = 1.0, r = 0.0;
    if (l != u) {
      if (mode == 3) {
        diag = 1.0 + delta_w;
        r = (i < D.n ? D.grad[size_t(bi) * D.n + i] : 0.0) - zL[i] + zU[i];
      } else {
        diag = delta_w;
        if (mode == 0 && D.lb_on && i < D.n) diag += D.lb_small[size_t(bi) * IPM_LB_SMALL];   // sigma I of the limited-memory Hessian
        r = D.glag[size_t(bi) * D.nv + i];
        if (mode == 2) {
          const double w2 = zeta * D.dr2[size_t(bi) * D.nv + i];
          diag += w2;
          r += w2 * (v[i] - D.vR[size_t(bi) * D.nv + i]);
        }
        const double cap = D.o.sigma_cap > 0 ? D.o.sigma_cap : 1e300;
        if (l > -IPM_INF) { const double d = v[i] - l; diag += fmin(zL[i] / d, cap); r -= mu / d; }
        if (u < IPM_INF) { const double d = u - v[i]; diag += fmin(zU[i] / d, cap); r += mu / d; }
      }
    }
    rhs[D.pos[i]] = -r;
    // the two-kernel path adds the two terms onto zero, in either order: acc + diag, exactly
    return (mode == 0 && hgi >= 0) ? acc + diag : diag;
  }
};

}  // namespace rpm
