// rpm_kkt_assemble.hip — row f-2: the KKT matrix of every running instance and its right-hand side (the values: rpm_kkt_slots.hpp;
// the factorisation: rpm_kkt_factor.hip, whose register-resident kernel builds the level-1 blocks itself).
//   K = [[W + Sigma + dw I, A^T], [A, -dc I]] (13) and its right-hand side      ipm_fill_kernel (ipm_zero_kernel + ipm_assemble_kernel)
//     (restoration: [[zeta D_R^2 + Sigma, A^T], [A, -(Sigma_p^-1 + Sigma_n^-1)]]; least-squares multipliers: [[I, A^T], [A, -dc I]])
#include <algorithm>

#include "rpm_device_internal.hpp"
#include "rpm_ipm_device.hpp"
#include "rpm_kkt_slots.hpp"

namespace rpm {

__global__ void ipm_zero_kernel(IpmDev D) {
  const int bi = blockIdx.y;
  const IpmInst& S = D.inst[bi];
  if (S.status != 0 || !S.refactor) return;
  double2* K = reinterpret_cast<double2*>(D.K + size_t(bi) * D.kstride);
  const long long n2 = D.kstride / 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long long)gridDim.x * blockDim.x)
    K[i] = make_double2(0.0, 0.0);
}
// by source, onto the storage ipm_zero_kernel zeroed (the values: SlotValue's, restated by source)
__global__ void ipm_assemble_kernel(IpmDev D) {
  const int bi = blockIdx.y;
  const IpmInst& S = D.inst[bi];
  if (S.status != 0 || !S.refactor) return;
  double* K = D.K + size_t(bi) * D.kstride;
  const double *v = D.v + size_t(bi) * D.nv, *vl = D.vl + size_t(bi) * D.nv, *vu = D.vu + size_t(bi) * D.nv;
  const double *zL = D.zL + size_t(bi) * D.nv, *zU = D.zU + size_t(bi) * D.nv;
  const int stride = gridDim.x * blockDim.x, t0 = blockIdx.x * blockDim.x + threadIdx.x;
  // mode 0: (13).  mode 2 (restoration, p and n eliminated): [[zeta D_R^2 + Sigma_v, A^T], [A, -(Sigma_p^-1 + Sigma_n^-1)]], no
  // Hessian (Gauss-Newton model).  mode 3 (least-squares multipliers): [[I, A^T], [A, -delta_c]].
  const int mode = S.mode;
  if (mode == 0 && !D.lb_on)   // duplicates of a slot (I-part / E-part of the reference's COO) are summed in COO order: bit-reproducible.  The
    for (int i = t0; i < D.n_hg; i += stride) {   // slot may also take the diagonal term below: two atomic adds onto zero commute
      double acc = 0.0;
      for (int j = D.hg_ptr[i]; j < D.hg_ptr[i + 1]; ++j) acc += D.hess[size_t(bi) * D.nnz_h + D.hg_src[j]];
      unsafeAtomicAdd(&K[D.hg_dst[i]], acc);
    }
  for (int k = t0; k < D.nnz_jac; k += stride)
    if (D.jac_dst[k] >= 0) K[D.jac_dst[k]] = D.jac[size_t(bi) * D.sv + k];
  for (int s = t0; s < D.ns; s += stride) K[D.slk_dst[s]] = -1.0;
  double* rhs = D.rhs + size_t(bi) * D.Nt;
  const double mu = mode == 2 ? S.mu_r : S.mu;
  for (int i = t0; i < D.nv; i += stride) {
    const double l = vl[i], u = vu[i];
    double diag = 1.0, r = 0.0;
    if (l != u) {
      if (mode == 3) {
        diag = 1.0 + S.delta_w;
        r = (i < D.n ? D.grad[size_t(bi) * D.n + i] : 0.0) - zL[i] + zU[i];
      } else {
        diag = S.delta_w;
        if (mode == 0 && D.lb_on && i < D.n) diag += D.lb_small[size_t(bi) * IPM_LB_SMALL];   // sigma I of the limited-memory Hessian
        r = D.glag[size_t(bi) * D.nv + i];
        if (mode == 2) {
          const double w2 = S.zeta * D.dr2[size_t(bi) * D.nv + i];
          diag += w2;
          r += w2 * (v[i] - D.vR[size_t(bi) * D.nv + i]);
        }
        const double cap = D.o.sigma_cap > 0 ? D.o.sigma_cap : 1e300;
        if (l > -IPM_INF) { const double d = v[i] - l; diag += fmin(zL[i] / d, cap); r -= mu / d; }
        if (u < IPM_INF) { const double d = u - v[i]; diag += fmin(zU[i] / d, cap); r += mu / d; }
      }
    }
    unsafeAtomicAdd(&K[D.diag_dst[i]], diag);
    rhs[D.pos[i]] = -r;
  }
  for (int r = t0; r < D.m; r += stride) {
    double k22 = -D.o.delta_c, rr = 0.0;
    if (mode == 0) rr = -D.c[size_t(bi) * D.m + r];
    else if (mode == 2) {
      const size_t q = size_t(bi) * D.m + r;
      const double pp = D.pp[q], nn = D.nn[q], sp = D.zp[q] / pp, sn = D.zn[q] / nn, lam = D.lam[q];
      const double rp = D.o.resto_rho - lam - mu / pp, rn = D.o.resto_rho + lam - mu / nn;
      k22 = -(1.0 / sp + 1.0 / sn);
      rr = -(D.c[q] - pp + nn) - rp / sp + rn / sn;
    }
    K[D.diag_dst[D.nv + r]] = k22;
    rhs[D.pos[D.nv + r]] = rr;
  }
}

// ipm_zero_kernel + ipm_assemble_kernel in one pass over the storage, by destination: a workgroup builds a chunk of the
// storage in LDS (zeros, then the chunk's structural slots, as_* tables in ascending order) and writes it out in full lines,
// so every line of the storage leaves the chip once per refactorisation instead of being zeroed, fetched again for a
// scattered read-modify-write and written a second time (1024-instance quadrotor sweep: 0.59 + 0.72 ms per iteration for the
// two kernels).  Chunks inside a level-1 block that kkt_factor_dense_kernel assembles itself (IpmDev::df_on) are left out.
__global__ __launch_bounds__(256) void ipm_fill_kernel(IpmDev D) {
  __shared__ double buf[IPM_FILL_CHUNK];
  const int bi = blockIdx.y;
  const IpmInst& S = D.inst[bi];
  if (S.status != 0 || !S.refactor) return;
  double* K = D.K + size_t(bi) * D.kstride;
  const int tid = threadIdx.x;
  const SlotValue value(D, bi);
  const bool some = D.df_on && D.l1_dense_lds && D.as_live;     // only the chunks not inside a level-1 block (kkt_level1_fused)
  const int n_here = some ? D.as_nlive : D.as_nchunk;
  for (int ci = blockIdx.x; ci < n_here; ci += gridDim.x) {
    const int c = some ? D.as_live[ci] : ci;
    const long long lo = (long long)c * IPM_FILL_CHUNK, hi = min(lo + IPM_FILL_CHUNK, D.kstride);
    const int e0 = D.as_ptr[c], e1 = D.as_ptr[c + 1];
    // this thread's first slot: its loads are under way while the chunk is zeroed
    const int ef = e0 + tid;
    double val_f = 0.0;
    int off_f = -1;
    if (ef < e1) { off_f = int(D.as_dst[ef] - lo); val_f = value(D.as_ki, D.as_hg, ef); }
    double2* b2 = reinterpret_cast<double2*>(buf);
    for (int i = tid; i < IPM_FILL_CHUNK / 2; i += 256) b2[i] = make_double2(0.0, 0.0);
    __syncthreads();
    if (off_f >= 0) buf[off_f] = val_f;
    for (int e = ef + 256; e < e1; e += 256) buf[D.as_dst[e] - lo] = value(D.as_ki, D.as_hg, e);
    __syncthreads();
    const int len = int(hi - lo);
    if ((reinterpret_cast<size_t>(K + lo) & 15) == 0) {
      double2* K2 = reinterpret_cast<double2*>(K + lo);
      typedef double d2v __attribute__((ext_vector_type(2)));   // streaming stores: the storage is next read by the factorisation, from HBM either way
      for (int i = tid; i < (len >> 1); i += 256) __builtin_nontemporal_store(d2v{b2[i].x, b2[i].y}, reinterpret_cast<d2v*>(K2 + i));
      if ((len & 1) && tid == 0) K[hi - 1] = buf[len - 1];
    } else {
      for (int i = tid; i < len; i += 256) K[lo + i] = buf[i];
    }
    __syncthreads();   // buf is free for the next chunk
  }
}

void ipm_launch_assemble(const IpmDev& D, int nnz_max, hipStream_t st) {
  if (D.as_nchunk > 0) {
    const int chunks = kkt_level1_fused(D) ? D.as_nlive : D.as_nchunk;
    hipLaunchKernelGGL(ipm_fill_kernel, dim3(unsigned(std::max(1, std::min(chunks, 65535))), unsigned(D.B)), dim3(256), 0, st, D);
    return;
  }
  const int assemble_blocks = std::max(1, std::min(D.B <= 32 ? 2048 : 64, (nnz_max + 255) / 256));   // a few large instances: the whole chip
  const int zero_blocks = int(std::max<long long>(1, std::min<long long>(256, D.kstride / 2 / 256 + 1)));
  hipLaunchKernelGGL(ipm_zero_kernel, dim3(unsigned(zero_blocks), unsigned(D.B)), dim3(256), 0, st, D);
  hipLaunchKernelGGL(ipm_assemble_kernel, dim3(unsigned(assemble_blocks), unsigned(D.B)), dim3(256), 0, st, D);
}

}  // namespace rpm
