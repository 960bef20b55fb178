// rpm_kkt_solve.hip — row f-2: substitution with the factors of rpm_kkt_factor.hip (in the right-hand side rpm_kkt_assemble.hip wrote), the right-hand-side glue of the nested
// dissection and the inertia verdict of Algorithm IC      kkt_solve_kernel, kkt_gather_seq_kernel, kkt_vec_kernel, ipm_inertia_kernel
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "rpm_device_internal.hpp"
#include "rpm_ipm_device.hpp"

namespace rpm {

// block column J0 of the band + border storage (rpm_kkt_factor.hip): its end and its panel rows (in-band first, then the border)
__device__ inline void block_range(const KktGeom& G, int J0, int* J1, int* nrb, int* nr) {
  if (J0 < G.Nb) {
    *J1 = min(J0 + IPM_W, G.Nb);
    const int last = min(*J1 - 1 + G.b, G.Nb - 1);
    *nrb = max(last - *J1 + 1, 0);
    *nr = *nrb + G.nb;
  } else {
    *J1 = min(J0 + IPM_W, G.Nt);
    *nrb = 0;
    *nr = G.Nt - *J1;
  }
}
__device__ inline int panel_row(const KktGeom& G, int J0, int J1, int nrb, int q) {
  return J0 >= G.Nb ? J1 + q : (q < nrb ? J1 + q : G.Nb + (q - nrb));
}

// L y = r, then x = L^-T D^-1 y, in place in rhs: one workgroup per instance, IPM_W columns per step.  The diagonal
// blocks hold L11^-1, so a step's own 16 unknowns are 16 parallel dot products.  The right-hand side lives in LDS when it
// fits (RL); the diagonal block and each thread's panel row of the NEXT step are fetched while the current one is worked.
template <bool RL, int PF = 1>
__global__ __launch_bounds__(256) void kkt_solve_kernel(const double* Kall, long long kstride, const KktSub* subs, int sub0, int n_here,
                                                        const IpmInst* inst, double* rhs_all, long long rhs_stride, int check_status,
                                                        int phase, int kmod) {
  // phase 0: forward and backward over all blocks; nested dissection level 1: phase 1 = forward over the band blocks only
  // (the border work space receives -L_border y, this interval's contribution to the separator system's right-hand side),
  // phase 2 = backward over the band blocks only (the work space then holds the separator / border solution)
  constexpr int W = IPM_W;
  // with the right-hand side in LDS the barriers order LDS traffic only: __syncthreads() would also wait for the factor entries
  // fetched for the NEXT step (s_waitcnt vmcnt(0)), a trip to the L2 / HBM on the chain of every step
#define SOLVE_BARRIER() do { if (RL) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); else __syncthreads(); } while (0)
  // several right-hand sides per instance (IpmDev::rhs_mult): right-hand side bi belongs to instance bi % kmod
  const int bi = blockIdx.x / n_here, bk = bi % kmod, t = threadIdx.x, nt = blockDim.x;
  if (check_status && (inst[bk].status != 0 || (check_status == 2 && !inst[bk].soc_req))) return;
  const KktSub sub = subs[sub0 + int(blockIdx.x) % n_here];
  const KktGeom G = sub.g;
  const double* K = Kall + size_t(bk) * kstride + sub.koff;
  double* rg = rhs_all + size_t(bi) * rhs_stride + sub.roff;
  extern __shared__ double rsh[];
  double* r = RL ? rsh : rg;
  __shared__ double Dg[W * (W + 1)], ys[W], zs[W], red[4][W];     // Dg: d on the diagonal, L11^-1 below it
  const int di = t / W, dj = t % W;
  const int nbb = (G.Nb + W - 1) / W, ncb = (G.nb + W - 1) / W, nblk = nbb + ncb;
  if (RL) {
    for (int i = t; i < G.Nt; i += nt) rsh[i] = rg[i];
    SOLVE_BARRIER();
  }
  struct Blk { int J0, J1, nrb, nr, w; };
  auto blk_of = [&](int blk) {
    Blk B;
    B.J0 = blk < nbb ? blk * W : G.Nb + (blk - nbb) * W;
    block_range(G, B.J0, &B.J1, &B.nrb, &B.nr);
    B.w = B.J1 - B.J0;
    return B;
  };
  // this thread's share of a step: one entry of the diagonal block and the 16 factor entries of panel row q = t
  auto fetch = [&](int blk, double& dg, double (&l)[W]) {
    if (blk < 0 || blk >= nblk) return;
    const Blk B = blk_of(blk);
    dg = (di < B.w && dj <= di) ? K[G.at(B.J0 + di, B.J0 + dj)] : 0.0;
    const int row = t < B.nr ? panel_row(G, B.J0, B.J1, B.nrb, t) : -1;
    // one 64-bit address (row, column J0) and a 32-bit step per column (a G.at() per entry is a 64-bit multiply each: most of a step's instructions)
    const bool brd = row >= G.Nb;
    const int kstep = brd ? G.CS : G.CS - 1;
    const double* kp = K + (size_t(B.J0) * G.CS + (brd ? G.b + 1 + row - G.Nb : max(row - B.J0, 0)));
#pragma unroll
    for (int c = 0; c < W; ++c)
      l[c] = (row >= 0 && c < B.w && (brd || row - (B.J0 + c) <= G.b)) ? kp[c * kstep] : 0.0;
  };
  // PF = 2 (launches of few workgroups, where occupancy is no concern): two steps' shares on their way — a step is a few hundred cycles of
  // LDS work between barriers, a trip to the L2 / HBM takes longer
  double dg0, l0[W], dg1, l1[W];
  const int fwd_end = phase == 1 ? nbb : (phase == 2 ? 0 : nblk), bwd_begin = phase == 2 ? nbb : (phase == 1 ? 0 : nblk);
  auto forward_step = [&](int blk, double& dg, double (&l)[W]) {
    const Blk B = blk_of(blk);
    if (di < W && dj <= di) Dg[di * (W + 1) + dj] = dg;
    if (t < W) zs[t] = t < B.w ? r[B.J0 + t] : 0.0;
    SOLVE_BARRIER();
    if (t < W) {                // y = L11^-1 r: 16 lanes, one row each
      double y = zs[t];
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (k < t && t < B.w) y = __builtin_fma(Dg[t * (W + 1) + k], zs[k], y);
      ys[t] = y;
      if (t < B.w) r[B.J0 + t] = y;
    }
    SOLVE_BARRIER();
    for (int q = t; q < B.nr; q += nt) {
      const int row = panel_row(G, B.J0, B.J1, B.nrb, q);
      double acc = 0.0;
#pragma unroll
      for (int c = 0; c < W; ++c) {
        const double lv = q == t ? l[c] : ((c < B.w && (row >= G.Nb || row - (B.J0 + c) <= G.b)) ? K[G.at(row, B.J0 + c)] : 0.0);
        acc = __builtin_fma(lv, ys[c], acc);
      }
      r[row] -= acc;
    }
    fetch(blk + PF, dg, l);     // in flight across the barrier and the next PF - 1 steps
    SOLVE_BARRIER();
  };
  if (fwd_end > 0) { fetch(0, dg0, l0); if (PF == 2) fetch(1 < fwd_end ? 1 : -1, dg1, l1); }
  for (int blk = 0; blk < fwd_end; blk += PF) {
    forward_step(blk, dg0, l0);
    if (PF == 2 && blk + 1 < fwd_end) forward_step(blk + 1, dg1, l1);
  }
  auto backward_step = [&](int blk, double& dg, double (&l)[W]) {
    const Blk B = blk_of(blk);
    if (di < W && dj <= di) Dg[di * (W + 1) + dj] = dg;
    double p[W];
#pragma unroll
    for (int c = 0; c < W; ++c) p[c] = 0.0;
    for (int q = t; q < B.nr; q += nt) {
      const int row = panel_row(G, B.J0, B.J1, B.nrb, q);
      const double xr = r[row];
#pragma unroll
      for (int c = 0; c < W; ++c) {
        const double lv = q == t ? l[c] : ((c < B.w && (row >= G.Nb || row - (B.J0 + c) <= G.b)) ? K[G.at(row, B.J0 + c)] : 0.0);
        p[c] = __builtin_fma(lv, xr, p[c]);
      }
    }
    fetch(blk - PF, dg, l);     // in flight across the reduction, the diagonal solve and the next PF - 1 steps
    {   // the 16 sums over the wave, each by the same tree as `for (o = 32; o; o >>= 1) v += shfl_down(v, o)` (lane l + lane l + o:
        // the same pairs, a + b for b + a at most), but the columns are dealt out while the lanes fold: 8 + 4 + 2 + 1 + 1 + 1
        // exchanges instead of 16 x 6 — column c's sum ends in lane 4 c.  (The LDS pipe, which carries the exchanges, bounded the
        // backward pass when 12 right-hand sides of the limited-memory update run side by side.)
      const int ln = t & 63;
      double q8[8], q4[4], q2[2], u;
      const bool h32 = ln & 32, h16 = ln & 16, h8 = ln & 8, h4 = ln & 4;
#pragma unroll
      for (int i = 0; i < 8; ++i) q8[i] = (h32 ? p[i + 8] : p[i]) + __shfl_xor(h32 ? p[i] : p[i + 8], 32);
#pragma unroll
      for (int i = 0; i < 4; ++i) q4[i] = (h16 ? q8[i + 4] : q8[i]) + __shfl_xor(h16 ? q8[i] : q8[i + 4], 16);
#pragma unroll
      for (int i = 0; i < 2; ++i) q2[i] = (h8 ? q4[i + 2] : q4[i]) + __shfl_xor(h8 ? q4[i] : q4[i + 2], 8);
      u = (h4 ? q2[1] : q2[0]) + __shfl_xor(h4 ? q2[0] : q2[1], 4);
      u += __shfl_xor(u, 2);
      u += __shfl_xor(u, 1);
      if ((ln & 3) == 0) red[t >> 6][ln >> 2] = u;
    }
    SOLVE_BARRIER();
    if (t < W) zs[t] = t < B.w ? r[B.J0 + t] / Dg[t * (W + 1) + t] - (red[0][t] + red[1][t] + red[2][t] + red[3][t]) : 0.0;
    SOLVE_BARRIER();
    if (t < B.w) {              // x = L11^-T z
      double x = zs[t];
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (k > t && k < B.w) x = __builtin_fma(Dg[k * (W + 1) + t], zs[k], x);
      r[B.J0 + t] = x;
    }
    SOLVE_BARRIER();
  };
  if (bwd_begin > 0) { fetch(bwd_begin - 1, dg0, l0); if (PF == 2) fetch(bwd_begin - 2, dg1, l1); }
  for (int blk = bwd_begin - 1; blk >= 0; blk -= PF) {
    backward_step(blk, dg0, l0);
    if (PF == 2 && blk - 1 >= 0) backward_step(blk - 1, dg1, l1);
  }
  if (RL)
    for (int i = t; i < G.Nt; i += nt) rg[i] = rsh[i];
#undef SOLVE_BARRIER
}

// ------------------------------------------------------------------------------------------------ inertia correction
// Algorithm IC: the factorisation is accepted when D has exactly nv positive entries (and no zero / NaN pivot)
__global__ __launch_bounds__(256) void ipm_inertia_kernel(IpmDev D) {   // a wave per instance: its lanes add up the sub-problems' pivot counts
  const int bi = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (bi >= D.B) return;
  IpmInst& S = D.inst[bi];
  if (S.status != 0 || !S.refactor) return;
  const IpmOpts& o = D.o;
  int np = 0, nn = 0, nz = 0;
  for (int s2 = lane; s2 < D.n_sub; s2 += 64) {   // pivot signs of all the sub-problems of this instance (one without dissection)
    const int* q = D.piv + (size_t(bi) * D.n_sub + s2) * 3;
    np += q[0]; nn += q[1]; nz += q[2];
  }
  for (int w = 32; w; w >>= 1) { np += __shfl_xor(np, w); nn += __shfl_xor(nn, w); nz += __shfl_xor(nz, w); }
  if (lane != 0) return;
  S.npos = np; S.nneg = nn; S.nbad = nz;
  if (S.npos == D.nv && S.nbad == 0) {
    S.refactor = 0;
    if (S.delta_w > 0) S.delta_w_last = S.delta_w;
    if (S.mode == 0) S.ic_hot = S.delta_w > 0;
    return;
  }
  if (S.delta_w == 0.0) S.delta_w = S.delta_w_last == 0.0 ? o.delta_w_first : fmax(o.delta_w_min, o.kw_dec * S.delta_w_last);
  else S.delta_w *= S.delta_w_last == 0.0 ? o.kw_inc_first : o.kw_inc;
  if (S.delta_w > o.delta_w_max) { S.status = 4; return; }
  atomicAdd(&D.cnt[1], 1);
}

// v[dst[i]] += v[src[ptr[i]]] + v[src[ptr[i] + 1]] + ... in list order, a WAVE per destination: 64 sources are fetched at a time, then
// every lane adds them up in order through shuffles (lane 0 stores).  The right-hand-side gather of the nested dissection: the
// global border's rows collect one term from every interval — 256 on the metric problem, 88 us as 256 dependent loads of one
// thread, a few microseconds this way — with the sums' order, and so their bits, unchanged.
__global__ __launch_bounds__(256) void kkt_gather_seq_kernel(double* vall, long long vstride, const int* __restrict__ ptr, const int* __restrict__ src,
                                                             const int* __restrict__ dst, int n, const IpmInst* inst, int check_status, int kmod) {
  const int bi = blockIdx.y, bk = bi % kmod;
  if (check_status && (inst[bk].status != 0 || (check_status == 2 && !inst[bk].soc_req))) return;
  double* v = vall + size_t(bi) * vstride;
  const int lane = threadIdx.x & 63, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
  for (int i = wave; i < n; i += n_waves) {
    const int j0 = ptr[i], j1 = ptr[i + 1];
    double acc = v[dst[i]];
    for (int j = j0; j < j1; j += 64) {
      const double mine = j + lane < j1 ? v[src[j + lane]] : 0.0;
      const int m = min(64, j1 - j);
      for (int k = 0; k < m; ++k) acc += __shfl(mine, k, 64);
    }
    if (lane == 0) v[dst[i]] = acc;
  }
}
// mode 0: v[pos[i]] = 0;  mode 1: v[dst[i]] = v[src[i]]
__global__ void kkt_vec_kernel(double* vall, long long vstride, const int* __restrict__ dst, const int* __restrict__ src, int n, int mode,
                               const IpmInst* inst, int check_status, int kmod) {
  const int bi = blockIdx.y, bk = bi % kmod;
  if (check_status && (inst[bk].status != 0 || (check_status == 2 && !inst[bk].soc_req) || (check_status == 3 && !inst[bk].refactor))) return;
  double* v = vall + size_t(bi) * vstride;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) v[dst[i]] = mode ? v[src[i]] : 0.0;
}
void kkt_launch_vec(const IpmDev& D, unsigned n_rhs, const int* dst, const int* src, int n, int mode, int check_status, hipStream_t st) {
  if (!n) return;
  const unsigned blocks = unsigned(std::max(1, std::min(256, (n + 255) / 256)));
  hipLaunchKernelGGL(kkt_vec_kernel, dim3(blocks, n_rhs), dim3(256), 0, st, D.rhs, (long long)D.Nt, dst, src, n, mode, D.inst,
                     check_status, D.B);
}

static void launch_solve_subs(const IpmDev& D, int sub0, int n_here, int phase, int check_status, hipStream_t st) {
  const dim3 grid(unsigned(D.B) * unsigned(D.rhs_mult > 1 ? D.rhs_mult : 1) * unsigned(n_here));
  if (size_t(D.max_sub_nt) * sizeof(double) <= 48 * 1024 && grid.x <= 512)        // few workgroups: two steps' factor entries in flight
    hipLaunchKernelGGL((kkt_solve_kernel<true, 2>), grid, dim3(256), size_t(D.max_sub_nt) * sizeof(double), st, D.K, D.kstride, D.subs, sub0, n_here,
                       D.inst, D.rhs, (long long)D.Nt, check_status, phase, D.B);
  else if (size_t(D.max_sub_nt) * sizeof(double) <= 48 * 1024)
    hipLaunchKernelGGL(kkt_solve_kernel<true>, grid, dim3(256), size_t(D.max_sub_nt) * sizeof(double), st, D.K, D.kstride, D.subs, sub0, n_here,
                       D.inst, D.rhs, (long long)D.Nt, check_status, phase, D.B);
  else
    hipLaunchKernelGGL(kkt_solve_kernel<false>, grid, dim3(256), 0, st, D.K, D.kstride, D.subs, sub0, n_here, D.inst, D.rhs, (long long)D.Nt,
                       check_status, phase, D.B);
}
void kkt_launch_solve(const IpmDev& D, int check_status, hipStream_t st, int forward_done) {
  const unsigned VB = unsigned(D.B) * unsigned(D.rhs_mult > 1 ? D.rhs_mult : 1);   // right-hand sides in D.rhs (rhs_mult per instance)
  if (D.n_l1 == 0) {
    launch_solve_subs(D, 0, 1, 0, check_status, st);
    return;
  }
  auto vec = [&](const int* dst, const int* src, int n, int mode) { kkt_launch_vec(D, VB, dst, src, n, mode, check_status, st); };
  auto gather = [&](const int* ptr, const int* src, const int* dst, int n) {
    if (!n) return;
    const unsigned blocks = unsigned(std::max(1, std::min(4096, (n + 3) / 4)));           // a wave per destination
    hipLaunchKernelGGL(kkt_gather_seq_kernel, dim3(blocks, VB), dim3(256), 0, st, D.rhs, (long long)D.Nt, ptr, src, dst, n, D.inst, check_status, D.B);
  };
  if (!(forward_done && kkt_level1_fused(D))) {                                        // (else kkt_factor_dense_kernel did both for this right-hand side)
    vec(D.gap_pos, nullptr, D.n_gap, 0);                                               // border work spaces start at zero
    launch_solve_subs(D, 0, D.n_l1, 1, check_status, st);                              // forward, every interval
  }
  gather(D.rg_ptr, D.rg_src, D.rg_dst, D.n_rg);
  if (D.n_l2) {
    launch_solve_subs(D, D.n_l1, D.n_l2, 1, check_status, st);                         // forward, every group
    gather(D.rg2_ptr, D.rg2_src, D.rg2_dst, D.n_rg2);
  }
  launch_solve_subs(D, D.n_l1 + D.n_l2, 1, 0, check_status, st);                       // last level
  if (D.n_l2) {
    vec(D.rs2_dst, D.rs2_src, D.n_rs2, 1);                                             // its solution into the groups' work spaces
    launch_solve_subs(D, D.n_l1, D.n_l2, 2, check_status, st);                         // backward, every group
  }
  vec(D.rs_dst, D.rs_src, D.n_rs, 1);                                                  // separator / border values into the intervals' work spaces
  launch_solve_subs(D, 0, D.n_l1, 2, check_status, st);                                // backward, every interval
}
void ipm_launch_inertia(const IpmDev& D, hipStream_t st) {
  hipLaunchKernelGGL(ipm_inertia_kernel, dim3(unsigned((D.B + 3) / 4)), dim3(256), 0, st, D);
}

}  // namespace rpm
