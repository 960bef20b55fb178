// rpm_kkt_factor.hip — row f-2: the factorisation of the KKT matrix of every running instance (the iteration around it:
// rpm_ipm_step_kernels.hip; the matrix and its right-hand side: rpm_kkt_assemble.hip, rpm_kkt_slots.hpp; substitution: rpm_kkt_solve.hip).
//   LDL^T without pivoting (one band, or nested dissection over the mesh intervals and, on long meshes, over groups of their
//     separators), pivot signs for Algorithm IC                                  kkt_factor_kernel, kkt_factor_dense_kernel, kkt_gather_add_kernel
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "rpm_device_internal.hpp"
#include "rpm_ipm_device.hpp"
#include "rpm_kkt_slots.hpp"

namespace rpm {

// ------------------------------------------------------------------------------------------------ lane helpers
// value of `v` in lane `lane` of the wave (lane uniform; a constant after unrolling): two v_readlane_b32 instead of the
// ds_bpermute pair of __shfl
__device__ inline double readlane_d(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
// value of `v` in the lane whose number is byte_addr / 4 (any lane per lane): a ds_bpermute pair
__device__ inline double bperm_d(int byte_addr, double v) {
  const int lo = __builtin_amdgcn_ds_bpermute(byte_addr, __double2loint(v)), hi = __builtin_amdgcn_ds_bpermute(byte_addr, __double2hiint(v));
  return __hiloint2double(hi, lo);
}
// value of `v` in lane K of the reader's own row of 16 lanes (DPP row_newbcast)
template <int K>
__device__ inline double row_bcast_d(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0x150 + K, 0xf, 0xf, false), hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0x150 + K, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
// One step of the 16 x 16 LDL^T + inverse of kkt_factor_dense_kernel's diagonal wave with the block's COLUMNS dealt to the four
// rows of 16 lanes: lane (q, r) = 16 q + r keeps, of matrix row r, the columns 4 g + q (R[g]: the block, V[g]: L11^-1 so far).
// Step K: the pivot column sits in group K & 3 — every lane fetches its own row's entry of it (the multiplier's numerator) and
// the entries of the rows that are its columns (ds_bpermute, 10 a step), row K of the inverse comes by row_newbcast, and a lane
// is left with 4 or 5 of the 16 products of a step.  Every entry sees the same operations in the same order as with a whole
// row per lane (a wave-uniform v_readlane per operand, 34 a step, 16 dependent products).
template <int K>
struct DiagStep {
  static __device__ __forceinline__ void run(double (&R)[4], double (&V)[4], int q, int r, int a_own, const int (&a_col)[4]) {
    constexpr int QK = K & 3, GK = K >> 2;
    const double dk = readlane_d(R[GK], QK * 16 + K);
    const double ar = bperm_d(a_own + QK * 64, R[GK]);
    double aj[4] = {0.0, 0.0, 0.0, 0.0}, mk[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (4 * g + 3 > K) aj[g] = bperm_d(a_col[g] + QK * 64, R[GK]);     // a(4 g + q, K) before scaling
      if (4 * g <= K) mk[g] = row_bcast_d<K>(V[g]);                       // row K of the inverse so far
    }
    // (a reciprocal estimate with two Newton steps instead of the division: 90.5 -> 86.6 us of diagonal-block time per
    // interval block, not worth leaving the left-looking kernel's arithmetic)
    const double lik = r > K ? ar / dk : 0.0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (4 * g > K) R[g] = __builtin_fma(-lik, aj[g], R[g]);             // columns right of the pivot
      else if (4 * g + 3 > K) { const double u = __builtin_fma(-lik, aj[g], R[g]); R[g] = q > K - 4 * g ? u : R[g]; }
      if (4 * g + 3 <= K) V[g] = __builtin_fma(-lik, mk[g], V[g]);        // columns up to the pivot
      else if (4 * g <= K) { const double u = __builtin_fma(-lik, mk[g], V[g]); V[g] = q <= K - 4 * g ? u : V[g]; }
    }
    if (q == QK && r > K) R[GK] = lik;
    if constexpr (K + 1 < IPM_W) DiagStep<K + 1>::run(R, V, q, r, a_own, a_col);
  }
};
typedef double d4 __attribute__((ext_vector_type(4)));
// The signs of the pivots a thread has seen, for Algorithm IC's inertia; a zero, NaN or overflowed pivot is bad.  The
// counts go in and out by value, which keeps them in registers under the branches as the factor kernels were tuned with.
struct PivotCount { int npos, nneg, nbad; };
__device__ __forceinline__ PivotCount count_pivot(double dk, PivotCount n) {
  if (dk > 0) ++n.npos; else if (dk < 0) ++n.nneg; else ++n.nbad;
  if (!(fabs(dk) < 1e300)) ++n.nbad;
  return n;
}
// every thread's counts into the workgroup's cnt[3] (LDS, zeroed at the start); cnt is complete on return
__device__ __forceinline__ void add_pivot_counts(int* cnt, PivotCount n) {
  if (n.npos) atomicAdd(&cnt[0], n.npos);
  if (n.nneg) atomicAdd(&cnt[1], n.nneg);
  if (n.nbad) atomicAdd(&cnt[2], n.nbad);
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------ band + border LDL^T
// Storage of one instance: column j holds rows j .. j+b of the band (slot i-j) and the nb border rows (slot b+1+i-Nb).
// IPM_W columns at a time: the diagonal block is factored in LDS, each panel row is solved by the thread that owns it.
// No pivoting: with dw large enough and dc > 0 the matrix is symmetric quasi-definite, whose LDL^T exists for every
// ordering (Vanderbei 1995); the signs of D give the inertia Algorithm IC asks for.

// Left-looking over the band: block column J (IPM_W = 16 columns) gathers the contributions of the b columns before it,
//     A(rows, J..J+15)^T  -=  T^T (16 x k) . L(rows, k)^T (k x 16 rows),      T[k][c] = d_k L(J+c, k),
// as v_mfma_f64_16x16x4_f64 products: one 16-row tile of the matrix per accumulator, the tiles of a block column dealt to
// the 4 waves, T staged in LDS (one conflict-free 8-byte read per lane and 4 columns), L streamed from HBM exactly where
// it is non-zero (a tile starts at its first in-band column).  Every factor entry is read ~b/16 times and written once
// (the right-looking form re-writes the whole (b + nb)^2 window per block column).  The panel solve is a second
// matrix product, Y^T = L11^-1 A^T, with the accumulators fed back as the B operand.  The border x border corner lives
// in LDS, is updated right-looking and factored there.  Operand maps (cdna_hip_programming.md §3): A: lane l holds
// A[l&15][l>>4], B: B[l>>4][l&15], C/D: row (l>>4) + 4 reg, column l&15.
#ifndef IPM_LB
#define IPM_LB 2   // waves per SIMD the 4-tile factorisation is compiled for (3: 168 VGPRs, 52 of them spilled since the pivots moved to v_readlane)
#endif
// MT 16-row tiles per wave, NW waves: <4,4> block columns of up to 256 rows, 3 workgroups per CU; <6,4> 384 rows, 2 per CU (at 3 it
// spills 91 VGPRs); <8,4> 512 rows; <3,8> 384 rows over 8 waves — for a few large instances (the metric problem: 268 workgroups
// on 256 CUs), where a second wave per SIMD halves every wave's share of a block column
template <int MT, int NW = 4>
__global__ __launch_bounds__(64 * NW, NW == 8 ? (MT == 2 ? 4 : 1) : (MT == 4 ? IPM_LB : (MT == 6 ? 2 : 1))) void kkt_factor_kernel(double* Kall, long long kstride, const KktSub* subs, int sub0,
                                                                               int n_here, int n_sub, IpmInst* inst, int* piv, int partial) {
  // workgroup = (instance, sub-problem sub0 + s).  partial 1: nested dissection level 1 — eliminate the band part only and
  // leave the Schur complement of the border x border corner, unfactored, in the corner's storage.  partial 2: the corner only
  // (what kkt_factor_dense_kernel left of a last level whose band part it eliminated; its pivot counts are added to).
  constexpr int W = IPM_W;
  const int bi = blockIdx.x / n_here, sidx = sub0 + int(blockIdx.x) % n_here, t = threadIdx.x, nt = blockDim.x;
  const IpmInst& S = inst[bi];
  if (S.status != 0 || !S.refactor) return;
  const KktSub sub = subs[sidx];
  const KktGeom G = sub.g;
  double* K = Kall + size_t(bi) * kstride + sub.koff;
  extern __shared__ double lds[];
  double* T = lds;                              // (b + 24) x W
  double* Dg = T + size_t(G.b + 24) * W;        // W x (W + 1)
  double* Mi = Dg + W * (W + 1);                // W x W: L11^-1, row-major
  double* invd = Mi + W * W;                    // W
  double* BL = invd + W;                        // nb x W: L of the border rows in the current block column
  double* BY = BL + size_t(G.nb) * W;           // nb x W: L D
  double* C = BY + size_t(G.nb) * W;            // nb (nb + 1) / 2: the corner's lower triangle, packed by rows
  __shared__ int cnt[3];
  if (t < 3) cnt[t] = 0;
  PivotCount pc = {0, 0, 0};
  const int nb = G.nb;
  const int wv = t >> 6, lr = t & 15, lq = (t & 63) >> 4;
#ifdef IPM_TIMING
#ifndef IPM_TIMING_SUB
#define IPM_TIMING_SUB (-1)   // which sub-problem's workgroup reports its phase clocks (-1: the last level's)
#endif
  long long tc[6] = {0, 0, 0, 0, 0, 0}, t_prev = wall_clock64();
#define IPM_TICK(i) do { __syncthreads(); const long long _n = wall_clock64(); tc[i] += _n - t_prev; t_prev = _n; } while (0)
#else
#define IPM_TICK(i)
#endif
  auto ct = [](int r, int c) { return r * (r + 1) / 2 + c; };   // the corner's lower triangle, packed by rows (c <= r)
  for (int idx = t; idx < nb * nb; idx += nt) {
    const int r = idx / nb, c = idx % nb;
    if (r >= c) C[ct(r, c)] = K[G.at(G.Nb + r, G.Nb + c)];
  }
  // corner -= L_border D L_border^T of a block column: the 16 x 16 tiles of its lower triangle dealt to the waves w0, w0 + 1, ..
  // (nw of them), four matrix products each (the scalar form — 16 FMAs per entry fed by LDS reads 128 bytes apart, a 16-way bank
  // conflict — was 73 % of a separator group's factorisation and 23 % of an interval's).  It only needs the column's border rows of
  // L and L D (BL, BY), which stay in LDS until the NEXT panel is solved: so block column J's update runs on the waves that are
  // idle while wave 0 factors the diagonal block of J + 1 (it was a phase of its own, 15 % of an interval block of the metric problem).
  auto corner_update = [&](int w0, int nw) {
    const int nbt = (nb + 15) >> 4, ntl = nbt * (nbt + 1) / 2;
    for (int tl = wv - w0; tl < ntl; tl += nw) {
      int ti = 0;
      while ((ti + 1) * (ti + 2) / 2 <= tl) ++ti;
      const int tj = tl - ti * (ti + 1) / 2, ra = ti * 16 + lr, cb = tj * 16 + lr;
      d4 cacc;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int rr = ti * 16 + lq + 4 * g;
        cacc[g] = (rr < nb && cb <= rr) ? C[ct(rr, cb)] : 0.0;
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const double a = ra < nb ? -BL[ra * W + 4 * g + lq] : 0.0, bq = cb < nb ? BY[cb * W + 4 * g + lq] : 0.0;
        cacc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bq, cacc, 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int rr = ti * 16 + lq + 4 * g;
        if (rr < nb && cb <= rr) C[ct(rr, cb)] = cacc[g];
      }
    }
  };
  for (int J0 = partial == 2 ? G.Nb : 0; J0 < G.Nb;) {
    const int J1 = min(J0 + W, G.Nb), w = J1 - J0;
    const int kbase = max(J0 - G.b, 0), nk = J0 - kbase, ngrp = (nk + 3) >> 2;
    const int nrb = max(min(J1 - 1 + G.b, G.Nb - 1) - J1 + 1, 0), rows = w + nrb + nb, ntile = (rows + 15) >> 4;
#pragma unroll 4
    for (int idx = t; idx < (ngrp + 4) * 4 * W; idx += nt) {      // zero rows behind the last column: the k-loop reads up to 3 groups past it
      const int kk = idx / W, c = idx % W, k = kbase + kk, j = J0 + c;
      T[idx] = (kk < nk && c < w && j - k <= G.b) ? K[G.at(j, k)] * K[G.at(k, k)] : 0.0;
    }
    __syncthreads();
    IPM_TICK(0);
    d4 acc[MT];
    const double* lp[MT];       // &L(r, kbase) of this lane's row in tile i: in-band rows walk columns with stride CS - 1, border rows CS
    int lstep[MT], kfirst[MT], gfirst[MT], rrow[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int q0 = (wv + NW * i) * 16, q = q0 + lr;
      const bool valid = q < rows;
      const int r = q < w ? J0 + q : (q - w < nrb ? J1 + (q - w) : G.Nb + (q - w - nrb));
      const bool border = r >= G.Nb;
      rrow[i] = valid ? r : -1;
      kfirst[i] = valid ? (border ? 0 : max(r - G.b - kbase, 0)) : (1 << 30);
      lp[i] = K + (valid ? G.at(r, kbase) : 0);
      lstep[i] = border ? G.CS : G.CS - 1;
      // the tile's first group of 4 columns with anything stored: from its first row when the whole tile is inside the band
      const int r_first = q0 < w ? J0 + q0 : J1 + (q0 - w);
      gfirst[i] = q0 >= rows ? (1 << 30) : ((q0 + 15 >= w + nrb) ? 0 : (max(r_first - G.b - kbase, 0) >> 2));
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = lq + 4 * g;
        acc[i][g] = (valid && c < w && J0 + c <= r && (border || r - (J0 + c) <= G.b)) ? K[G.at(r, J0 + c)] : 0.0;
      }
    }
    {
      // KD column groups of L in flight per tile while the previous KD are multiplied (4 where the registers allow: the loop
      // waits on loads that come from the L2 / Infinity Cache, 2 waves per SIMD hide little of that)
      constexpr int KD = MT <= 4 ? 4 : 2;
      auto ld = [&](int i, int kg) -> double {
        const int kk = 4 * kg + lq;
        return (kg >= gfirst[i] && kk >= kfirst[i] && kk < nk) ? lp[i][size_t(kk) * lstep[i]] : 0.0;
      };
      double bq[KD][MT];
#pragma unroll
      for (int j = 0; j < KD; ++j)
#pragma unroll
        for (int i = 0; i < MT; ++i) bq[j][i] = ld(i, j);
      for (int kg = 0; kg < ngrp; kg += KD) {
        double a[KD], nq[KD][MT];
#pragma unroll
        for (int j = 0; j < KD; ++j) a[j] = -T[(4 * (kg + j) + lq) * W + lr];
#pragma unroll
        for (int j = 0; j < KD; ++j)
#pragma unroll
          for (int i = 0; i < MT; ++i) nq[j][i] = ld(i, kg + KD + j);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          if (kg + KD - 1 < gfirst[i]) continue;
#pragma unroll
          for (int j = 0; j < KD; ++j) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j], bq[j][i], acc[i], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < KD; ++j)
#pragma unroll
          for (int i = 0; i < MT; ++i) bq[j][i] = nq[j][i];
      }
    }
    IPM_TICK(1);
    if (wv != 0) {
      if (J0 > 0 && nb > 0) corner_update(1, NW - 1);    // the previous block column's, while wave 0 is busy below
    } else {                    // tile 0 holds the diagonal block (rows q < w): its LDL^T and the inverse of L11 by this wave
      // the accumulator tile is DiagStep's layout already: lane (lq, lr) holds columns lq + 4 g of row lr
      double R[4], V[4];
      int a_col[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j = 4 * g + lq;
        R[g] = (lr < w && j <= lr) ? acc[0][g] : (j == lr ? 1.0 : 0.0);
        V[g] = j == lr ? 1.0 : 0.0;
        a_col[g] = j << 2;
      }
      DiagStep<0>::run(R, V, lq, lr, lr << 2, a_col);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j = 4 * g + lq;
        if (lr < w && j <= lr) Dg[lr * (W + 1) + j] = R[g];
        Mi[lr * W + j] = V[g];
        if (j == lr) invd[lr] = lr < w ? 1.0 / R[g] : 0.0;
      }
    }
    __syncthreads();
    IPM_TICK(2);
    // panel rows: Y^T = L11^-1 A^T (4 products with the accumulator as B operand), L21^T = D^-1 Y^T
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      if ((wv + NW * i) * 16 >= rows) continue;
      d4 y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int g = 0; g < 4; ++g) y = __builtin_amdgcn_mfma_f64_16x16x4f64(Mi[lr * W + 4 * g + lq], acc[i][g], y, 0, 0, 0);
      const int q = (wv + NW * i) * 16 + lr, r = rrow[i];
      if (r < 0 || q < w) continue;
      const bool border = r >= G.Nb;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = lq + 4 * g;
        const double l = y[g] * invd[c];
        if (c < w && (border || r - (J0 + c) <= G.b)) K[G.at(r, J0 + c)] = l;
        if (border) { BL[(r - G.Nb) * W + c] = l; BY[(r - G.Nb) * W + c] = c < w ? y[g] : 0.0; }
      }
    }
    {                           // the diagonal block is stored as d on the diagonal and L11^-1 below it (what the solves use)
      const int di = t / W, dj = t % W;
      if (di < w && dj <= di) K[G.at(J0 + di, J0 + dj)] = di == dj ? Dg[di * (W + 1) + dj] : Mi[di * W + dj];
    }
    if (t < w) pc = count_pivot(Dg[t * (W + 1) + t], pc);
    __syncthreads();
    IPM_TICK(3);
    IPM_TICK(4);
    J0 = J1;
  }
  if (G.Nb > 0 && nb > 0 && partial != 2) {          // the last block column's corner update
    corner_update(0, NW);
    __syncthreads();
  }
  if (partial == 2) __syncthreads();   // (the corner is in LDS)
  if (partial == 1) {                                            // level 1 of the nested dissection: hand the corner over as it is
    for (int idx = t; idx < nb * nb; idx += nt) {
      const int r = idx / nb, c = idx % nb;
      if (r >= c) K[G.at(G.Nb + r, G.Nb + c)] = C[ct(r, c)];
    }
    add_pivot_counts(cnt, pc);
    if (t < 3) piv[(size_t(bi) * n_sub + sidx) * 3 + t] = cnt[t];
#ifdef IPM_TIMING
    if (t == 0 && sidx == IPM_TIMING_SUB)
      for (int i = 0; i < 6; ++i) inst[bi].dbg[i] = tc[i];
#endif
    return;
  }
  for (int k = 0; k < nb; ++k) {                            // the corner, unblocked, in LDS
    __syncthreads();
    const double dk = C[ct(k, k)];
    for (int idx = t; idx < nb * nb; idx += nt) {
      const int r = idx / nb, c = idx % nb;
      if (r > k && c > k && c <= r) C[ct(r, c)] -= C[ct(r, k)] / dk * C[ct(c, k)];
    }
    __syncthreads();
    for (int r = k + 1 + t; r < nb; r += nt) C[ct(r, k)] /= dk;
  }
  __syncthreads();
  for (int idx = t; idx < nb; idx += nt) {                  // the corner's 16 x 16 diagonal sub-blocks: L -> L^-1, column by column
    const int c0 = idx / W * W, cj = idx, w2 = min(W, nb - c0);
    double x[W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
      double v = c0 + i == cj ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < i; ++k)
        if (i < w2 && c0 + k >= cj) v = __builtin_fma(-C[ct(c0 + i, c0 + k)], x[k], v);
      x[i] = c0 + i < cj ? 0.0 : v;
    }
    // in place: the 16 columns of a sub-block belong to 16 consecutive lanes of one wave, which has read all of them
    // (the loop above) before any lane writes its column back
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < W; ++i)
      if (i < w2 && c0 + i > cj) C[ct(c0 + i, cj)] = x[i];
  }
  __syncthreads();
  for (int idx = t; idx < nb * nb; idx += nt) {
    const int r = idx / nb, c = idx % nb;
    if (r >= c) K[G.at(G.Nb + r, G.Nb + c)] = C[ct(r, c)];
    if (r == c) pc = count_pivot(C[ct(r, r)], pc);
  }
  add_pivot_counts(cnt, pc);
  IPM_TICK(5);
  if (t < 3) piv[(size_t(bi) * n_sub + sidx) * 3 + t] = (partial == 2 ? piv[(size_t(bi) * n_sub + sidx) * 3 + t] : 0) + cnt[t];
#ifdef IPM_TIMING
  if (t == 0 && (IPM_TIMING_SUB < 0 || sidx == IPM_TIMING_SUB))
    for (int i = 0; i < 6; ++i) inst[bi].dbg[i] = tc[i];
#endif
}

// Level 1 of the nested dissection when an interval block is small and (nearly) dense — the quadrotor sweep's are of order 252
// with a half bandwidth of 200: the whole lower triangle lives in the REGISTERS of one workgroup as 16 x 16 accumulator tiles
// (tile (I, K), K <= I, transposed like kkt_factor_kernel's: lane l holds columns (l >> 4) + 4 reg of block K for row l & 15 of
// block I), dealt round robin to 7 waves (at most IPM_DENSE_SLOTS = 22 tiles each: 17 block rows), and the elimination runs
// right-looking: block column J's diagonal tile is factored by the eighth wave, which holds no tiles (the same register LDL^T
// with the inverse alongside; its 100-odd registers would not fit beside 22 accumulator tiles),
// the tiles below it are solved against it (4 matrix products each) and leave L and L D in LDS, every tile to the right takes
// its rank-16 update from there (4 products).  Nothing is read twice: the left-looking kernel streams the 488 KB of such a
// block ~12 times from the L2 / Infinity Cache, a 16-column step every 25 us.  Same products in the same order, so the factors
// are the left-looking kernel's bit for bit.  Partial elimination only (the band part; the border x border corner is handed
// on as the Schur complement).
// EARLY: blocks of more than IPM_DENSE_ROWS block rows (the steps for their first block columns cost the plain kernel 15 %).
// CORNER: a last level — with partial = 0 the corner's block columns are eliminated too, their panels solved by SUBSTITUTION with
// L11 (a lane's 16 steps, each a broadcast among the four lanes of a row) and a true division by d, as kkt_factor_kernel's unblocked
// corner does, instead of the product with the explicit L11^-1: the global border holds the pivots of -delta_c and the
// multipliers of the linkages, and with the inverse there 3 of 28 perturbed starts of the metric problem ended in a failed line search
template <bool EARLY, bool CORNER>
__global__ __launch_bounds__(512, 1) void kkt_factor_dense_kernel(double* Kall, long long kstride, const KktSub* subs, int sub0, int n_here,
                                                                  int n_sub, IpmInst* inst, int* piv, IpmDev D, int assemble, int forward,
                                                                  int partial) {
  constexpr int W = IPM_W, NWV = IPM_DENSE_TILE_WAVES, MAXS = IPM_DENSE_SLOTS;
  // the barriers of this kernel order LDS traffic only: __syncthreads() would also wait for the stores of L into the storage
  // (s_waitcnt vmcnt(0)), a trip to the L2 on the critical path of every block column
#define IPM_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
  const int bi = blockIdx.x / n_here, sidx = sub0 + int(blockIdx.x) % n_here, t = threadIdx.x;
  const IpmInst& S = inst[bi];
  if (S.status != 0 || !S.refactor) return;
  const KktSub sub = subs[sidx];
  const KktGeom G = sub.g;
  double* K = Kall + size_t(bi) * kstride + sub.koff;
  const int nbb = (G.Nb + W - 1) / W, nbr = (G.nb + W - 1) / W, NTB = nbb + nbr;
  // the trailing R block rows live in registers; the E block columns before them ("early") go through the storage
  const int E = EARLY ? ipm_dense_early(NTB) : 0, R = NTB - E, ntl = R * (R + 1) / 2;
  const int nbe = (CORNER && !partial) ? NTB : nbb;    // block columns to eliminate: the band part, or (the last level) the corner's as well
  extern __shared__ double lds[];
  double* Dg = lds;                       // 2 x W x (W + 1): the diagonal tile of block column J in copy J & 1 (the next one is handed over
                                          // while the eighth wave still stores the current one)
  constexpr int DGN = W * (W + 1);
  double* Mi = Dg + 2 * DGN;              // W x 18: L11^-1, row-major (rows padded like the panel's, see below)
  double* invd = Mi + W * IPM_DENSE_LDS_ROW;   // W
  // rows of 18 doubles: the 16 lanes that read one column of 16 successive rows then hit 16 different pairs of banks (at 16
  // doubles per row they share two, and the matrix products starve: 18 us per block column instead of 3)
  constexpr int BS = IPM_DENSE_LDS_ROW;
  double* dv = invd + W;                   // W: the pivots d (what the storage holds on the diagonal)
  double* BL = dv + W;                     // NTB x 16 x BS: L of the current block column, by block row
  double* BY = BL + size_t(NTB) * W * BS;  // the same for L D
  double* rsh = BY + size_t(NTB) * W * BS; // forward: this block's right-hand side, NTB x 16
  double* ysh = rsh + size_t(NTB) * W;     // forward: y of the current block column
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, lr = t & 15, lq = (t & 63) >> 4;
  // hand_over: block column J's panel rows of block row J + 1 are in LDS (value J + 1) — all the owner of the next diagonal tile waits for
  __shared__ int hand_over;
  if (t == 0) hand_over = 0;
  // The owner of those rows always reaches its store (no early exit lies before it), so the wait ends; the bound is there so that the
  // grid drains whatever happens — and if it were ever hit the factorisation is NOT delivered: the instance ends with status 5.
  auto wait_hand_over = [&](int value) {
    int spin = 0;
    while (__hip_atomic_load(&hand_over, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < value && ++spin < (1 << 22)) __builtin_amdgcn_s_sleep(1);
    if (spin >= (1 << 22)) inst[bi].status = 5;
  };
  auto row0 = [&](int I) { return I < nbb ? W * I : G.Nb + W * (I - nbb); };
  auto rend = [&](int I) { return I < nbb ? G.Nb : G.Nt; };
  // assemble: the block is built here, not read — the values of its structural slots (a few per cent of the storage) go to LDS
  // (the panel's space, free until the first block column is solved), number 0 being a structural zero; every tile lane then picks
  // its four entries by number (df_map).  The right-hand side entries that go with the diagonal slots are written on the way.
  double* vals = BL;
  unsigned long long mp[MAXS];     // a tile wave's lanes: the numbers of the entries they hold, on their way while the values are fetched
  if (assemble) {
    if (wv != NWV) {
#pragma unroll
      for (int s = 0; s < MAXS; ++s) mp[s] = D.df_map[(size_t(sidx) * D.df_tiles + wv + NWV * s) * 64 + lane];
    }
    const int ea = D.df_ptr[3 * sidx], eb = D.df_ptr[3 * sidx + 1], ec = D.df_ptr[3 * sidx + 2], ed = D.df_ptr[3 * sidx + 3];
    const SlotValue value(D, bi);
    if (t == 0) vals[0] = 0.0;
    const double* jac = D.jac + size_t(bi) * D.sv;
#pragma unroll 4
    for (int e = ea + t; e < eb; e += 512) vals[1 + e - ea] = jac[D.df_ki[e] & 0x0fffffff];
    // (SlotValue's Hessian duplicate sum, restated: a loop of its own for the Hessian slots, which avoids divergence)
    const bool with_h = value.mode == 0 && !D.lb_on;
    const double* hess = D.hess + size_t(bi) * D.nnz_h;
#pragma unroll 2
    for (int e = eb + t; e < ec; e += 512) {
      double a = 0.0;
      if (with_h) {
        const int hgi = D.df_ki[e] & 0x0fffffff;
        for (int j = D.hg_ptr[hgi]; j < D.hg_ptr[hgi + 1]; ++j) a += hess[D.hg_src[j]];
      }
      vals[1 + e - ea] = 0.0 + a;
    }
    for (int e = ec + t; e < ed; e += 512) vals[1 + e - ea] = value(D.df_ki, D.df_hg, e);
    __syncthreads();
  }
  // forward: the first half of the substitution that follows an accepted factorisation (kkt_solve_kernel's phase 1: L y = r over the
  // band blocks, the border work space takes -L_border y) runs along with the elimination — the panel of a block column is in
  // LDS anyway, and the factor is not streamed from HBM a second time for it.  Same sums in the same order as that kernel's.
  double* rg = D.rhs + size_t(bi) * D.Nt + sub.roff;
  if (forward) {
    for (int i = t; i < G.Nt; i += 512) {
      const int I = i < G.Nb ? i / W : nbb + (i - G.Nb) / W;
      rsh[I * W + (i - row0(I))] = rg[i];
    }
  }
  if (wv == NWV) {
    // ---------------- the eighth wave holds no tiles: it factors the diagonal blocks (its registers are free for that) ----------------
    __builtin_amdgcn_s_setprio(3);   // the chain of diagonal blocks is the critical path: this wave goes first on its SIMD
    PivotCount pc = {0, 0, 0};
#ifdef IPM_TIMING
    long long tq[4] = {0, 0, 0, 0}, tp = wall_clock64();
#define IPM_DTICK(i) do { const long long n_ = wall_clock64(); tq[i] += n_ - tp; tp = n_; } while (0)
#else
#define IPM_DTICK(i)
#endif
    for (int J = 0; J < nbe; ++J) {
      const int J0 = row0(J), w = min(W, rend(J) - J0);
      double* DgJ = Dg + (J & 1) * DGN;
      IPM_LDS_BARRIER();          // B1: the owner of tile (J, J) has put it into its copy of Dg — and, from J = 1 on, block column J - 1's panel is in LDS
      IPM_DTICK(0);
      {   // kkt_factor_kernel's elimination, entry for entry, over all 64 lanes (DiagStep)
        double R[4], V[4];
        int a_col[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int j = 4 * g + lq;
          R[g] = (lr < w && j <= lr) ? DgJ[lr * (W + 1) + j] : (j == lr ? 1.0 : 0.0);
          V[g] = j == lr ? 1.0 : 0.0;
          a_col[g] = j << 2;
        }
        DiagStep<0>::run(R, V, lq, lr, lr << 2, a_col);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int j = 4 * g + lq;
          if (lr < w && j <= lr) DgJ[lr * (W + 1) + j] = R[g];
          Mi[lr * IPM_DENSE_LDS_ROW + j] = V[g];
          if (j == lr) {
            invd[lr] = lr < w ? 1.0 / R[g] : 0.0;
            dv[lr] = lr < w ? R[g] : 0.0;
          }
        }
      }
      IPM_DTICK(1);
      IPM_LDS_BARRIER();          // B2: Dg, Mi, invd are there
      if (forward) {              // y = L11^-1 r of this block's unknowns (r is final: the tile waves added the last panel's share before B2),
        double y = lr < w ? rsh[J * W + lr] : 0.0;   // while they solve the panel
#pragma unroll
        for (int k = 0; k < W; ++k) {
          const double zk = k < w ? rsh[J * W + k] : 0.0;
          if (k < lr && lr < w) y = __builtin_fma(Mi[lr * IPM_DENSE_LDS_ROW + k], zk, y);
        }
        if (lq == 0) {
          ysh[lr] = y;
          if (lr < w) rg[J0 + lr] = y;
        }
      }
      // the diagonal block is stored as d on the diagonal and L11^-1 below it (what the solves use)
      for (int idx = lane; idx < W * W; idx += 64) {
        const int di = idx / W, dj = idx % W;
        if (di < w && dj <= di) K[G.at(J0 + di, J0 + dj)] = di == dj ? DgJ[di * (W + 1) + dj] : Mi[di * IPM_DENSE_LDS_ROW + dj];
      }
      if (lane < w) pc = count_pivot(DgJ[lane * (W + 1) + lane], pc);
      IPM_DTICK(2);
    }
    IPM_LDS_BARRIER();            // the last block column's panel is in LDS (the tile waves' last meeting point)
#ifdef IPM_TIMING
    if (lane == 0 && sidx == 0) { inst[bi].dbg[6] = tq[0] + tq[2]; inst[bi].dbg[7] = tq[1]; }   // waiting for the tile waves | factoring
#endif
    int npos = pc.npos, nneg = pc.nneg, nbad = pc.nbad;
    for (int o = 32; o; o >>= 1) { npos += __shfl_xor(npos, o); nneg += __shfl_xor(nneg, o); nbad += __shfl_xor(nbad, o); }
    if (lane == 0) {
      int* pv = piv + (size_t(bi) * n_sub + sidx) * 3;
      pv[0] = npos; pv[1] = nneg; pv[2] = nbad;
    }
    return;
  }
  // ---------------- tile waves ----------------
  // Tiles are numbered column by column (tile (I, K): K NTB - K (K - 1) / 2 + I - K) and dealt round robin, slot s of wave wv
  // holds tile wv + 7 s: the tiles a step touches are then a RANGE of slots — those of block column J for the panel solve,
  // everything from the first tile of column J + 1 on for the update — entered through a switch and walked without a branch
  // per tile, so that the LDS reads and matrix products of successive tiles overlap.
#define IPM_REP22(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15) M(16) M(17) M(18) M(19) M(20) M(21)
  static_assert(MAXS == 22, "IPM_REP22");
  auto colstart = [&](int Kr) { return Kr * R - Kr * (Kr - 1) / 2; };   // first resident tile of block column E + Kr
  // a tile of an early block column: from / to the storage, in the register tiles' layout (tile (I, Kb) belongs to wave I % 7)
  auto t_load = [&](int I, int Kb) {
    d4 a;
    const int r = row0(I) + lr;
    const bool rv = r < rend(I), border = r >= G.Nb;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cc = row0(Kb) + lq + 4 * g;
      a[g] = (rv && cc < rend(Kb) && cc <= r && (border || r - cc <= G.b)) ? K[G.at(r, cc)] : 0.0;
    }
    return a;
  };
  auto t_store = [&](const d4& a, int I, int Kb) {
    const int r = row0(I) + lr;
    const bool rv = r < rend(I), border = r >= G.Nb;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cc = row0(Kb) + lq + 4 * g;
      if (rv && cc < rend(Kb) && cc <= r && (border || r - cc <= G.b)) K[G.at(r, cc)] = a[g];
    }
  };
  auto t_update = [&](d4 a, int I, int Kb) {       // A(I, Kb) -= L(I, J) D L(Kb, J)^T from the panel in LDS (IPM_UPD_BODY's products)
    const double* bl = BL + (I * W + lr) * BS + lq;
    const double* by = BY + (Kb * W + lr) * BS + lq;
#pragma unroll
    for (int g = 0; g < 4; ++g) a = __builtin_amdgcn_mfma_f64_16x16x4f64(-by[4 * g], bl[4 * g], a, 0, 0, 0);
    return a;
  };
  auto t_put = [&](const d4& a, int wd, double* dg) {   // a diagonal tile of width wd: its lower triangle to Dg
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = lq + 4 * g;
      if (lr < wd && c <= lr) dg[lr * (W + 1) + c] = a[g];
    }
  };
  if (assemble && E > 0) {       // the early tiles are built in the storage (the values' LDS space is the panel's)
    for (int Kb = 0; Kb < E; ++Kb)
      for (int I = Kb; I < NTB; ++I) {
        if (I % NWV != wv) continue;
        const unsigned long long m = D.df_map[(size_t(sidx) * D.df_tiles + ipm_dense_tile(NTB, I, Kb)) * 64 + lane];
        d4 a;
#pragma unroll
        for (int g = 0; g < 4; ++g) a[g] = vals[(m >> (16 * g)) & 0xffff];
        t_store(a, I, Kb);
      }
  }
  int sIK[MAXS];                // block row << 8 | block column of the slot's tile (wave-uniform); unused slots: tile (0, 0), never stored
  d4 acc[MAXS];
#pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    const int tl = wv + NWV * s;
    int Kb = 0;
    while (Kb + 1 < R && colstart(Kb + 1) <= tl) ++Kb;
    const bool have = tl < ntl;
    const int I = have ? E + Kb + (tl - colstart(Kb)) : 0;
    Kb = have ? E + Kb : 0;
    sIK[s] = __builtin_amdgcn_readfirstlane(I << 8 | Kb);
    if (assemble) {
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[s][g] = vals[(mp[s] >> (16 * g)) & 0xffff];
      continue;
    }
    const int r = row0(I) + lr;
    const bool rv = have && r < rend(I), border = r >= G.Nb;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cc = row0(Kb) + lq + 4 * g;
      const bool ok = rv && cc < rend(Kb) && cc <= r && (border || r - cc <= G.b);
      acc[s][g] = ok ? K[G.at(r, cc)] : 0.0;
    }
  }
  auto first_slot_at = [&](int tl) { return tl <= wv ? 0 : (tl - wv + NWV - 1) / NWV; };   // first slot of this wave with tile number >= tl
  // slot s takes its rank-16 update from the panel in LDS: A(I, K) -= L(I, J) D L(K, J)^T
#define IPM_UPD_BODY(s) {                                                                                                    \
    int ik = sIK[s];                                                                                                         \
    asm volatile("" : "+s"(ik));   /* keeps the 44 LDS addresses from being hoisted out of the J loop into registers */      \
    const double* bl = BL + ((ik >> 8) * W + lr) * BS + lq;                                                                  \
    const double* by = BY + ((ik & 255) * W + lr) * BS + lq;                                                                 \
    _Pragma("unroll") for (int g = 0; g < 4; ++g) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(-by[4 * g], bl[4 * g], acc[s], 0, 0, 0); \
  }
  // slot s is a diagonal tile of width wd: its lower triangle goes to Dg for the eighth wave
#define IPM_PUT_BODY(s, wd, dg) { _Pragma("unroll") for (int g = 0; g < 4; ++g) { const int c = lq + 4 * g; if (lr < (wd) && c <= lr) (dg)[lr * (W + 1) + c] = acc[s][g]; } }
  if (wv == 0) {
    if (E == 0) IPM_PUT_BODY(0, min(W, rend(0)), Dg)    // tile (0, 0) is tile number 0: slot 0 of wave 0
    else t_put(t_load(0, 0), min(W, rend(0)), Dg);
  }
  // early block column J: this wave's tiles (I, J), I > J, in ebuf (I = first such I + 7 q) for its panel only — kept across the
  // resident tiles' update they pushed those out of the registers —, tile (J + 1, J + 1) in edg with the wave that owns it, fetched a step ahead
  constexpr int EQ = (IPM_DENSE_ROWS + IPM_DENSE_EARLY - 1 + NWV - 1) / NWV;
  d4 ebuf[EQ], edg;
  auto first_own = [&](int from) { return from + (wv - from % NWV + NWV) % NWV; };   // first I >= from with I % 7 == wv
  if (E > 0) {
    const int f0 = first_own(1);
#pragma unroll
    for (int q = 0; q < EQ; ++q)
      if (f0 + NWV * q < NTB) ebuf[q] = t_load(f0 + NWV * q, 0);
    if (E > 1 && 1 % NWV == wv) edg = t_load(1, 1);
  }
  IPM_LDS_BARRIER();              // B1 of block column 0
  IPM_LDS_BARRIER();              // B2: its diagonal block is factored
#ifdef IPM_TIMING
  long long tw[6] = {0, 0, 0, 0, 0, 0}, twp = wall_clock64();
#ifdef IPM_TIMING_EARLY   // the phases of the EARLY block columns in the record's places, everything else in "early"
#define IPM_ETICK(i) do { const long long n_ = wall_clock64(); tw[i] += n_ - twp; twp = n_; } while (0)
#define IPM_TTICK(i) do { const long long n_ = wall_clock64(); tw[5] += n_ - twp; twp = n_; } while (0)
#else
#define IPM_TTICK(i) do { const long long n_ = wall_clock64(); tw[i] += n_ - twp; twp = n_; } while (0)
#define IPM_ETICK(i) IPM_TTICK(5)
#endif
#else
#define IPM_TTICK(i)
#define IPM_ETICK(i)
#endif
  // forward: r(row) -= L(row, J) y for every row below block column J, thread p owns row p of the tile rows.  Off the chain of
  // diagonal blocks: after the next diagonal tile has been handed over (the panel and y stay in LDS until the next B2)
  auto forward_share = [&](int J) {
    const int I = t >> 4;
    if (I > J && I < NTB && row0(I) + lr < rend(I)) {
      const double* bl = BL + (size_t(I) * W + lr) * BS;
      double a = 0.0;
#pragma unroll
      for (int c = 0; c < W; ++c) a = __builtin_fma(bl[c], ysh[c], a);
      rsh[I * W + lr] -= a;
    }
  };
  // a corner tile's panel solve by substitution: Y(r, c) = A(r, c) - sum_{k < c} Y(r, k) L11(c, k), L11 below the diagonal of Dg
  auto corner_subst = [&](const d4& a, int J) {
    const double* DgJ = Dg + (J & 1) * DGN;
    d4 y = a;
#pragma unroll
    for (int c = 0; c < W - 1; ++c) {
      const double yc = __shfl(y[c >> 2], lr + 16 * (c & 3));   // Y(r, c) is final: from the lane of this row that holds column c
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j = lq + 4 * g;
        if (j > c) y[g] = __builtin_fma(-yc, DgJ[j * (W + 1) + c], y[g]);
      }
    }
    return y;
  };
  for (int J = 0; J < nbe; ++J) {
    const int J0 = row0(J), w = min(W, rend(J) - J0);
    int s0_early = 0;
    if (EARLY && J < E) {
      // ---- an early block column: the same steps with its tiles (and those of the early columns to its right) taken from the
      // storage, each by the wave that owns it; the resident tiles take their update as always
      IPM_ETICK(4);
      const int f0 = first_own(J + 1);
      if (J > 0) {              // this column's tiles: fetched now (they have the updates of the columns before J - 1), updated with
#pragma unroll                  // column J - 1's panel, which is still in LDS
        for (int q = 0; q < EQ; ++q)
          if (f0 + NWV * q < NTB) ebuf[q] = t_load(f0 + NWV * q, J);
#pragma unroll
        for (int q = 0; q < EQ; ++q)
          if (f0 + NWV * q < NTB) ebuf[q] = t_update(ebuf[q], f0 + NWV * q, J);
      }
#pragma unroll
      for (int q = 0; q < EQ; ++q) {
        const int I = f0 + NWV * q;
        if (I >= NTB) break;
        d4 y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int g = 0; g < 4; ++g) y = __builtin_amdgcn_mfma_f64_16x16x4f64(Mi[lr * IPM_DENSE_LDS_ROW + 4 * g + lq], ebuf[q][g], y, 0, 0, 0);
        const int r = row0(I) + lr;
        const bool rv = r < rend(I), border = r >= G.Nb;
        const int kstep = border ? G.CS : G.CS - 1;
        double* kp = K + (size_t(J0) * G.CS + (border ? G.b + 1 + r - G.Nb : r - J0)) + lq * kstep;
        const int lo_ = (I * W + lr) * BS + lq;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c = lq + 4 * g;
          const double l = y[g] * invd[c];
          const bool ok = rv && c < w;
          if (ok && (border || r - (J0 + c) <= G.b)) kp[4 * g * kstep] = l;
          BL[lo_ + 4 * g] = ok ? l : 0.0;
          BY[lo_ + 4 * g] = ok ? (border ? y[g] : l * dv[c]) : 0.0;
        }
        if (I == J + 1) __hip_atomic_store(&hand_over, J + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      IPM_ETICK(0);
      int s0 = 0;
      if (J + 1 < nbe) {        // the next diagonal tile, before the workgroup meets
        const int w1 = min(W, rend(J + 1) - row0(J + 1));
        double* DgN = Dg + ((J + 1) & 1) * DGN;
        if (J + 1 < E) {
          if ((J + 1) % NWV == wv) t_put(t_update(edg, J + 1, J + 1), w1, DgN);   // (this wave wrote the panel's rows it needs)
        } else if (wv == 0) {   // the first resident tile: slot 0 of wave 0
          wait_hand_over(J + 1);
          IPM_UPD_BODY(0) IPM_PUT_BODY(0, w1, DgN)
          s0 = 1;
        }
      }
      s0_early = s0;
    }
    const int cs = colstart(max(J - E, 0)), cs1 = colstart(max(J - E, 0) + 1);
    if (!(EARLY && J < E)) {
    IPM_TTICK(4);               // waiting at B2
    // the tiles below the diagonal one: Y^T = L11^-1 A^T, L^T = D^-1 Y^T; both go to LDS for the updates, L to the storage
    {
      const int sa = first_slot_at(cs + 1), sb = min(MAXS, first_slot_at(cs1));   // slots [sa, sb)
      const bool first_owner = (cs + 1) % NWV == wv;   // this wave's first tile of the column is (J + 1, J): the rows the next diagonal tile needs
      if (CORNER && J >= nbb) {
        // a corner block column: one copy of the substitution code for all slots (inside the switch it would be there 22 times)
        for (int sl = sa; sl < sb; ++sl) {
          d4 a = {0.0, 0.0, 0.0, 0.0};
          switch (sl) {
#define IPM_PICK(s) case s: a = acc[s]; break;
            IPM_REP22(IPM_PICK)
#undef IPM_PICK
            default: break;
          }
          const d4 y = corner_subst(a, J);
          const int I = J + (wv + NWV * sl - cs), r = row0(I) + lr;
          const bool rv = r < rend(I);
          double* kp = K + (size_t(J0) * G.CS + (G.b + 1 + r - G.Nb)) + lq * G.CS;      // (every row below a corner column is a border row)
          const int lo_ = (I * W + lr) * BS + lq;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int c = lq + 4 * g;
            const bool ok = rv && c < w;
            const double l = ok ? y[g] / dv[c] : 0.0;
            if (ok) kp[4 * g * G.CS] = l;
            BL[lo_ + 4 * g] = l;
            BY[lo_ + 4 * g] = ok ? y[g] : 0.0;
          }
          if (sl == sa && first_owner) __hip_atomic_store(&hand_over, J + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      } else
      switch (sa) {
#define IPM_PANEL(s) case s: if (s < sb) {                                                                                   \
          d4 y = {0.0, 0.0, 0.0, 0.0};                                                                                       \
          _Pragma("unroll") for (int g = 0; g < 4; ++g) y = __builtin_amdgcn_mfma_f64_16x16x4f64(Mi[lr * IPM_DENSE_LDS_ROW + 4 * g + lq], acc[s][g], y, 0, 0, 0); \
          int ik = sIK[s];                                                                                                   \
          asm volatile("" : "+s"(ik));                                                                                       \
          const int I = ik >> 8, r = row0(I) + lr;                                                                           \
          const bool rv = r < rend(I), border = r >= G.Nb;                                                                   \
          /* the four entries of a lane sit 4 columns apart: one 64-bit address (row r, column J0 + lq) and a 32-bit step — a   \
             per-entry G.at() is a 64-bit vector multiply each, and the stores' address arithmetic was 60 % of the panel's time */ \
          const int kstep = border ? G.CS : G.CS - 1;                                                                        \
          double* kp = K + (size_t(J0) * G.CS + (border ? G.b + 1 + r - G.Nb : r - J0)) + lq * kstep;                         \
          const int lo_ = (I * W + lr) * BS + lq;                                                                            \
          _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                                    \
            const int c = lq + 4 * g;                                                                                        \
            const double l = y[g] * invd[c];                                                                                 \
            const bool ok = rv && c < w;                                                                                     \
            if (ok && (border || r - (J0 + c) <= G.b)) kp[4 * g * kstep] = l;                                                \
            BL[lo_ + 4 * g] = ok ? l : 0.0;                                                                                  \
            /* L D as kkt_factor_kernel forms it: the product of the stored l and d for a band row (its T), y itself for a   \
               border row (its BY) — the two differ in the last bit, and Delta-III's path is sensitive to that */            \
            BY[lo_ + 4 * g] = ok ? (border ? y[g] : l * dv[c]) : 0.0;                                                        \
          }                                                                                                                  \
          if (s == sa && first_owner) __hip_atomic_store(&hand_over, J + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); \
        }
        IPM_REP22(IPM_PANEL)
#undef IPM_PANEL
        default: break;
      }
    }
    IPM_TTICK(0);               // panel
    }
    // every tile to the right takes its update; the next diagonal tile first and BEFORE the workgroup meets: its owner needs the
    // panel's rows of block row J + 1 only, which their owner announces (hand_over) after its first tile.  One barrier then says
    // both "the panel is in LDS" and "the next diagonal tile is in its copy of Dg" (they were two, with this update between them)
    int s0 = (EARLY && J < E) ? s0_early : first_slot_at(cs1);
    if (!(EARLY && J < E) && J + 1 < nbe && cs1 % NWV == wv) {
      const int w1 = min(W, rend(J + 1) - row0(J + 1));
      double* DgN = Dg + ((J + 1) & 1) * DGN;
      wait_hand_over(J + 1);
      switch (s0) {
#define IPM_NEXT(s) case s: IPM_UPD_BODY(s) IPM_PUT_BODY(s, w1, DgN) break;
        IPM_REP22(IPM_NEXT)
#undef IPM_NEXT
        default: break;
      }
      ++s0;
    }
    IPM_TTICK(2);               // next diagonal tile
    IPM_LDS_BARRIER();            // the panel is in LDS; B1 of block column J + 1
    IPM_TTICK(1);               // waiting there
    if (forward) forward_share(J);
    switch (s0) {
#define IPM_UPD(s) case s: IPM_UPD_BODY(s) if (s & 1) __builtin_amdgcn_sched_barrier(0);   /* two tiles' loads and products may interleave, not all 22 (registers) */
      IPM_REP22(IPM_UPD)
#undef IPM_UPD
      default: break;
    }
    if (EARLY && J < E) {
      for (int Kb = J + 2; Kb < E; ++Kb)      // early columns further right: through the storage
        for (int I = first_own(Kb); I < NTB; I += NWV) t_store(t_update(t_load(I, Kb), I, Kb), I, Kb);
      if (J + 2 < E && (J + 2) % NWV == wv) edg = t_load(J + 2, J + 2);
    }
    IPM_TTICK(3);               // update
    if (J + 1 < nbe) IPM_LDS_BARRIER();   // B2 of block column J + 1
  }
#ifdef IPM_TIMING
  // (build with -DIPM_TIMING_SUB=<out of range> so that the left-looking kernel of the last level leaves these alone:
  //  wave 0's panel | wait at B3 | next diagonal tile + B1 | update | wait at B2, 100 MHz ticks per interval block)
  if (t == 0 && sidx == 0) { inst[bi].dbg[0] = tw[0]; inst[bi].dbg[1] = tw[1]; inst[bi].dbg[2] = tw[2]; inst[bi].dbg[3] = tw[3]; inst[bi].dbg[4] = tw[4]; inst[bi].dbg[5] = tw[5]; }
#endif
#undef IPM_UPD_BODY
#undef IPM_PUT_BODY
  if (forward) {   // the border work space (each row by the thread that kept it)
    const int I = t >> 4;
    if (I >= nbb && I < NTB && row0(I) + lr < rend(I)) rg[row0(I) + lr] = rsh[I * W + lr];
  }
  // the Schur complement of the corner, unfactored, back into the corner's storage
#pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    if (partial && (sIK[s] & 255) >= nbb && wv + NWV * s < ntl) {
      const int r = row0(sIK[s] >> 8) + lr;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cc = row0(sIK[s] & 255) + lq + 4 * g;
        if (r < G.Nt && cc < G.Nt && cc <= r) K[G.at(r, cc)] = acc[s][g];
      }
    }
  }
#undef IPM_REP22
#undef IPM_LDS_BARRIER
}
size_t kkt_factor_dense_lds_bytes(int block_rows) {
  return (2 * size_t(IPM_W) * (IPM_W + 1) + size_t(IPM_W) * IPM_DENSE_LDS_ROW + 2 * IPM_W + 2 * size_t(block_rows) * IPM_W * IPM_DENSE_LDS_ROW +
          size_t(block_rows) * IPM_W + IPM_W) * sizeof(double);
}
int kkt_factor_dense_max_block_rows() {   // 7 waves x IPM_DENSE_SLOTS tiles hold the lower triangle of IPM_DENSE_ROWS block rows; the early columns on top
  return IPM_DENSE_ROWS + IPM_DENSE_EARLY;
}
hipError_t kkt_factor_dense_prepare(size_t lds_bytes) {
  if (lds_bytes <= 48 * 1024) return hipSuccess;
  const int plain = int(std::min(lds_bytes, kkt_factor_dense_lds_bytes(IPM_DENSE_ROWS)));
  hipError_t er = hipFuncSetAttribute(reinterpret_cast<const void*>(kkt_factor_dense_kernel<false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, plain);
  if (er == hipSuccess)
    er = hipFuncSetAttribute(reinterpret_cast<const void*>(kkt_factor_dense_kernel<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, plain);
  if (er != hipSuccess || lds_bytes <= kkt_factor_dense_lds_bytes(IPM_DENSE_ROWS)) return er;
  er = hipFuncSetAttribute(reinterpret_cast<const void*>(kkt_factor_dense_kernel<true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes));
  if (er != hipSuccess) return er;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kkt_factor_dense_kernel<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes));
}
// (the LDS size says how many block rows a level's largest block has)
static bool dense_early(size_t lds_bytes) { return lds_bytes > kkt_factor_dense_lds_bytes(IPM_DENSE_ROWS); }

size_t kkt_factor_lds_bytes(const IpmPlan& p) {
  return p.nd ? p.max_factor_lds : ipm_factor_lds_bytes(p.b, p.nb);
}
// tiles_per_wave, here and in launch_factor_subs: 4 and 6 are MT tiles per wave of 4 waves (block columns of up to 256 and 384
// rows), the two-digit codes 28 and 38 are <MT, NW> = <2, 8> and <3, 8> — the same rows over 8 waves, for a few large
// instances —, anything else IPM_MT tiles per wave of 4 waves (512 rows)
hipError_t kkt_factor_prepare(int tiles_per_wave, size_t lds_bytes) {
  if (lds_bytes <= 48 * 1024) return hipSuccess;
  if (tiles_per_wave == 38) return hipFuncSetAttribute(reinterpret_cast<const void*>(kkt_factor_kernel<3, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes));
  if (tiles_per_wave == 28) return hipFuncSetAttribute(reinterpret_cast<const void*>(kkt_factor_kernel<2, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes));
  return hipFuncSetAttribute(tiles_per_wave == 4 ? reinterpret_cast<const void*>(kkt_factor_kernel<4>)
                             : tiles_per_wave == 6 ? reinterpret_cast<const void*>(kkt_factor_kernel<6>)
                                                   : reinterpret_cast<const void*>(kkt_factor_kernel<IPM_MT>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes));
}
// ---- nested dissection glue: sums in a fixed (interval) order, so the factorisation stays deterministic ----------------------
// K[dst[i]] += sum_j K[src[j]], j in [ptr[i], ptr[i+1]): the level-1 Schur complements into the separator system
// Destinations are sorted by the length of their source lists (build_ipm_plan_nd): the first n_long of them (>= 32 sources: the
// global border's corner entries collect one contribution from EVERY interval, 256 on the metric problem) take a wave each —
// lanes stride the list, partial sums combined in a fixed butterfly order — the rest a thread each.
__global__ void kkt_gather_add_kernel(double* Kall, long long kstride, const int* __restrict__ ptr, const int* __restrict__ src,
                                      const int* __restrict__ dst, int n, const IpmInst* inst, int need_refactor, int n_long, int kmod) {
  const int bi = blockIdx.y, bk = bi % kmod;
  if (inst[bk].status != 0 || (need_refactor && !inst[bk].refactor)) return;
  double* K = Kall + size_t(bi) * kstride;
  const int lane = threadIdx.x & 63, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
  for (int i = wave; i < n_long; i += n_waves) {
    double acc = 0.0;
    for (int j = ptr[i] + lane; j < ptr[i + 1]; j += 64) acc += K[src[j]];
    for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) K[dst[i]] += acc;
  }
  for (int i = n_long + blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    double acc = K[dst[i]];
    for (int j = ptr[i]; j < ptr[i + 1]; ++j) acc += K[src[j]];
    K[dst[i]] = acc;
  }
}

// level 1 assembled and forward-substituted inside kkt_factor_dense_kernel
int kkt_level1_fused(const IpmDev& D) { return (D.n_l1 > 0 && D.l1_dense_lds && D.df_on && D.df_map) ? 1 : 0; }
static void launch_factor_subs(const IpmDev& D, int sub0, int n_here, int partial, int tiles_per_wave, size_t lds_bytes, hipStream_t st,
                               size_t dense_lds = 0) {
  const dim3 grid(unsigned(D.B) * unsigned(n_here));
  if (dense_lds) {   // every sub-problem of this level fits the register tiles
    // a last level: its corner there too (D.last_dense_corner; the panels of the corner's block columns by substitution, see the
    // kernel), or by kkt_factor_kernel's unblocked elimination (partial = 2: 143 us for the metric problem's 73 x 73)
    const bool corner = !partial && D.last_dense_corner;
    const int dense_partial = corner ? 0 : 1;
#define IPM_LAUNCH_DENSE(EARLY_, CORNER_)                                                                                          \
    hipLaunchKernelGGL((kkt_factor_dense_kernel<EARLY_, CORNER_>), grid, dim3(512), dense_lds, st, D.K, D.kstride, D.subs, sub0, n_here, D.n_sub, \
                       D.inst, D.piv, D, 0, 0, dense_partial)
    if (dense_early(dense_lds)) { if (corner) IPM_LAUNCH_DENSE(true, true); else IPM_LAUNCH_DENSE(true, false); }
    else { if (corner) IPM_LAUNCH_DENSE(false, true); else IPM_LAUNCH_DENSE(false, false); }
#undef IPM_LAUNCH_DENSE
    if (partial || corner) return;
    partial = 2;       // the corner alone, below
  }
  if (tiles_per_wave == 28)
    hipLaunchKernelGGL((kkt_factor_kernel<2, 8>), grid, dim3(512), lds_bytes, st, D.K, D.kstride, D.subs, sub0, n_here, D.n_sub, D.inst, D.piv, partial);
  else if (tiles_per_wave == 38)
    hipLaunchKernelGGL((kkt_factor_kernel<3, 8>), grid, dim3(512), lds_bytes, st, D.K, D.kstride, D.subs, sub0, n_here, D.n_sub, D.inst, D.piv, partial);
  else if (tiles_per_wave == 4)
    hipLaunchKernelGGL(kkt_factor_kernel<4>, grid, dim3(256), lds_bytes, st, D.K, D.kstride, D.subs, sub0, n_here, D.n_sub, D.inst, D.piv, partial);
  else if (tiles_per_wave == 6)
    hipLaunchKernelGGL(kkt_factor_kernel<6>, grid, dim3(256), lds_bytes, st, D.K, D.kstride, D.subs, sub0, n_here, D.n_sub, D.inst, D.piv, partial);
  else
    hipLaunchKernelGGL(kkt_factor_kernel<IPM_MT>, grid, dim3(256), lds_bytes, st, D.K, D.kstride, D.subs, sub0, n_here, D.n_sub, D.inst, D.piv,
                       partial);
}
void kkt_launch_factor(const IpmDev& D, int tiles_per_wave, size_t lds_bytes, hipStream_t st) {
  if (D.n_l1 == 0) {
    launch_factor_subs(D, 0, 1, 0, tiles_per_wave, lds_bytes, st);
    return;
  }
  auto corners = [&](const int* ptr, const int* src, const int* dst, int n, int n_long) {
    if (!n) return;
    const unsigned blocks = unsigned(std::max(1, std::min(1024, (n + 255) / 256)));
    hipLaunchKernelGGL(kkt_gather_add_kernel, dim3(blocks, unsigned(D.B)), dim3(256), 0, st, D.K, D.kstride, ptr, src, dst, n, D.inst, 1, n_long, D.B);
  };
  const int fused = kkt_level1_fused(D);
  if (fused) kkt_launch_vec(D, unsigned(D.B), D.gap_pos, nullptr, D.n_gap, 0, 3, st);   // the forward sweep runs inside the kernel: border work spaces start at zero
  if (D.l1_dense_lds && dense_early(D.l1_dense_lds))                                   // every interval up to its corner
    hipLaunchKernelGGL((kkt_factor_dense_kernel<true, false>), dim3(unsigned(D.B) * unsigned(D.n_l1)), dim3(512), D.l1_dense_lds, st, D.K, D.kstride, D.subs, 0,
                       D.n_l1, D.n_sub, D.inst, D.piv, D, fused, fused, 1);
  else if (D.l1_dense_lds)
    hipLaunchKernelGGL((kkt_factor_dense_kernel<false, false>), dim3(unsigned(D.B) * unsigned(D.n_l1)), dim3(512), D.l1_dense_lds, st, D.K, D.kstride, D.subs, 0,
                       D.n_l1, D.n_sub, D.inst, D.piv, D, fused, fused, 1);
  else
    launch_factor_subs(D, 0, D.n_l1, 1, tiles_per_wave, lds_bytes, st);
  corners(D.cg_ptr, D.cg_src, D.cg_dst, D.n_cg, D.n_cg_long);
  if (D.n_l2) {
    launch_factor_subs(D, D.n_l1, D.n_l2, 1, tiles_per_wave, lds_bytes, st, D.l2_dense_lds);   // every group of separators up to its corner
    corners(D.cg2_ptr, D.cg2_src, D.cg2_dst, D.n_cg2, D.n_cg2_long);
  }
  launch_factor_subs(D, D.n_l1 + D.n_l2, 1, 0, tiles_per_wave, lds_bytes, st, D.last_dense_lds);   // last level: (group) separators + border
}

}  // namespace rpm
