// Sustained store probe (perf exploration): what the write path takes for the byte stream of ONE rpm_tile_pl_kernel launch of
// the metric problem (64 iterates, ~450 MB, ~100 us), from the kernel's own launch shape and nothing else.  No arithmetic, no
// loads: persistent workgroups, one per CU, 768 threads = two halves x (4 "compute" + 2 "DMA" waves).  A half walks tiles
// slot, slot + G, ... (G = 2 x workgroups) of 64 nodes; tile item = instance * tiles_per_instance + tile, as in the kernel:
//   * the compute waves write the tile's 512-byte runs (8 B per lane) of the g rows and the Jacobian blocks in three bursts
//     (wave c takes roles c, c + 4, c + 8; role 0: the NO rows of g, roles 1..NV-1: NO blocks, role NV: 2 NO blocks);
//   * the DMA waves write the tile's share of the constant block, NX copies, as 16-byte stores from a 128-byte line boundary,
//     after the barrier that opens the tile.
// Parameters: the tile order (which slot of a round a half takes), the store policy of each stream, and a linear reference
// (the same bytes as a plain 16-byte-per-lane fill from the same persistent shape).
// Vector stores only; one barrier per tile as in the kernel.
#include <hip/hip_runtime.h>

typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));

// store policies: 0 plain, 1 non-temporal, 2 write-through (sc1), 3 write-through + non-temporal
template <int POLICY>
__device__ __forceinline__ void ss_store(double* p, double v) {
  if constexpr (POLICY == 0) *p = v;
  else if constexpr (POLICY == 1) __builtin_nontemporal_store(v, p);
  else if constexpr (POLICY == 2) asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
  else asm volatile("global_store_dwordx2 %0, %1, off sc1 nt" ::"v"(p), "v"(v) : "memory");
}
template <int POLICY>
__device__ __forceinline__ void ss_store(d2u* p, d2u v) {
  if constexpr (POLICY == 0) *p = v;
  else if constexpr (POLICY == 1) __builtin_nontemporal_store(v, p);
  else if constexpr (POLICY == 2) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
  else asm volatile("global_store_dwordx4 %0, %1, off sc1 nt\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

// The slot in [0, G) of a round that half `half` of workgroup b takes; G = nh * nb.  Workgroups b, b + 8, ... share an XCD.
//   0  each XCD a contiguous eighth of the round (the kernel's xcd_place: one instance per XCD and round on the metric problem)
//   1  round-robin: slot = nh * b + half
//   2  the round in two groups of four eighths; XCD 4 q + c takes quarter c of each eighth of group q (one phase of four
//      instances per XCD and round)
//   3  XCD pairs: a pair takes a contiguous quarter of the round, its two XCDs alternate workgroup-sized pieces (nh tiles)
//   4  like 3, alternating single tiles
// 2..4 need nb % 8 == 0 (2: G % 32 == 0 as well); other grids take order 0.
__host__ __device__ inline int ss_slot(int order, int nh, int nb, int b, int half) {
  const int xcd = b & 7, i = b >> 3;
  if (order == 1) return nh * b + half;
  if (order >= 2 && (nb & 7) == 0) {
    const int S = nh * (nb >> 3), l = nh * i + half;   // slots per XCD, this half's among them
    if (order == 2 && (S & 3) == 0) {
      const int Q = S >> 2, q = xcd >> 2, c = xcd & 3, r = l / Q, t = l - r * Q;
      return q * 4 * S + r * S + c * Q + t;
    }
    if (order == 3) return (xcd >> 1) * 2 * S + 2 * nh * i + nh * (xcd & 1) + half;
    if (order == 4) return (xcd >> 1) * 2 * S + 2 * l + (xcd & 1);
  }
  const int per = nb >> 3, rem = nb & 7;
  return nh * (xcd * per + (xcd < rem ? xcd : rem) + i) + half;
}

struct SsLayout {
  int P, N, tiles_per_phase;      // phases, nodes per phase, 64-node tiles per phase
  int NX, NO, NB;                 // states, output rows per node, Jacobian blocks per output row
  int off_nnz;                    // a phase's constant list (each tile writes off_nnz / tiles_per_phase of it, NX copies)
  int nnz_nl, nnz_lin;            // `values`: [P x NO x NB x N] [nnz_lin] [P x NX x off_nnz]
  long long sg, sv;               // instance strides of g and values, in doubles
  int n_inst;
};

template <int JP, int CP>
__global__ __launch_bounds__(768, 1) void k_sustained(const SsLayout Y, int order, double* __restrict__ gall,
                                                      double* __restrict__ vall) {
  constexpr int NH = 2, RG = 4, NDMA = 2, HT = 64 * (RG + NDMA);
  const int half = __builtin_amdgcn_readfirstlane(int(threadIdx.x) / HT);
  const int tid = int(threadIdx.x) - half * HT;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int nb = int(gridDim.x), G = NH * nb;
  const int nt = Y.P * Y.tiles_per_phase, W = nt * Y.n_inst;
  const int w = ss_slot(order, NH, nb, int(blockIdx.x), half), w0 = ss_slot(order, NH, nb, int(blockIdx.x), 0);
  const int n_iter = w < W ? (W - w + G - 1) / G : 0;
  const int n_iter_wg = w0 < W ? (W - w0 + G - 1) / G : 0;
  const int R = Y.NB;             // roles: 0 the g rows, 1 .. NB - 2 one block column each, NB - 1 the t0 and tf columns
  for (int j = 0; j < n_iter_wg; ++j) {
    if (wave >= RG) {
      __builtin_amdgcn_s_waitcnt(0);
      __syncthreads();
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    if (j >= n_iter) continue;
    const int item = w + j * G, inst = item / nt, tidx = item - inst * nt;
    const int ph = tidx / Y.tiles_per_phase, tp = tidx - ph * Y.tiles_per_phase;
    double* __restrict__ vals = vall + size_t(inst) * Y.sv;
    if (wave >= RG) {
      // constant share of this tile: off_nnz / tiles_per_phase doubles, NX copies off_nnz apart, 16 B per lane
      const int dw = wave - RG;
      const int share = Y.off_nnz / Y.tiles_per_phase;
      double* cdst = vals + Y.nnz_nl + Y.nnz_lin + size_t(ph) * Y.NX * Y.off_nnz + tp * share;
      const int head = int((16 - ((reinterpret_cast<size_t>(cdst) >> 3) & 15)) & 15);
      const d2u cv = {1.0 + lane, 2.0};
      for (int q = head + dw * 128 + 2 * lane; q + 1 < share; q += NDMA * 128)
        for (int i = 0; i < Y.NX; ++i) ss_store<CP>(reinterpret_cast<d2u*>(cdst + size_t(i) * Y.off_nnz + q), cv);
    } else {
      const int k = tp * 64 + lane;
      double* vb = vals + size_t(ph) * Y.NO * Y.NB * Y.N;
      for (int role = wave; role < R; role += RG) {
        if (role == 0) {
          double* g = gall + size_t(inst) * Y.sg + size_t(ph) * Y.NO * Y.N;
          for (int o = 0; o < Y.NO; ++o) g[size_t(o) * Y.N + k] = 1.0 + o;
        } else if (role < R - 1) {
          for (int o = 0; o < Y.NO; ++o) ss_store<JP>(vb + size_t(o * Y.NB + role - 1) * Y.N + k, 1.0 + o);
        } else {
          for (int o = 0; o < Y.NO; ++o) {
            ss_store<JP>(vb + size_t(o * Y.NB + R - 2) * Y.N + k, 1.0 + o);
            ss_store<JP>(vb + size_t(o * Y.NB + R - 1) * Y.N + k, 2.0 + o);
          }
        }
      }
    }
  }
}

// the same bytes as a linear fill: workgroup b writes 12 KB pieces b, b + nb, ... of the launch's `values` then g
__global__ __launch_bounds__(768, 1) void k_sustained_linear(d2u* __restrict__ out, size_t n16) {
  const d2u v = {1.0 + threadIdx.x, 2.0};
  for (size_t q = size_t(blockIdx.x) * 768 + threadIdx.x; q < n16; q += size_t(gridDim.x) * 768) out[q] = v;
}

extern "C" {
int ss_slot_host(int order, int nh, int nb, int b, int half) { return ss_slot(order, nh, nb, b, half); }

// bytes one launch stores (the heads and tails of the constant shares that the kernel writes as single stores are left out)
double ss_bytes(const SsLayout* Y) {
  const double share = Y->off_nnz / Y->tiles_per_phase;
  return 8.0 * Y->n_inst * Y->P * (double(Y->NO) * Y->N + double(Y->NO) * Y->NB * Y->N + Y->tiles_per_phase * share * Y->NX);
}

// jp, cp: store policy of the Jacobian and of the constant stream; order < 0: the linear reference.  Writes the time of each of
// `samples` timed regions of `per` launches, in us per launch, to us[]; buffers are cycled launch by launch.
int ss_run(const SsLayout* Y, int order, int jp, int cp, int grid, void** gs, void** vs, int nbuf, int per, int samples, float* us) {
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return 1;
  int r = 0;
  for (int s = -2; s < samples; ++s) {
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; i < per; ++i, ++r) {
      double* g = static_cast<double*>(gs[r % nbuf]);
      double* v = static_cast<double*>(vs[r % nbuf]);
      if (order < 0) {
        hipLaunchKernelGGL(k_sustained_linear, dim3(grid), dim3(768), 0, nullptr, reinterpret_cast<d2u*>(v), size_t(ss_bytes(Y) / 16));
        continue;
      }
#define SS_CASE(J, C) \
  if (jp == J && cp == C) hipLaunchKernelGGL((k_sustained<J, C>), dim3(grid), dim3(768), 0, nullptr, *Y, order, g, v)
      SS_CASE(0, 0); SS_CASE(0, 1); SS_CASE(0, 2); SS_CASE(0, 3);
      SS_CASE(1, 0); SS_CASE(1, 1); SS_CASE(1, 2); SS_CASE(1, 3);
      SS_CASE(2, 0); SS_CASE(2, 1); SS_CASE(2, 2); SS_CASE(2, 3);
#undef SS_CASE
    }
    (void)hipEventRecord(e1, nullptr);
    if (hipEventSynchronize(e1) != hipSuccess) return 2;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (s >= 0) us[s] = ms * 1e3f / per;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
}
