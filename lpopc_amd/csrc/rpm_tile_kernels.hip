// rpm_tile_kernels.hip — the constraint / Jacobian kernels for gfx950 (MI355X / CDNA4) and their launchers.
//
// Kernels (DESIGN.md §Kernels has the roofline of each):
//   tile kernels      K1+K2+K3 fused: per-node dynamics/path evaluation, forward-difference (or
//                     analytic) node Jacobian, LGR defect D.X - (dt/2) f, and the coalesced block
//                     scatter of the COO Jacobian values, plus the tile's share of the
//                     constant Doffdiag block.  Replace NLPWrapper::GetConsFun (LpNLPWrapper.cpp:55-229),
//                     GetPhaseJacbi (:524-862), LpFDderive::DerivDae (LpFiniteDifferenceDerive.cpp:194-324)
//                     and dsmatrix::operator* (SparseMatrix/LpSparseMatrix.cpp:127-155).  Three thread
//                     layouts of the same arithmetic, bit-identical results, chosen by launch size (cons_layout):
//     rpm_tile_kernel      one role per thread, tiles of <= T nodes: the shortest critical path
//     rpm_tile_rl_kernel   role-looped: 64 nodes x RG role groups, a wave is one role of 64 nodes
//     rpm_tile_pl_kernel   pipelined: the role loop made persistent, DMA waves stage the next tile
//   endpoint block    K4: events, linkages, A_lin.x rows and their Jacobian entries
//                     (LpNLPWrapper.cpp:125-136,180-211,406-522,833-861; :45,:242); one extra workgroup
//                     of the same launch, or (pipelined) one DMA wave.
//
// A workgroup (a half of one in the pipelined kernel) works on a tile of consecutive collocation nodes of one
// phase; the node is the fastest thread index, so that the N-long diagonal runs of every Jacobian
// block are written by consecutive lanes (coalesced 8-byte stores).  Role 0 evaluates the unperturbed
// dynamics, role 1+v the dynamics with variable v perturbed (v = states, controls, time, static parameters) —
// the reference's (2+nx+nu+nq) whole-vector user calls become (2+nx+nu+nq) roles.
// State roles also compute their state's D.X row from the LDS-staged D rows and X tile.
// What a role computes is written once, in the shared rules below the endpoint block (role_dynamics ...
// jacobian_blocks); a layout adds its thread layout, its loads, its synchronisation and how a value is stored.
#include "rpm_device_internal.hpp"

namespace rpm {


// ------------------------------------------------------------------------------------------
// The base values of an endpoint work item (the first n of lane 0's outputs val[NV]) to every lane, for the differences
// against the base: a lane shuffle where one wave does the item (WAVE), else LDS plus a workgroup barrier.
template <int NV, bool WAVE>
__device__ __forceinline__ void base_to_lanes(const double* val, int n, int lane, double* lds, double* base) {
  if constexpr (WAVE) {
#pragma unroll
    for (int i = 0; i < NV; ++i) base[i] = __shfl(val[i], 0, 64);
  } else {
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i)
        if (i < n) lds[i] = val[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) base[i] = lds[i];
  }
}

// endpoint rows: events, linkages, linear rows.  Each work item (TaskDev) is one workgroup of the same
// launch, so the three kinds run concurrently on different CUs.
// WAVE = true: the work item is done by ONE wave (lanes = perturbations, the base values travel by lane shuffle, no
// workgroup barrier), so a wave of a workgroup that is busy with something else can take it (rpm_tile_pl_kernel).
template <class Prob, bool WG, bool WJ, bool AN, bool WAVE = false>
__device__ void endpoint_block(const KParams& K, const TaskDev task, const double* __restrict__ x,
                               double* __restrict__ g, double* __restrict__ vals, double* lds, int inst) {
  constexpr int NX = Prob::NX, NQ = prob_nq<Prob>::value, NQs = NQ > 0 ? NQ : 1;
  bool bad_g = false, bad_j = false;
  constexpr int NE = Prob::NE_MAX > 0 ? Prob::NE_MAX : 1;
  constexpr int NL = Prob::NLINK_MAX > 0 ? Prob::NLINK_MAX : 1;
  static_assert(!WAVE || 2 * NX + 3 + 2 * NQ <= 64, "endpoint perturbations must fit one wave");
  const int tid = WAVE ? int(threadIdx.x & 63) : int(threadIdx.x);
  const int nthr = WAVE ? 64 : int(blockDim.x);
  const double* c = K.consts + size_t(inst) * K.consts_stride;
  if (task.type == 0) {
    // linear rows  A_lin * x  (LpNLPWrapper.cpp:45; COO loop order of LpSparseMatrix.cpp:142-153) and
    // their constant Jacobian entries (:242)
    for (int r = tid; r < K.P + K.L; r += nthr) {
      if (WG) {
        double acc = 0.0;
        acc += K.alin_v[2 * r] * x[K.alin_j[2 * r]];
        acc += K.alin_v[2 * r + 1] * x[K.alin_j[2 * r + 1]];
        g[K.m_nl + r] = acc;
        chk_note(bad_g, acc);
      }
      if (WJ) {
        vals[K.nnz_nl + 2 * r] = K.alin_v[2 * r];
        vals[K.nnz_nl + 2 * r + 1] = K.alin_v[2 * r + 1];
      }
    }
  } else if (task.type == 1) {
    // ---- events of one phase: lane 0 = base, lanes 1..2NX+2+NQ = perturbations [x0.., t0, xf.., tf, p..]
    //      (LpFDderive::DerivEvent, LpFiniteDifferenceDerive.cpp:326-409)
    const PhaseDev ph = K.phases[task.idx];
    const int pi = tid;
    const bool act = pi <= 2 * NX + 2 + NQ;
    double x0[NX], xf[NX], ev[NE], pp[NQs];
#pragma unroll
    for (int j = 0; j < NQ; ++j) pp[j] = x[ph.x_t0 + 2 + j];
    double t0 = x[ph.x_t0], tf = x[ph.x_t0 + 1];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      x0[j] = x[ph.x_state0 + j * (ph.N + 1)];
      xf[j] = x[ph.x_state0 + j * (ph.N + 1) + ph.N];
    }
    double h = 1.0;
    if (WJ && !AN && pi >= 1) {
      const int v = pi - 1;
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        if (v == j) { h = K.tol * (fabs(x0[j]) + 1); x0[j] += h; }
        if (v == NX + 1 + j) { h = K.tol * (fabs(xf[j]) + 1); xf[j] += h; }
      }
      if (v == NX) { h = K.tol * (1 + fabs(t0)); t0 += h; }
      if (v == 2 * NX + 1) { h = K.tol * (1 + fabs(tf)); tf += h; }
#pragma unroll
      for (int j = 0; j < NQ; ++j)
        if (v == 2 * NX + 2 + j) { h = K.tol * (1 + fabs(pp[j])); pp[j] += h; }
    }
#pragma unroll
    for (int i = 0; i < NE; ++i) ev[i] = 0.0;
    if (act && (pi == 0 || !AN)) pf_event<Prob>(ph.phase_num, t0, x0, tf, xf, pp, c, ev);
    if (WG && pi == 0) {
#pragma unroll
      for (int i = 0; i < NE; ++i)
        if (i < ph.ne) { g[ph.g0 + (NX + Prob::NC) * ph.N + i] = ev[i]; chk_note(bad_g, ev[i]); }
    }
    double base[NE];
    base_to_lanes<NE, WAVE>(ev, ph.ne, pi, lds, base);
    if (WJ && act && pi >= 1) {
      const int v = pi - 1;
      double de[NE];
      if constexpr (AN) {
        pf_event_jac_col<Prob>(ph.phase_num, v, t0, x0, tf, xf, pp, c, de);
      } else {
#pragma unroll
        for (int i = 0; i < NE; ++i) de[i] = (ev[i] - base[i]) / h;
      }
      // position inside an event's row of entries: (x0_j, xf_j) pairs, then t0, tf, then the parameters (:837-859)
      int pos;
      if (v < NX) pos = 2 * v;
      else if (v == NX) pos = 2 * NX;
      else if (v <= 2 * NX) pos = 2 * (v - NX - 1) + 1;
      else pos = v;   // tf at 2NX+1, parameter j at 2NX+2+j
#pragma unroll
      for (int i = 0; i < NE; ++i)
        if (i < ph.ne) { vals[ph.v_evt0 + i * (2 * NX + 2 + NQ) + pos] = de[i]; chk_note(bad_j, de[i]); }
    }
  } else {
    // ---- one linkage pair: lane 0 = base, then the perturbations [xf_left.., p_left.., x0_right.., p_right..]
    //      (LpFDderive::DerivLink, LpFiniteDifferenceDerive.cpp:411-502; each parameter by its own step and the right phase's
    //      parameters from the right phase — the reference hands the left ones twice, SURVEY B-9)
    const LinkDev lk = K.links[task.idx];
    const PhaseDev pl = K.phases[lk.left];
    const PhaseDev pr = K.phases[lk.right];
    const int pi = tid;
    const bool act = pi <= 2 * NX + 2 * NQ;
    double xl[NX], xr[NX], lo[NL], ql[NQs], qr[NQs];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      ql[j] = x[pl.x_t0 + 2 + j];
      qr[j] = x[pr.x_t0 + 2 + j];
    }
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      xl[j] = x[pl.x_state0 + j * (pl.N + 1) + pl.N];
      xr[j] = x[pr.x_state0 + j * (pr.N + 1)];
    }
    double h = 1.0;
    if (WJ && !AN && pi >= 1) {
      const int v = pi - 1;
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        if (v == j) { h = K.tol * (1 + fabs(xl[j])); xl[j] += h; }
        if (v == NX + NQ + j) { h = K.tol * (1 + fabs(xr[j])); xr[j] += h; }
      }
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        if (v == NX + j) { h = K.tol * (1 + fabs(ql[j])); ql[j] += h; }
        if (v == 2 * NX + NQ + j) { h = K.tol * (1 + fabs(qr[j])); qr[j] += h; }
      }
    }
#pragma unroll
    for (int i = 0; i < NL; ++i) lo[i] = 0.0;
    if (act && (pi == 0 || !AN)) pf_link<Prob>(lk.left + 1, lk.right + 1, xl, xr, ql, qr, c, lk.nlink, lo);
    if (WG && pi == 0) {
#pragma unroll
      for (int i = 0; i < NL; ++i)
        if (i < lk.nlink) { g[lk.g0 + i] = lo[i]; chk_note(bad_g, lo[i]); }
    }
    double base[NL];
    base_to_lanes<NL, WAVE>(lo, lk.nlink, pi, lds, base);
    if (WJ && act && pi >= 1) {
      const int v = pi - 1;
      double dl[NL];
      if constexpr (AN) {
        pf_link_jac_col<Prob>(lk.left + 1, lk.right + 1, v, xl, xr, ql, qr, c, lk.nlink, dl);
      } else {
#pragma unroll
        for (int i = 0; i < NL; ++i) dl[i] = (lo[i] - base[i]) / (1.0 * h);
      }
#pragma unroll
      for (int i = 0; i < NL; ++i)
        if (i < lk.nlink) { vals[lk.v0 + v * lk.nlink + i] = dl[i]; chk_note(bad_j, dl[i]); }  // column-major, :461-501
    }
  }
  chk_report(K.chk, bad_g, bad_j);
}

// ------------------------------------------------------------------------------------------
// The per-node role arithmetic of the three tile layouts (rpm_tile_kernel, rpm_tile_rl_kernel, rpm_tile_pl_kernel).  One
// copy, so that the layouts stay bit-identical: the dynamics (role_dynamics), the perturbation (perturb_uniform), the published
// base (publish_base), the defect (store_defect) and what becomes of a role's outputs (jacobian_blocks; the pipelined kernel
// restates it, see there); stage_tile_inputs is the LDS staging of the two kernels without DMA waves.  Each layout keeps its
// own thread layout, loads of the node's point, D.X sum, synchronisation, constant-block stores and the one expression that
// stores a Jacobian value (the lambda it hands to jacobian_blocks).  A thread works on node k of its tile (lane kk of the
// [..][T] LDS rows) for one role: role 0 is the unperturbed dynamics, role 1 + v the dynamics with variable
// v = [states, controls, time, static parameters] perturbed.
// CHK: the one-role kernel notes NaN/Inf among the values it stores (host-pointer path); the others pass false.

// The dynamics of a role at (tk, xs, us = [controls, static parameters]): f and c, or with AN column v of the node
// Jacobian for roles >= 1.  STG (has_stage functors): from the sub-expressions of the node's unperturbed point, recomputing
// only what the perturbed variable enters (same operations, same bits as the whole dae()).
template <class Prob, bool WJ, bool AN, bool STG = false, class CP>
__device__ __forceinline__ void role_dynamics(int phase_num, int role, double tk, const double* xs, const double* us, CP c,
                                              double* f, double* cp,
                                              const typename stage_of<Prob>::type* base_stage = nullptr) {
  const int v = role - 1;
  if constexpr (STG) {
    Prob::dae_from(phase_num, tk, xs, us, c, *base_stage, (WJ && role >= 1) ? v : -1, f, cp);
  } else if (!AN || role == 0) {
    pf_dae<Prob>(phase_num, tk, xs, us, us + Prob::NU, c, f, cp);
  } else if constexpr (AN) {
    pf_dae_jac_col<Prob>(phase_num, v, tk, xs, us, us + Prob::NU, c, f, cp);  // f, cp now hold column v of the Jacobian
  }
}

// The one-role and the role-looped kernel stage a tile's X rows, U rows and (WG) D rows in LDS with all nthr threads
// (coalesced: every run is contiguous in HBM); the caller's barrier follows.  The pipelined kernel's DMA waves copy the same
// runs straight into LDS instead (`stage` there).  (x without __restrict__: with it one role-looped instantiation takes 4
// more VGPRs and loses a wave of occupancy.)
template <int NX, int NU, int T, bool WG>
__device__ __forceinline__ void stage_tile_inputs(const KParams& K, const TileDev& tl, const double* x, int tid, int nthr,
                                                  double* Xs, double* Us, double* Ds) {
  for (int q = tid; q < NX * tl.span_len; q += nthr) {
    const int i = q / tl.span_len, r = q - i * tl.span_len;
    Xs[i * K.max_span + r] = x[tl.x_state0 + i * (tl.N + 1) + tl.span0 + r];
  }
  for (int q = tid; q < NU * tl.cnt; q += nthr) {
    const int j = q / tl.cnt, r = q - j * tl.cnt;
    Us[j * T + r] = x[tl.x_control0 + j * tl.N + tl.k0 + r];
  }
  if (WG)
    for (int q = tid; q < tl.drow_len; q += nthr) Ds[q] = K.dvals[tl.drow0 + q];
}

// Finite-difference step of a wave-uniform role: h = tol (1+|v|), v+h  (LpFiniteDifferenceDerive.cpp:208-214).  The caller
// fetches the one perturbed variable pv by its (scalar) row; h and pv + h are formed once and the sum is put back where the
// variable belongs — instead of forming them for every variable and selecting.  Returns h.
template <int NX, int NU, int NQ>
__device__ __forceinline__ double perturb_uniform(int v, double pv, double tol, double* xs, double* us, double& tk) {
  const double h = tol * (1 + fabs(pv));
  const double pp = pv + h;
#pragma unroll
  for (int i = 0; i < NX; ++i) xs[i] = (v == i) ? pp : xs[i];
#pragma unroll
  for (int j = 0; j < NU; ++j) us[j] = (v == NX + j) ? pp : us[j];
  tk = (v == NX + NU) ? pp : tk;
#pragma unroll
  for (int j = 0; j < NQ; ++j) us[NU + j] = (v == NX + NU + 1 + j) ? pp : us[NU + j];
  return h;
}

// Role 0 publishes the unperturbed outputs: f and c into Fb ([NO][T]) for the other roles' differences, and c into the path
// rows of g (LpNLPWrapper.cpp:138-164).
template <class Prob, int T, bool WG, bool CHK>
__device__ __forceinline__ void publish_base(const double* f, const double* cp, double* Fb, int kk, double* g, int g0, int N,
                                             int k, bool& bad_g) {
  constexpr int NX = Prob::NX, NC = Prob::NC;
#pragma unroll
  for (int i = 0; i < NX; ++i) Fb[i * T + kk] = f[i];
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    Fb[(NX + j) * T + kk] = cp[j];
    if (WG) {
      g[g0 + (NX + j) * N + k] = cp[j];
      if (CHK) chk_note(bad_g, cp[j]);
    }
  }
}

// The defect of state sv at node k: D.X - (dt/2) f  (LpNLPWrapper.cpp:113,122).
template <int T, bool CHK>
__device__ __forceinline__ void store_defect(int sv, double dx, double tspan, const double* Fb, int kk, double* g, int g0,
                                             int N, int k, bool& bad_g) {
  const double dfc = dx - Fb[sv * T + kk] * (tspan / 2.0);
  g[g0 + sv * N + k] = dfc;
  if (CHK) chk_note(bad_g, dfc);
}

// What becomes of the outputs f, cp of role 1 + v at node k: the column J = (perturbed - unperturbed) / h of the node Jacobian
// (AN: f, cp already hold it) and from it this role's entry of every Jacobian block, handed to store(blk, val) with
// blk = o * NB + column block for output row o — the caller's store puts it at values[v_nl0 + blk * N + k].
//   v != time: blocks d/dx_v, d/du_v or d/dp_j of every output row (:698-743, :763-769, :776-796, :814-820), Ddiag - ret on
//     the diagonal block (:712); the parameter blocks follow the two time blocks and take their derivative column, not the
//     time column — SURVEY B-6, B-7
//   v == time: the d/dt0 and d/dtf blocks (:748-760, :801-811); B-5 sign of the reference kept
template <class Prob, int T, bool AN, class Store>
__device__ __forceinline__ void jacobian_blocks(int v, double h, const double* f, const double* cp, const double* Fb, int kk,
                                                double tau, double t0, double tf, double ddiag, Store store) {
  constexpr int NX = Prob::NX, NU = Prob::NU, NC = Prob::NC, NQ = prob_nq<Prob>::value;
  constexpr int NO = NX + NC;              // outputs per node: f then c
  constexpr int NB = NX + NU + 2 + NQ;     // Jacobian blocks per output row: x.., u.., t0, tf, p..
  double J[NO];
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    const double pert = o < NX ? f[o < NX ? o : 0] : cp[o >= NX ? o - NX : 0];
    J[o] = AN ? pert : (pert - Fb[o * T + kk]) / h;
  }
  if (v != NX + NU) {
    const int bv = v < NX + NU ? v : v + 1;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      double val;
      if (o < NX) {
        const double ret = J[o] * (tf - t0) / 2.0;
        val = (o == v) ? ddiag - ret : -ret;
      } else {
        val = J[o];
      }
      store(o * NB + bv, val);
    }
  } else {
    const double a0 = -(tau * 0.5) + 0.5, af = (tau * 0.5) + 0.5;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      double v0, vf;
      if (o < NX) {
        const double fb = Fb[o * T + kk];
        const double dt = J[o] * (tf - t0) / 2.0;
        v0 = fb * (0.5) - a0 * dt;
        vf = -fb * (0.5) + af * dt;
      } else {
        v0 = a0 * J[o];
        vf = af * J[o];
      }
      store(o * NB + NX + NU, v0);
      store(o * NB + NX + NU + 1, vf);
    }
  }
}

// (xcd_place, the XCD-aware order of the workgroups of all three kernels: rpm_device_internal.hpp)

// a wave-uniform field of a tile record staged as ints (in LDS or in the constant address space)
#define RPM_REC(rec, f) __builtin_amdgcn_readfirstlane((rec)[offsetof(TileDev, f) / 4])

// ------------------------------------------------------------------------------------------
template <class Prob, int T, bool WG, bool WJ, bool AN, bool DXM = false>
__global__ void rpm_tile_kernel(const KParams K, const double* __restrict__ xall,
                                double* __restrict__ gall, double* __restrict__ vall) {
  constexpr int NX = Prob::NX, NU = Prob::NU, NC = Prob::NC, NQ = prob_nq<Prob>::value;
  constexpr int NV = NX + NU + 1 + NQ;     // perturbation variables: states, controls, time, static parameters
  constexpr int R = WJ ? NV + 1 : (NX > 0 ? NX : 1);
  constexpr int NCs = NC > 0 ? NC : 1;
  extern __shared__ double lds[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const double* __restrict__ x = xall + size_t(blockIdx.y) * K.n;
  double* __restrict__ g = gall + size_t(blockIdx.y) * K.sg;
  double* __restrict__ vals = vall + size_t(blockIdx.y) * K.sv;
  if (int(blockIdx.x) >= K.n_my_tiles) {  // the launch's trailing workgroups: endpoint work items
    endpoint_block<Prob, WG, WJ, AN>(K, K.tasks[int(blockIdx.x) - K.n_my_tiles], x, g, vals, lds, int(blockIdx.y));
    return;
  }
  const TileDev tl = K.tiles[xcd_place(int(blockIdx.x), K.n_my_tiles)];
  const TileDev& ph = tl;   // the phase fields the kernel needs are replicated in the tile record
  const auto c = (const __attribute__((address_space(4))) double*)(K.consts + size_t(blockIdx.y) * K.consts_stride);   // constant address space: scalar loads
  const TileLds L(NX, NU, NC, T, K.max_span, K.max_drow);
  double *Xs = lds + L.Xs, *Us = lds + L.Us, *Ds = lds + L.Ds, *Fb = lds + L.Fb, *DXs = lds + L.DXs;

  // ---- issue the loads nothing depends on first: this thread's node record and its share of the
  //      constant-block sources (stored at the very end) ----
  const int kk = tid % T, role = tid / T;
  bool bad_g = false, bad_j = false;              // NaN/Inf among the values this thread stores (host-pointer path)
  const int kc = kk < tl.cnt ? kk : tl.cnt - 1;   // clamp so idle lanes read valid memory
  const int k = tl.k0 + kc;
  const int nidx = ph.node0 + k;
  const double tau = K.points[nidx];
  const NodeDev nd = K.nodes[nidx];
  const double ddiag = WJ ? K.diag[nidx] : 0.0;
  constexpr int CPRE = 8;                          // constant-block sources prefetched per thread
  double cpre[CPRE > 0 ? CPRE : 1];
  if (WJ && !K.skip_const) {
#pragma unroll
    for (int u = 0; u < CPRE; ++u) {
      const int q = tid + u * nthr;
      cpre[u] = q < tl.c_cnt ? K.doff_vals[tl.c_src0 + q] : 0.0;
    }
  }

  stage_tile_inputs<NX, NU, T, WG>(K, tl, x, tid, nthr, Xs, Us, Ds);
  const double t0 = x[ph.x_t0], tf = x[ph.x_t0 + 1];
  __syncthreads();

  const bool act = kk < tl.cnt && role < R;
  const double tspan = tf - t0;
  double tk = (tau + 1) * (tspan / 2.0) + t0;      // LpNLPWrapper.cpp:80
  double xs[NX > 0 ? NX : 1], us[NU + NQ > 0 ? NU + NQ : 1];   // us = [controls, static parameters]
#pragma unroll
  for (int i = 0; i < NX; ++i) xs[i] = Xs[i * K.max_span + (k - tl.span0)];
#pragma unroll
  for (int j = 0; j < NU; ++j) us[j] = Us[j * T + kc];
#pragma unroll
  for (int j = 0; j < NQ; ++j) us[NU + j] = x[ph.x_t0 + 2 + j];

  // ---- D.X for this thread's state: ascending-column sum, separate multiply and add, exactly the
  //      order of the reference's COO loop for one output row (LpSparseMatrix.cpp:142-153) ----
  const int sv = WJ ? role - 1 : role;
  double dx = 0.0;
  if (WG && !DXM && sv >= 0 && sv < NX) {
    const double* drow = Ds + (nd.drow_off - tl.drow0);
    const double* xcol = Xs + sv * K.max_span + (nd.dcol0 - tl.span0);
    for (int j = 0; j < nd.dlen; ++j) dx += drow[j] * xcol[j];
  }
  // ---- MFMA variant (dx_mode = 1): the tile's D.X as dense 16x16x4 FP64 matrix-core products.  The tile's D
  //      rows form a block-banded (cnt x span_len) matrix A (zero outside each row's interval), B = the staged X
  //      rows (span_len x nx); wave 0 accumulates ceil(span_len/4) v_mfma_f64_16x16x4_f64 per 16 rows x 16 states.
  //      Operand maps (cdna_hip_programming.md §3): A: lane l holds A[l&15][l>>4], B: B[l>>4][l&15],
  //      C/D: col = l&15, row = (l>>4) + 4*reg.  The k-order of the sum differs from the reference's ascending
  //      column loop, so results agree to rounding (~1e-16 relative), not bit for bit. ----
  if constexpr (DXM && WG) {
    if (tid < 64) {
      typedef double d4 __attribute__((ext_vector_type(4)));
      const int lr = tid & 15, kq = tid >> 4;
      const int ksteps = (tl.span_len + 3) >> 2;
      for (int rb = 0; rb < T; rb += 16) {
        const int row = rb + lr;
        const bool row_ok = row < tl.cnt;
        const NodeDev ndr = K.nodes[ph.node0 + tl.k0 + (row_ok ? row : tl.cnt - 1)];
        const int rel0 = ndr.dcol0 - tl.span0;
        const double* drow = Ds + (ndr.drow_off - tl.drow0);
        for (int cb = 0; cb < NX; cb += 16) {
          const int st = cb + lr;
          d4 acc = {0.0, 0.0, 0.0, 0.0};
          for (int s = 0; s < ksteps; ++s) {
            const int kcol = 4 * s + kq;
            const int rel = kcol - rel0;
            const double a = (row_ok && rel >= 0 && rel < ndr.dlen) ? drow[rel] : 0.0;
            const double b = (st < NX && kcol < tl.span_len) ? Xs[st * K.max_span + kcol] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int orow = rb + kq + 4 * i;
            if (st < NX && orow < tl.cnt) DXs[st * T + orow] = acc[i];
          }
        }
      }
    }
  }

  // ---- perturb this role's variable (the step of perturb_uniform; the role is not wave-uniform here: formed for every
  //      variable and selected) ----
  double h = 1.0;
  const int v = role - 1;
  if (WJ && !AN && role >= 1) {
#pragma unroll
    for (int i = 0; i < NX; ++i)
      if (v == i) { h = K.tol * (1 + fabs(xs[i])); xs[i] += h; }
#pragma unroll
    for (int j = 0; j < NU; ++j)
      if (v == NX + j) { h = K.tol * (1 + fabs(us[j])); us[j] += h; }
    if (v == NX + NU) { h = K.tol * (1 + fabs(tk)); tk += h; }
#pragma unroll
    for (int j = 0; j < NQ; ++j)
      if (v == NX + NU + 1 + j) { h = K.tol * (1 + fabs(us[NU + j])); us[NU + j] += h; }
  }
  double f[NX > 0 ? NX : 1], cp[NCs];
  role_dynamics<Prob, WJ, AN>(ph.phase_num, role, tk, xs, us, c, f, cp);
  if (role == 0 && act) publish_base<Prob, T, WG, true>(f, cp, Fb, kk, g, ph.g0, ph.N, k, bad_g);
  __syncthreads();

  if (act) {
    const int N = ph.N;
    if (WG && sv >= 0 && sv < NX) store_defect<T, true>(sv, DXM ? DXs[sv * T + kk] : dx, tspan, Fb, kk, g, ph.g0, N, k, bad_g);
    if (WJ && role >= 1) {
      double* vb = vals + ph.v_nl0 + k;
      jacobian_blocks<Prob, T, AN>(v, h, f, cp, Fb, kk, tau, t0, tf, ddiag, [&](int blk, double val) {
        vb[size_t(blk) * N] = val;
        chk_note(bad_j, val);
      });
    }
  }
  chk_report(K.chk, bad_g, bad_j);

  // ---- this workgroup's share of the constant Doffdiag block (LpNLPWrapper.cpp:715-718): the block is
  //      nx back-to-back copies of the phase's off-diagonal value list; read each source value once,
  //      store it into every state's copy (all runs contiguous across lanes) ----
  if (WJ && !K.skip_const) {
    const double* __restrict__ src = K.doff_vals + tl.c_src0;
    double* __restrict__ dst = vals + tl.c_dst0;
#pragma unroll
    for (int u = 0; u < CPRE; ++u) {
      const int q = tid + u * nthr;
      if (q < tl.c_cnt) {
#pragma unroll
        for (int i = 0; i < NX; ++i) dst[size_t(i) * tl.c_stride + q] = cpre[u];
      }
    }
    for (int q = tid + CPRE * nthr; q < tl.c_cnt; q += nthr) {
      const double dv = src[q];
#pragma unroll
      for (int i = 0; i < NX; ++i) dst[size_t(i) * tl.c_stride + q] = dv;
    }
  }
}

// ------------------------------------------------------------------------------------------
// rpm_tile_rl_kernel ("role-looped"): the throughput variant for large grids (many instances per launch).
// Same arithmetic and the same output order as rpm_tile_kernel, different thread layout: a workgroup is T nodes x RG
// role GROUPS, and each thread walks the roles g, g+RG, g+2RG, ... of its node one after another.  With T = 64,
// RG = 4 a wave is 64 consecutive nodes of ONE role, so every Jacobian store instruction writes 512 contiguous bytes
// (instead of 4 x 128 B), a launch has 4x fewer workgroups of 4 waves each (one residency round on 256 CUs at 16
// instances of the metric problem), and each workgroup pays its load chain once for 3 dynamics evaluations per thread.
#ifdef RPM_DIAG
#define RPM_TRC(i)                                                                                            \
  if (K.trace && threadIdx.x == 0)                                                                            \
  K.trace[(size_t(blockIdx.y) * gridDim.x + blockIdx.x) * 8 + (i)] = wall_clock64()
#else
#define RPM_TRC(i)
#endif
template <class Prob, int T, int RG, bool WG, bool WJ, bool AN>
__global__ __launch_bounds__(T* RG) void rpm_tile_rl_kernel(const KParams K, const double* __restrict__ xall,
                                                            double* __restrict__ gall, double* __restrict__ vall) {
  constexpr int NX = Prob::NX, NU = Prob::NU, NC = Prob::NC, NQ = prob_nq<Prob>::value;
  constexpr int NV = NX + NU + 1 + NQ;
  constexpr int R = WJ ? NV + 1 : (NX > 0 ? NX : 1);
  constexpr int NCs = NC > 0 ? NC : 1;
  constexpr int NTHR = T * RG;
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const double* __restrict__ x = xall + size_t(blockIdx.y) * K.n;
  double* __restrict__ g = gall + size_t(blockIdx.y) * K.sg;
  double* __restrict__ vals = vall + size_t(blockIdx.y) * K.sv;
  RPM_TRC(0);
  if (int(blockIdx.x) >= K.n_my_tiles) {
    endpoint_block<Prob, WG, WJ, AN>(K, K.tasks[int(blockIdx.x) - K.n_my_tiles], x, g, vals, lds, int(blockIdx.y));
    return;
  }
  const TileDev tl = K.tiles[xcd_place(int(blockIdx.x), K.n_my_tiles)];
  const TileDev& ph = tl;
  const auto c = (const __attribute__((address_space(4))) double*)(K.consts + size_t(blockIdx.y) * K.consts_stride);   // constant address space: scalar loads
  const TileLds L(NX, NU, NC, T, K.max_span, K.max_drow);
  double *Xs = lds + L.Xs, *Us = lds + L.Us, *Ds = lds + L.Ds, *Fb = lds + L.Fb;
  const int kk = tid % T, grp = __builtin_amdgcn_readfirstlane(tid / T);   // a wave is one role group: roles are wave-uniform (scalar branches, scalar block offsets)
  const int kc = kk < tl.cnt ? kk : tl.cnt - 1;
  const int k = tl.k0 + kc;
  const int nidx = ph.node0 + k;
  const double tau = K.points[nidx];
  const NodeDev nd = K.nodes[nidx];
  const double ddiag = WJ ? K.diag[nidx] : 0.0;
  stage_tile_inputs<NX, NU, T, WG>(K, tl, x, tid, NTHR, Xs, Us, Ds);
  const double t0 = x[ph.x_t0], tf = x[ph.x_t0 + 1];
  RPM_TRC(1);
  __syncthreads();
  RPM_TRC(2);

  const bool node_ok = kk < tl.cnt;
  const double tspan = tf - t0;
  const double tk0 = (tau + 1) * (tspan / 2.0) + t0;      // LpNLPWrapper.cpp:80
  const int N = ph.N;
  bool first = true, no_chk = false;   // no_chk: the NaN/Inf bookkeeping is the one-role kernel's (CHK = false)
  for (int role = grp; role < R || first; role += RG) {
    const bool act = node_ok && role < R;
    double xs[NX > 0 ? NX : 1], us[NU + NQ > 0 ? NU + NQ : 1];   // us = [controls, static parameters]
#pragma unroll
    for (int i = 0; i < NX; ++i) xs[i] = Xs[i * K.max_span + (k - tl.span0)];
#pragma unroll
    for (int j = 0; j < NU; ++j) us[j] = Us[j * T + kc];
#pragma unroll
    for (int j = 0; j < NQ; ++j) us[NU + j] = x[ph.x_t0 + 2 + j];
    double tk = tk0;
    const int sv = WJ ? role - 1 : role;
    double dx = 0.0;
    if (WG && sv >= 0 && sv < NX) {   // D.X in the reference's ascending-column order (LpSparseMatrix.cpp:142-153)
      const double* drow = Ds + (nd.drow_off - tl.drow0);
      const double* xcol = Xs + sv * K.max_span + (nd.dcol0 - tl.span0);
      for (int j = 0; j < nd.dlen; ++j) dx += drow[j] * xcol[j];
    }
    double h = 1.0;
    const int v = role - 1;
    if (WJ && !AN && role >= 1) {   // the role is wave-uniform: fetch the one perturbed variable by its (scalar) row
      double pv;
      if (v < NX) pv = Xs[v * K.max_span + (k - tl.span0)];
      else if (v < NX + NU) pv = Us[(v - NX) * T + kc];
      else if (v == NX + NU) pv = tk;
      else pv = x[ph.x_t0 + 1 + (v - NX - NU)];   // static parameter v - NX - NU - 1
      h = perturb_uniform<NX, NU, NQ>(v, pv, K.tol, xs, us, tk);
    }
    double f[NX > 0 ? NX : 1], cp[NCs];
    role_dynamics<Prob, WJ, AN>(ph.phase_num, role, tk, xs, us, c, f, cp);
    if (first) {   // wave-uniform: the first pass publishes the unperturbed outputs before anyone forms a difference
      if (role == 0 && act) publish_base<Prob, T, WG, false>(f, cp, Fb, kk, g, ph.g0, N, k, no_chk);
      __syncthreads();
      RPM_TRC(3);
      first = false;
    }
    if (act) {
      if (WG && sv >= 0 && sv < NX) store_defect<T, false>(sv, dx, tspan, Fb, kk, g, ph.g0, N, k, no_chk);
      if (WJ && role >= 1) {
        double* vb = vals + ph.v_nl0 + k;
        jacobian_blocks<Prob, T, AN>(v, h, f, cp, Fb, kk, tau, t0, tf, ddiag,
                                     [&](int blk, double val) { vb[size_t(blk) * N] = val; });
      }
    }
  }
  RPM_TRC(4);
  if (WJ && !K.skip_const) {
    // this tile's share of the constant Doffdiag block (LpNLPWrapper.cpp:715-718)
    const double* __restrict__ src = K.doff_vals + tl.c_src0;
    double* __restrict__ dst = vals + tl.c_dst0;
    // lane 0 of every wave lands on a 128-byte line of the destination (a run that straddles lines costs the HBM write
    // path a third of its rate, tools/ubench/store_pattern.py): the index range is shifted down by the distance of
    // dst from the line boundary below it
    const int lead = int((reinterpret_cast<size_t>(dst) >> 3) & 15);
    for (int q = tid - lead; q < tl.c_cnt; q += NTHR) {
      if (q >= 0) {
        const double dv = src[q];
#pragma unroll
        for (int i = 0; i < NX; ++i) dst[size_t(i) * tl.c_stride + q] = dv;
      }
    }
  }
#ifdef RPM_DIAG
  RPM_TRC(5);
  if (K.trace) {
    __builtin_amdgcn_s_waitcnt(0);
    RPM_TRC(6);
    if (threadIdx.x == 0) {
      unsigned hw;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      unsigned xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      K.trace[(size_t(blockIdx.y) * gridDim.x + blockIdx.x) * 8 + 7] = (static_cast<unsigned long long>(xcc) << 32) | hw;
    }
  }
#endif
}

// ------------------------------------------------------------------------------------------
// rpm_tile_pl_kernel ("pipelined"): the role-looped layout made persistent and wave-specialised.  Why: the per-
// workgroup timeline of rpm_tile_rl_kernel is serial (input loads 4-5 us behind the store traffic, 3 dynamics passes,
// then a 2.5 us burst of constant-block stores that blocks the issuing waves), every workgroup of a launch is in the
// same phase at the same time, and a launch is only two residency rounds, so neither the SIMDs (busy 35 %) nor HBM
// (busy 45 %) are kept fed (tools/trace_timeline.py).  Here a workgroup is NH independent halves of RG compute waves +
// NDMA DMA waves (pl_shape), and a half walks tiles w, w+G, w+2G, ...:
//   * the DMA waves copy the NEXT tile's inputs (tile record, t0 tf, X rows, U rows, D rows, node records, its slice
//     of the constant list) from HBM straight into the other LDS staging buffer (global_load_lds_dwordx4) while the
//     compute waves work on the current one, and write the current tile's share of the constant Doffdiag block, so
//     the compute waves never wait for a load or a store burst; they run at raised priority (s_setprio);
//   * the compute waves run exactly the role loop of rpm_tile_rl_kernel (same arithmetic, same output order:
//     bit-identical results, tests/test_gpu_parity.py) out of the staged buffer;
//   * endpoint work items (events, linkages, linear rows) are taken by DMA waves once their tiles are done, one wave
//     each (endpoint_block<..., WAVE = true>).
// One workgroup barrier per tile (A: staging buffer ready; the DMA waves execute s_waitcnt vmcnt(0) before it); F
// (unperturbed dynamics published) is a flag in LDS that only the compute waves look at, so the DMA waves spend the
// first pass — when the compute waves store nothing — on the constant block.  Host-checked limits: a tile's constant
// share <= PL_CMAX doubles (it passes through registers of the DMA waves), 2 NX + 3 <= 64 (endpoint perturbations
// fit one wave).
constexpr int PL_CMAX = 1280, PL_REC = 32;   // a tile's constant share: at most PL_CMAX doubles
static_assert(sizeof(TileDev) / sizeof(int) < PL_REC, "tile record plus the instance index must fit the staged record");
static_assert(sizeof(TileDev) % 8 == 0, "the tile record is copied as doubles");

// Dynamic LDS of rpm_tile_pl_kernel, offsets in doubles (a tile is 64 nodes).  A half of a workgroup owns one block of
// `half` doubles: two staging buffers of `stage` doubles each, then Fb, the two ready words and (dx_mode 1) DXs.  The kernel
// carves its arrays by it; the host sizes the launch by pl_shape().NH x half.
struct PlLds {
  // one staging buffer: record (TileDev, then the instance index), record of the half's tile after this one (PL_REC ints each)
  // | t0 tf p.. (even count) | X [nx][max_span] | U [nu][64] | D rows (max_drow) | tau [64] | diag of D [64] | node records
  // [64] | share of the constant list (max_cshare; launches with a Jacobian); `stage` is its size
  int rec, next, tt, X, U, D, tau, diag, nodes, cv, stage;
  // a half's block: 2 staging buffers | Fb [nx + nc][64] | fb_ready, dx_ready (ints) | dx_mode 1: DXs [nx][64]; `half` is its size
  int Fb, ready, DXs, half;
  __host__ __device__ constexpr PlLds(int nx, int nu, int nc, int nq, int max_span, int max_drow, int max_cshare, bool with_jac,
                                      bool dxm)
      : rec(0), next(PL_REC / 2), tt(PL_REC), X(tt + 2 + ((nq + 1) & ~1)), U(X + nx * max_span), D(U + nu * 64),
        tau(D + max_drow), diag(tau + 64), nodes(diag + 64), cv(nodes + 2 * 64), stage(cv + (with_jac ? max_cshare : 0)),
        Fb(2 * stage), ready(Fb + (nx + nc) * 64), DXs(ready + 2), half(DXs + (dxm ? nx * 64 : 0)) {}
};
// pins: every array starts where the one before it ends, and the two sizes are the formulas the launches have always been
// sized by
constexpr bool pl_lds_pinned(int nx, int nu, int nc, int nq, int span, int drow, int cshare, bool wj, bool dxm) {
  const PlLds L(nx, nu, nc, nq, span, drow, cshare, wj, dxm);
  const int nqe = (nq + 1) & ~1;
  return L.rec == 0 && L.next == L.rec + PL_REC / 2 && L.tt == L.next + PL_REC / 2 && L.X == L.tt + 2 + nqe &&
         L.U == L.X + nx * span && L.D == L.U + nu * 64 && L.tau == L.D + drow && L.diag == L.tau + 64 &&
         L.nodes == L.diag + 64 && L.cv == L.nodes + 2 * 64 && L.stage == L.cv + (wj ? cshare : 0) && L.Fb == 2 * L.stage &&
         L.ready == L.Fb + (nx + nc) * 64 && L.DXs == L.ready + 2 && L.half == L.DXs + (dxm ? nx * 64 : 0) &&
         L.stage == PL_REC + 2 + nqe + nx * span + nu * 64 + drow + 4 * 64 + (wj ? cshare : 0) &&
         L.half == 2 * L.stage + (nx + nc) * 64 + 2 + (dxm ? nx * 64 : 0);
}
static_assert(pl_lds_pinned(LaunchProblem::NX, LaunchProblem::NU, LaunchProblem::NC, 0, 73, 64 * 9, 1024, true, false) &&   // odd span: U on an odd double
                  pl_lds_pinned(LaunchProblem::NX, LaunchProblem::NU, LaunchProblem::NC, 1, 80, 64 * 17, 1280, true, true) &&
                  pl_lds_pinned(QuadrotorProblem::NX, QuadrotorProblem::NU, QuadrotorProblem::NC, 0, 65, 64 * 65, 640, false, true),
              "PlLds: an array overlaps its neighbour or a size changed");
typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));   // a pair of doubles at 8-byte alignment
#define RPM_GPTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define RPM_LPTR(p) ((__attribute__((address_space(3))) void*)(p))
// One wave copies `len` doubles from global memory straight into LDS (both sides 8-byte aligned).  Inlined (a call
// would start with s_waitcnt 0 and serialise the loads) but not unrolled: the DMA wave runs this code once per tile,
// so it should be small enough to stay in the instruction cache.
template <int NPART>
__device__ __forceinline__ void pl_dma_run(const double* gsrc, double* ldst, int len, int lane, int part) {
  const int pairs = len >> 1;   // chunk ch (64 pairs) is copied by the wave with part == ch % NPART
#pragma unroll 1
  for (int ch = part; ch * 64 < pairs; ch += NPART)
    if (ch * 64 + lane < pairs)
      __builtin_amdgcn_global_load_lds(RPM_GPTR(gsrc + ch * 128 + 2 * lane), RPM_LPTR(ldst + ch * 128), 16, 0, 0);
  if ((len & 1) && part == 0 && lane < 2)   // odd tail: the last double as two dwords
    __builtin_amdgcn_global_load_lds(RPM_GPTR(reinterpret_cast<const int*>(gsrc + len - 1) + lane),
                                     RPM_LPTR(ldst + len - 1), 4, 0, 0);
}


// The two bulk output streams of the pipelined kernel go through pl_store<POLICY>: plain, non-temporal, or write-through +
// non-temporal (global_store_dwordx4 ... sc1 nt: the line is not kept in the XCD's L2).  Nobody in the launch reads these
// addresses, so the policy changes when the bytes leave L2 and nothing else.  Vector stores only.  The write-through form is
// inline asm, which hipcc neither counts in its s_waitcnt bookkeeping (the DMA waves wait vmcnt(0) in front of every
// barrier A themselves, and nothing reads the data) nor pads: s_nop 1 keeps the next instruction off the data registers
// until the store has read them.
constexpr int PL_ST_PLAIN = 0, PL_ST_NT = 1, PL_ST_WT_NT = 2;
constexpr int pl_jac_policy(int jp) { return jp == 0 ? PL_ST_PLAIN : PL_ST_NT; }
constexpr int pl_const_policy(int cp) { return cp == 0 ? PL_ST_NT : PL_ST_WT_NT; }
template <int POLICY>
__device__ __forceinline__ void pl_store(double* p, double v) {
  static_assert(POLICY == PL_ST_PLAIN || POLICY == PL_ST_NT, "8-byte stores: plain or non-temporal");
  if constexpr (POLICY == PL_ST_PLAIN) *p = v;
  else __builtin_nontemporal_store(v, p);
}
template <int POLICY>
__device__ __forceinline__ void pl_store(d2u* p, d2u v) {
  static_assert(POLICY == PL_ST_NT || POLICY == PL_ST_WT_NT, "16-byte stores: non-temporal or write-through + non-temporal");
  if constexpr (POLICY == PL_ST_NT) __builtin_nontemporal_store(v, p);
  else asm volatile("global_store_dwordx4 %0, %1, off sc1 nt\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

// A tile's share of the constant Doffdiag block (LpNLPWrapper.cpp:715-718) out of the staged buffer (record at `cur`, the
// share at cv_src): NX copies, c_stride apart, into the instance's values array; the share is dealt in 128-double
// chunks to NPART waves (this one is `part`).
// 16-byte stores that start on 128-byte lines of the destination: misaligned by 32 B the same stream reaches 3.6 instead
// of 5.4 TB/s, by 64 B 5.1 (tools/ubench/store_pattern.py).  `head` elements bring the first copy to a line boundary (the
// others follow when c_stride is a multiple of 16, e.g. on uniform meshes); they and an odd last element go out as
// single stores.  Non-temporal: this bulk stream (55 % of the metric problem's bytes) is never read again.
template <int NX, int NPART, int POLICY>
__device__ __forceinline__ void pl_const_stores(const double* cur, const double* cv_src, int inst_word, double* __restrict__ vall,
                                                long long sv, int lane, int part) {
  constexpr int CCH = (PL_CMAX / 128 + NPART - 1) / NPART;   // 128-double chunks per wave
  const int* rec = reinterpret_cast<const int*>(cur);
  const int c_dst0 = RPM_REC(rec, c_dst0);
  const int inst = __builtin_amdgcn_readfirstlane(rec[inst_word]);
  const int c_cnt = RPM_REC(rec, c_cnt);
  const int c_stride = RPM_REC(rec, c_stride);
  double* __restrict__ cdst = vall + size_t(inst) * sv + c_dst0;
  const int head = min(int((16 - ((reinterpret_cast<size_t>(cdst) >> 3) & 15)) & 15), c_cnt);   // to a 128-byte line
  d2u cv[CCH];
#pragma unroll
  for (int ch = 0; ch < CCH; ++ch) {
    const int q = max(min(head + (NPART * ch + part) * 128 + 2 * lane, c_cnt - 2), 0);
    cv[ch].x = cv_src[q];
    cv[ch].y = cv_src[q + 1];
  }
  const bool odd_tail = ((c_cnt - head) & 1) != 0;
  const int edge = lane < head ? lane : (lane == head && odd_tail ? c_cnt - 1 : -1);   // lanes 0..head: the leftovers
  const double cedge = cv_src[max(edge, 0)];
#pragma unroll
  for (int ch = 0; ch < CCH; ++ch) {
    const int q = head + (NPART * ch + part) * 128 + 2 * lane;   // 16 B per lane: 1 KB per store instruction
    if (q + 1 < c_cnt) {
#pragma unroll
      for (int i = 0; i < NX; ++i) pl_store<POLICY>(reinterpret_cast<d2u*>(cdst + size_t(i) * c_stride + q), cv[ch]);
    }
  }
  if (part == 0 && edge >= 0) {
#pragma unroll
    for (int i = 0; i < NX; ++i) cdst[size_t(i) * c_stride + edge] = cedge;
  }
}

// role groups (= compute waves) of the pipelined kernel for a problem with R = nx + nu + 2 roles: one role per wave
// when they fit (R <= 12; with the 2 DMA waves 14 waves = 4 per SIMD, which the launch bound turns into a 128-VGPR
// budget), else the fewest equal passes (R = 18: two passes of 9 waves, 11 waves = 3 per SIMD, 168 VGPRs)
constexpr int pl_role_groups(int R) { return (R + (R + 11) / 12 - 1) / ((R + 11) / 12); }

// Shape of the pipelined kernel's workgroup for a problem with R = nx + nu + 2 roles: NH independent halves, each RG
// compute waves (roles g, g + RG, ...) + NDMA DMA waves.  R <= 12: two halves of 4 + 2 waves = 12 waves, 3 per SIMD
// (2 compute + 1 DMA, 168-VGPR budget), three passes per tile — measured best on the metric problem (33.2 us per
// 16-iterate launch) against 2 x (6 + 2) at 128 VGPRs (35.0), one role per wave 12 + 4 (36.3) and 3 x (4 + 1) (38.6).
// Larger problems: one half, the fewest equal passes (R = 18: 9 + 2 waves, 3 per SIMD).
struct PlShape { int NH, RG, NDMA; };
constexpr PlShape pl_shape(int R) { return R <= 12 ? PlShape{2, 4, 2} : PlShape{1, pl_role_groups(R), 2}; }
// (Measured and rejected shapes of this kernel — waves meeting through LDS counters instead of s_barrier, dedicated store
// waves taking finished Jacobian columns out of LDS slots, a dedicated constant-block wave, all waves staging the first tile,
// other wave counts — were compile-time variants of it until round 3; DESIGN.md section 4 keeps their numbers, the code is
// in the history at commit 26aa614.)

// (Tried for the one-half shape, R > 12 roles: __launch_bounds__(..., 6) so that two 11-wave workgroups share a CU and one's
// store phases overlap the other's dynamics.  The quadrotor kernel needs ~156 VGPRs; at 80 it spills 76 of them and the
// 1024-instance sweep takes 89.9 us instead of 51 — DESIGN.md §4.)
// JP, CP: the store policy of the Jacobian and of the constant-block stream (pl_jac_policy, pl_const_policy)
template <class Prob, int NH, int RG, int NDMA, bool WG, bool WJ, bool AN, bool DXM = false, bool STG = false, int JP = 0, int CP = 0>
__global__ __launch_bounds__(NH * 64 * (RG + NDMA), 1) void rpm_tile_pl_kernel(
    const KParams K, int n_inst, int tile_order, const double* __restrict__ xall, double* __restrict__ gall,
    double* __restrict__ vall) {
  constexpr int T = 64;   // a role of a tile is one wave
  constexpr int HT = 64 * (RG + NDMA);   // threads of one half
  constexpr int NX = Prob::NX, NU = Prob::NU, NC = Prob::NC, NQ = prob_nq<Prob>::value;
  constexpr int NXs = NX > 0 ? NX : 1, NUs = NU + NQ > 0 ? NU + NQ : 1;
  constexpr int NO = NX + NC, NV = NX + NU + 1 + NQ, NB = NX + NU + 2 + NQ;
  constexpr int R = WJ ? NV + 1 : (NX > 0 ? NX : 1);
  constexpr int NCs = NC > 0 ? NC : 1;
  constexpr int NTHR = T * RG;
  constexpr int NREC = int(sizeof(TileDev) / sizeof(int));
  extern __shared__ double lds_all[];
  // the halves of a workgroup are independent (own tiles, own LDS); they only share the barriers
  const int half = NH > 1 ? __builtin_amdgcn_readfirstlane(int(threadIdx.x) / HT) : 0;   // wave-uniform
  const int tid = int(threadIdx.x) - half * HT;
  // XCD-aware order (xcd_place), here of halves: the tiles a round of the launch works on (w + j G over all w) leave each
  // XCD's L2 as contiguous pieces of every Jacobian block instead of 2-tile pieces interleaved with the other seven XCDs',
  // and the halves end their last tiles together (102.3 against 108.9 us per 64-iterate step)
  // (engine option "tile_order": which slot of a round a half takes, pl_tile_slot; 0 is the order described here)
  const int nb = int(gridDim.x);
  const int G = NH * nb, w = pl_tile_slot(tile_order, NH, nb, int(blockIdx.x), half);   // this half's place in the tile order
  const int w_h0 = NH > 1 ? pl_tile_slot(tile_order, NH, nb, int(blockIdx.x), 0) : w;
  const int nt = K.n_my_tiles;
  const int W = nt * n_inst;
  const int n_iter = w < W ? (W - w + G - 1) / G : 0;                 // tiles w, w + G, ... of this half
  const int n_iter_wg = (W - w_h0 + G - 1) / G;                       // of half 0: the barrier count of the workgroup
  const PlLds L(NX, NU, NC, NQ, K.max_span, K.max_drow, K.max_cshare, WJ, DXM);
  // (const locals for what the lambdas and the tile loops use: read as L.x there, 22 instantiations allocate registers differently)
  const int S_TT = L.tt, S_X = L.X, S_U = L.U, S_D = L.D, S_TAU = L.tau, S_DG = L.diag, S_ND = L.nodes, S_CV = L.cv, S_SIZE = L.stage;
  double* lds = lds_all + half * L.half;
  double *Fb = lds + L.Fb, *DXs = lds + L.DXs;
  int* fb_ready = reinterpret_cast<int*>(lds + L.ready);   // tile count for which Fb holds the unperturbed dynamics
  int* dx_ready = fb_ready + 1;                            // dx_mode 1: DMA waves that have published their rows of D.X, summed over tiles
#ifdef RPM_DIAG
#define RPM_PTRC(j, slot)                                                           \
  if (K.trace && (threadIdx.x & 63) == 0 && (j) < 2) K.trace[size_t(w) * 64 + (j)*32 + (slot)] = wall_clock64()
// a half's launch-edge stamps (words 22, 23 of its first row): the last tile's barrier A, the end of the last tile's last pass
// (latest compute wave)
#define RPM_PEDGE(slot) \
  if (K.trace && (threadIdx.x & 63) == 0) K.trace[size_t(w) * 64 + (slot)] = wall_clock64()
#define RPM_PEDGE_MAX(slot) \
  if (K.trace && (threadIdx.x & 63) == 0) atomicMax(K.trace + size_t(w) * 64 + (slot), (unsigned long long)wall_clock64())
#else
#define RPM_PTRC(j, slot)
#define RPM_PEDGE(slot)
#define RPM_PEDGE_MAX(slot)
#endif
  if (tid == 0) { RPM_PTRC(0, 31); }

  // A tile's inputs go from global memory straight into an LDS staging buffer (global_load_lds_dwordx4, 16 B per lane, no
  // VGPR round trip): a wave only issues them.  Every run is dealt chunk-wise to the NP waves that stage the tile (this
  // one is `part`), the first chunk of successive runs to successive waves.
  // The addresses of a tile's runs come from its record.  In steady state that record is already in LDS (each
  // staging buffer also carries the record of the tile AFTER its own), so issuing the next tile's loads never waits
  // for global memory; only the first tile of a workgroup reads its record from HBM.
  struct TileRuns { int k0, cnt, span0, span_len, drow0, drow_len, N, x_state0, x_control0, x_t0, node0, c_src0, c_cnt; };
  auto runs_of = [&](auto p) {   // p: the record as ints, in LDS or (first tile) in the constant address space
    return TileRuns{RPM_REC(p, k0), RPM_REC(p, cnt), RPM_REC(p, span0), RPM_REC(p, span_len), RPM_REC(p, drow0),
                    RPM_REC(p, drow_len), RPM_REC(p, N), RPM_REC(p, x_state0), RPM_REC(p, x_control0), RPM_REC(p, x_t0),
                    RPM_REC(p, node0), RPM_REC(p, c_src0), RPM_REC(p, c_cnt)};
  };
  auto stage = [&](auto np_c, int part, int lane, int item, double* buf, const TileRuns tl) {
    constexpr int NP = decltype(np_c)::value;
    const int inst = item / nt, tidx = item - inst * nt;
    const double* __restrict__ x = xall + size_t(inst) * K.n;
    int rot = 0;
    auto run = [&](const double* gsrc, double* ldst, int len) {
      pl_dma_run<NP>(gsrc, ldst, len, lane, (part + NP - (rot++ % NP)) % NP);
    };
    if (part == 0 && lane == 0) reinterpret_cast<int*>(buf + L.rec)[NREC] = inst;   // before the direct loads: an LDS write after them waits for them
    run(reinterpret_cast<const double*>(K.tiles + tidx), buf + L.rec, NREC / 2);
    if (item + G < W) {   // the record of this workgroup's tile after this one
      const int item2 = item + G, inst2 = item2 / nt;
      run(reinterpret_cast<const double*>(K.tiles + (item2 - inst2 * nt)), buf + L.next, NREC / 2);
    }
    run(x + tl.x_t0, buf + S_TT, 2 + NQ);   // t0, tf and the static parameters behind them
#pragma unroll
    for (int i = 0; i < NX; ++i) run(x + tl.x_state0 + i * (tl.N + 1) + tl.span0, buf + S_X + i * K.max_span, tl.span_len);
#pragma unroll
    for (int j = 0; j < NU; ++j) run(x + tl.x_control0 + j * tl.N + tl.k0, buf + S_U + j * T, tl.cnt);
    run(K.points + tl.node0 + tl.k0, buf + S_TAU, tl.cnt);
    if (WJ) run(K.diag + tl.node0 + tl.k0, buf + S_DG, tl.cnt);
    run(reinterpret_cast<const double*>(K.nodes + tl.node0 + tl.k0), buf + S_ND, 2 * tl.cnt);
    if (WG) run(K.dvals + tl.drow0, buf + S_D, tl.drow_len);
    if (WJ && !K.skip_const) run(K.doff_vals + tl.c_src0, buf + S_CV, tl.c_cnt);
  };
  const auto first_runs = [&]() { return runs_of((const __attribute__((address_space(4))) int*)(K.tiles + (w - (w / nt) * nt))); };
  if (tid >= NTHR) {
    // ---------------- DMA waves (two: a direct-to-LDS load takes ~60 ns to issue, so the runs of a tile and the
    // chunks of the constant block are dealt alternately to them) ----------------
    const int lane = (tid - NTHR) & 63;
    const int dw = __builtin_amdgcn_readfirstlane((tid - NTHR) >> 6);
    // The DMA waves' instruction stream is long and scalar; sharing a SIMD with three busy compute waves it would get
    // a quarter of the issue slots (4 us to issue one tile's loads).  They run at raised priority instead.
    __builtin_amdgcn_s_setprio(3);
    if (dw == 0 && lane == 0) { *fb_ready = 0; *dx_ready = 0; }
    // the tile table never changes: constant address space, i.e. scalar loads for the first record
    {
      const auto r0 = first_runs();
      RPM_PTRC(0, 19);
      if (n_iter > 0) stage(std::integral_constant<int, NDMA>{}, dw, lane, w, lds, r0);
      RPM_PTRC(0, 20);
    }
#ifdef RPM_DIAG
    unsigned long long wait_sum = 0, wait_max = 0;   // this wave's s_waitcnt in front of barrier A, over all tiles
#endif
    for (int j = 0; j < n_iter_wg; ++j) {
      const double* cur = lds + (j & 1) * S_SIZE;
      double* nxt = lds + ((j + 1) & 1) * S_SIZE;
#ifdef RPM_DIAG
      const unsigned long long tw0 = wall_clock64();
#endif
      __builtin_amdgcn_s_waitcnt(0);   // the staged loads (and the constant stores before them) have landed
#ifdef RPM_DIAG
      const unsigned long long tw = wall_clock64() - tw0;
      wait_sum += tw;
      wait_max = tw > wait_max ? tw : wait_max;
#endif
      __syncthreads();                 // A: buffer `cur` is complete
      RPM_PTRC(j, 16);
      if constexpr (DXM && WG) {
        // dx_mode 1: the tile's D.X on the FP64 matrix cores (v_mfma_f64_16x16x4_f64), by the DMA waves — the matrix pipe is
        // idle in this kernel and these waves have slack — first thing after the buffer is complete, so that the state
        // roles find it published when their dynamics are done.  A = the tile's block-banded D rows (zero outside a row's
        // interval), B = the staged X rows (span x NX, zero-padded to 16 columns); 16-row blocks are dealt to the NDMA
        // waves; a block only walks the columns its rows' intervals touch (5 k-steps for a 16-node interval).  Operand
        // maps: A: lane l holds A[l&15][l>>4], B: B[l>>4][l&15], C/D: col = l&15, row = (l>>4) + 4 reg.  The k-order
        // (and the fused multiply-add) differ from the reference's ascending-column loop: agreement to rounding only.
        if (j < n_iter) {
          typedef double d4 __attribute__((ext_vector_type(4)));
          const int* rec = reinterpret_cast<const int*>(cur + L.rec);
          const int cnt = RPM_REC(rec, cnt);
          const int span0 = RPM_REC(rec, span0);
          const int drow0 = RPM_REC(rec, drow0);
          const NodeDev* ND = reinterpret_cast<const NodeDev*>(cur + S_ND);
          const double* Ds = cur + S_D;
          const double* Xs = cur + S_X;
          const int lr = lane & 15, kq = lane >> 4;
          for (int rb = 16 * dw; rb < cnt; rb += 16 * NDMA) {
            const int row = rb + lr;
            const bool row_ok = row < cnt;
            const NodeDev ndr = ND[row_ok ? row : cnt - 1];
            const int rel0 = ndr.dcol0 - span0;
            const double* drow = Ds + (ndr.drow_off - drow0);
            const NodeDev nfirst = ND[rb], nlast = ND[min(rb + 15, cnt - 1)];      // wave-uniform: LDS broadcast reads
            const int kmin = __builtin_amdgcn_readfirstlane(nfirst.dcol0 - span0);
            const int kmax = __builtin_amdgcn_readfirstlane(nlast.dcol0 + nlast.dlen - span0);
            for (int cb = 0; cb < NX; cb += 16) {
              const int st = cb + lr;
              d4 acc = {0.0, 0.0, 0.0, 0.0};
              for (int k0 = kmin; k0 < kmax; k0 += 4) {
                const int kcol = k0 + kq;
                const int rel = kcol - rel0;
                const double a = (row_ok && rel >= 0 && rel < ndr.dlen) ? drow[rel] : 0.0;
                const double b = (st < NX && kcol < kmax) ? Xs[st * K.max_span + kcol] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
              }
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int orow = rb + kq + 4 * i;
                if (st < NX && orow < cnt) DXs[st * T + orow] = acc[i];
              }
            }
          }
          if (lane == 0) __hip_atomic_fetch_add(dx_ready, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
      // this tile's share of the constant Doffdiag block (LpNLPWrapper.cpp:715-718), written while the compute waves are
      // in their first pass and store nothing; then the next tile's loads.  (The order matters twice: an LDS read of
      // this wave after the direct-to-LDS loads would wait for them, and the Jacobian stores of the later passes
      // should not meet these in the memory system.)
      if (WJ && !K.skip_const && j < n_iter) pl_const_stores<NX, NDMA, pl_const_policy(CP)>(cur + L.rec, cur + S_CV, NREC, vall, K.sv, lane, dw);
      RPM_PTRC(j, 17);
      if (j + 1 < n_iter) {
        stage(std::integral_constant<int, NDMA>{}, dw, lane, w + (j + 1) * G, nxt, runs_of(reinterpret_cast<const int*>(cur + L.next)));
      }
      RPM_PTRC(j, 18);
    }
#ifdef RPM_DIAG
    if (K.trace && lane == 0 && n_iter > 0) {
      K.trace[size_t(w) * 64 + 28 + dw] = wait_sum;
      K.trace[size_t(w) * 64 + 32 + 28 + dw] = wait_max;
    }
#endif
    // endpoint work items of this workgroup, one wave each
    const int n_end = K.n_tasks * n_inst;
    for (int it = NDMA * w + dw; it < n_end; it += NDMA * G) {
      const int inst = it / K.n_tasks;
      endpoint_block<Prob, WG, WJ, AN, true>(K, K.tasks[it - inst * K.n_tasks], xall + size_t(inst) * K.n,
                                             gall + size_t(inst) * K.sg, vall + size_t(inst) * K.sv, nullptr, inst);
    }
    return;
  }

  // ---------------- compute waves: the role loop of rpm_tile_rl_kernel out of the staged buffer ----------------
  const int kk = tid % T, grp = __builtin_amdgcn_readfirstlane(tid / T);   // a wave is one role group: roles are wave-uniform (scalar branches, scalar block offsets)
  for (int jt = 0; jt < n_iter_wg; ++jt) {
    const double* cur = lds + (jt & 1) * S_SIZE;
    // A, without draining this wave's Jacobian stores: __syncthreads() is fence + s_barrier and the fence waits for
    // vmcnt(0); the stores of tile jt-1 go to addresses nobody in this launch reads, only the LDS traffic has to be over
    // (+0.7 % at 64 iterates per launch, nothing at 16: the store phases are back-pressure, not this wait)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (jt >= n_iter) continue;   // the other half still has a tile: keep the barrier count
    if (grp < 4) { RPM_PTRC(jt, grp * 4 + 0); }
    if (grp == 0 && jt == n_iter - 1) { RPM_PEDGE(22); }
    const int* rec = reinterpret_cast<const int*>(cur + L.rec);
    const int k0 = RPM_REC(rec, k0);
    const int cnt = RPM_REC(rec, cnt);
    const int span0 = RPM_REC(rec, span0);
    const int drow0 = RPM_REC(rec, drow0);
    const int N = RPM_REC(rec, N);
    const int phase_num = RPM_REC(rec, phase_num);
    const int g0 = RPM_REC(rec, g0);
    const int v_nl0 = RPM_REC(rec, v_nl0);
    const int inst = __builtin_amdgcn_readfirstlane(rec[NREC]);
    double* __restrict__ g = gall + size_t(inst) * K.sg;
    double* __restrict__ vals = vall + size_t(inst) * K.sv;
    const auto c4 = (const __attribute__((address_space(4))) double*)(K.consts + size_t(inst) * K.consts_stride);
    const double* Xs = cur + S_X;
    const double* Us = cur + S_U;
    const double* Ds = cur + S_D;
    const int kc = kk < cnt ? kk : cnt - 1;
    const int k = k0 + kc;
    const bool node_ok = kk < cnt;
    bool first = true, no_chk = false;
    // STG: the sub-expressions of the dynamics at the node's unperturbed point, once per wave and tile (role_dynamics)
    typename stage_of<Prob>::type base_stage;
    if constexpr (STG) {
      static_assert(NQ == 0 && !AN, "staged evaluation: finite differences, no static parameters");
      double xs0[NXs], us0[NUs];
#pragma unroll
      for (int i = 0; i < NX; ++i) xs0[i] = Xs[i * K.max_span + (k - span0)];
#pragma unroll
      for (int j = 0; j < NU; ++j) us0[j] = Us[j * T + kc];
      const double tau0 = cur[S_TAU + kc], t00 = cur[S_TT], tf0 = cur[S_TT + 1];
      Prob::stage(phase_num, (tau0 + 1) * ((tf0 - t00) / 2.0) + t00, xs0, us0, c4, base_stage);
    }
    // per-pass scalars (tau, t0, tf, the node record, the diagonal of D) are re-read from LDS where they are used
    // instead of living in registers across the dynamics call: the 10-wave workgroup has 168 VGPRs per lane
    for (int role = grp; role < R || first; role += RG) {
      const bool act = node_ok && role < R;
#ifdef RPM_DIAG
      const bool trc = role == 5;
      if (trc) { RPM_PTRC(jt, 24); }
#endif
      double xs[NXs], us[NUs];   // us = [controls, static parameters]
#pragma unroll
      for (int i = 0; i < NX; ++i) xs[i] = Xs[i * K.max_span + (k - span0)];
#pragma unroll
      for (int j = 0; j < NU; ++j) us[j] = Us[j * T + kc];
#pragma unroll
      for (int j = 0; j < NQ; ++j) us[NU + j] = cur[S_TT + 2 + j];
      double tk;
      {
        const double tau = cur[S_TAU + kc], t0 = cur[S_TT], tf = cur[S_TT + 1];
        tk = (tau + 1) * ((tf - t0) / 2.0) + t0;      // LpNLPWrapper.cpp:80
      }
      const int sv = WJ ? role - 1 : role;
      double dx = 0.0;
      if (WG && !DXM && sv >= 0 && sv < NX) {   // D.X in the reference's ascending-column order (LpSparseMatrix.cpp:142-153)
        const NodeDev nd = reinterpret_cast<const NodeDev*>(cur + S_ND)[kc];
        const double* drow = Ds + (nd.drow_off - drow0);
        const double* xcol = Xs + sv * K.max_span + (nd.dcol0 - span0);
        // same ascending order, operands fetched four columns at a time so that the LDS latency is paid per batch
        int j = 0;
        for (; j + 4 <= nd.dlen; j += 4) {
          const double d0 = drow[j], d1 = drow[j + 1], d2 = drow[j + 2], d3 = drow[j + 3];
          const double x0 = xcol[j], x1 = xcol[j + 1], x2 = xcol[j + 2], x3 = xcol[j + 3];
          dx += d0 * x0;
          dx += d1 * x1;
          dx += d2 * x2;
          dx += d3 * x3;
        }
        for (; j < nd.dlen; ++j) dx += drow[j] * xcol[j];
      }
#ifdef RPM_DIAG
      if (trc) { if (dx == 1e300) xs[0] = 0; RPM_PTRC(jt, 25); }
#endif
      double h = 1.0;
      const int v = role - 1;
      if (WJ && !AN && role >= 1) {   // the role is wave-uniform: fetch the one perturbed variable by its (scalar) row
        double pv;
        if (v < NX) pv = Xs[v * K.max_span + (k - span0)];
        else if (v < NX + NU) pv = Us[(v - NX) * T + kc];
        else if (v == NX + NU) pv = tk;
        else pv = cur[S_TT + 1 + (v - NX - NU)];   // static parameter v - NX - NU - 1
        h = perturb_uniform<NX, NU, NQ>(v, pv, K.tol, xs, us, tk);
      }
      double f[NXs], cp[NCs];
      role_dynamics<Prob, WJ, AN, STG>(phase_num, role, tk, xs, us, c4, f, cp, &base_stage);
#ifdef RPM_DIAG
      if (trc) { if (f[0] == 1e300) cp[0] = 0; RPM_PTRC(jt, 26); }
#endif
      if (first) {   // wave-uniform: the first pass publishes the unperturbed outputs before anyone forms a difference
        if (role == 0 && act) publish_base<Prob, T, WG, false>(f, cp, Fb, kk, g, g0, N, k, no_chk);
        if (grp < 4) { RPM_PTRC(jt, grp * 4 + 1); }
        // F: the other compute waves wait for role 0's outputs.  A flag in LDS, not s_barrier: the DMA waves stay out
        // of it (they are busy with the constant block and the next tile), and the role-0 wave never waits.
        if (grp == 0) {
          __hip_atomic_store(fb_ready, jt + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
          while (__hip_atomic_load(fb_ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < jt + 1)
            __builtin_amdgcn_s_sleep(1);
        }
        if (grp < 4) { RPM_PTRC(jt, grp * 4 + 2); }
        first = false;
      }
      if (act) {
        const double tau = cur[S_TAU + kc], t0 = cur[S_TT], tf = cur[S_TT + 1];
        const double ddiag = cur[S_DG + kc];
        if (WG && sv >= 0 && sv < NX) {
          if constexpr (DXM) {   // published by the DMA waves (matrix cores); NDMA of them per tile
            while (__hip_atomic_load(dx_ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < NDMA * (jt + 1)) __builtin_amdgcn_s_sleep(1);
            dx = DXs[sv * T + kk];
          }
          store_defect<T, false>(sv, dx, tf - t0, Fb, kk, g, g0, N, k, no_chk);
        }
        if (WJ && role >= 1) {
          // The rule of jacobian_blocks, restated: through the helper the staged quadrotor instantiations (168 VGPRs, the
          // 1024-instance sweep's kernels) spill 20 instead of 12 bytes per lane.  Keep the two in step.
          double J[NO];
#pragma unroll
          for (int o = 0; o < NO; ++o) {
            const double pert = o < NX ? f[o < NX ? o : 0] : cp[o >= NX ? o - NX : 0];
            J[o] = AN ? pert : (pert - Fb[o * T + kk]) / h;
          }
          double* __restrict__ vb = vals + v_nl0;   // block bases stay scalar; the node index k is the only per-lane part
          if (v != NX + NU) {
            const int bv = v < NX + NU ? v : v + 1;
#pragma unroll
            for (int o = 0; o < NO; ++o) {
              double val;
              if (o < NX) {
                const double ret = J[o] * (tf - t0) / 2.0;
                val = (o == v) ? ddiag - ret : -ret;
              } else {
                val = J[o];
              }
              pl_store<pl_jac_policy(JP)>(vb + size_t(o * NB + bv) * N + k, val);
            }
          } else {
            const double a0 = -(tau * 0.5) + 0.5, af = (tau * 0.5) + 0.5;
#pragma unroll
            for (int o = 0; o < NO; ++o) {
              double v0, vf;
              if (o < NX) {
                const double fb = Fb[o * T + kk];
                const double dt = J[o] * (tf - t0) / 2.0;
                v0 = fb * (0.5) - a0 * dt;
                vf = -fb * (0.5) + af * dt;
              } else {
                v0 = a0 * J[o];
                vf = af * J[o];
              }
              pl_store<pl_jac_policy(JP)>(vb + size_t(o * NB + NX + NU) * N + k, v0);
              pl_store<pl_jac_policy(JP)>(vb + size_t(o * NB + NX + NU + 1) * N + k, vf);
            }
          }
        }
      }
#ifdef RPM_DIAG
      if (trc) { RPM_PTRC(jt, 27); }
#endif
    }
    if (grp < 4) { RPM_PTRC(jt, grp * 4 + 3); }
    if (jt == n_iter - 1) { RPM_PEDGE_MAX(23); }
  }
}

// Dynamic LDS of a pipelined launch, in bytes.  The constant share is reserved in every launch, also those without a
// Jacobian (the occupancy query of tile_pipeline_setup was made with it).
static size_t pl_lds_bytes(int nx, int nu, int nc, int nq, const KParams& kp, bool dxm) {
  const PlLds L(nx, nu, nc, nq, kp.max_span, kp.max_drow, kp.max_cshare, true, dxm);
  return size_t(pl_shape(nx + nu + 2 + nq).NH) * L.half * sizeof(double);
}

// Occupancy, LDS size and eligibility of the pipelined kernel for this engine; called by device_init.
void tile_pipeline_setup(Engine& e, Device* d, const ProblemDims& pd, int device_id) {
  // rpm_tile_pl_kernel: persistent workgroups of RG compute + 2 DMA waves; as many per CU as the occupancy
      // calculator grants the full (g + Jacobian) variant
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess || ncu <= 0) ncu = 256;
    const int max_c = d->kp.max_cshare;
    int per_cu = 0;
    with_problem(e.problem_id, [&](auto prob) {
      using P = decltype(prob);
      constexpr PlShape S = pl_shape(P::NX + P::NU + 2 + prob_nq<P>::value);
      d->pl_lds = pl_lds_bytes(pd.nx, pd.nu, pd.nc, pd.nq, d->kp, false);
      if (d->pl_lds > 160 * 1024) return;
      auto kern = rpm_tile_pl_kernel<P, S.NH, S.RG, S.NDMA, true, true, false>;
      if (d->pl_lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  int(d->pl_lds));
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, S.NH * 64 * (S.RG + S.NDMA), d->pl_lds) != hipSuccess)
        per_cu = 0;
      (void)hipGetLastError();
      per_cu *= S.NH;   // resident halves per CU
    });
    d->pl_slots = per_cu * ncu;
    d->pl_ok = e.role_looped && e.tile_nodes == 64 && max_c <= PL_CMAX && max_c >= 2 && 2 * pd.nx + 3 + 2 * pd.nq <= 64 &&
               per_cu >= 1;
}

// ------------------------------------------------------------------------------------------
// a kernel's dynamic LDS beyond the default 64 KB
template <class Kern>
static hipError_t allow_lds(Kern kern, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
}

// the one-role and the role-looped kernel: one workgroup per tile and per endpoint work item, grid.y = instances
template <class Kern>
static hipError_t launch_tiles(const Engine& e, Kern kern, int threads, const KParams& kp, const double* dx, double* dg,
                               double* dv, hipStream_t st) {
  const Device& d = *e.dev;
  hipError_t s = allow_lds(kern, d.lds_bytes);
  if (s != hipSuccess) return s;
  dim3 grid(unsigned(d.kp.n_my_tiles + d.kp.n_tasks), unsigned(e.n_instances));
  if (grid.x == 0) return hipSuccess;   // an interval-sharded rank that owns no tile of this (small) mesh
  hipLaunchKernelGGL(kern, grid, dim3(threads), d.lds_bytes, st, kp, dx, dg, dv);
  return hipGetLastError();
}

// dx_mode 1 on the pipelined kernel: finite-difference mode only (as in the one-role kernel), and the D.X buffers must fit
static bool pl_dxm_ok(const Engine& e) {
  ProblemDims pd;
  problem_dims(e.problem_id, &pd);
  return e.first_derive != RPM_DERIVE_ANALYTIC && pl_lds_bytes(pd.nx, pd.nu, pd.nc, pd.nq, e.dev->kp, true) <= 160 * 1024;
}

template <class Prob, bool WG, bool WJ, bool AN, bool DXM, bool STG = false, int JP = 0, int CP = 0>
static hipError_t launch_tile_pl(const Engine& e, const KParams& kp, const double* dx, double* dg, double* dv, hipStream_t st) {
  if constexpr (WJ && JP == 0 && CP == 0) {
    // engine option "store_policy" (jacobian + 2 * constant, rpm_device_internal.hpp); launches without a Jacobian have neither stream.
    // Measured in the kernel, 64 iterates of the metric problem per launch, one box: 0 94.3, 1 86.4, 2 99.5, 3 90.3 us (the
    // write-through constant stream wins in the store-only probe and loses here); 1 also wins with the constant block skipped
    // (67.2 -> 65.2), on 1024 quadrotor instances (42.3 -> 38.1) and at 16 iterates per launch (29.0 -> 26.8)
    switch (e.opt_store_policy) {
      case 1: return launch_tile_pl<Prob, WG, WJ, AN, DXM, STG, 1, 0>(e, kp, dx, dg, dv, st);
      case 2: return launch_tile_pl<Prob, WG, WJ, AN, DXM, STG, 0, 1>(e, kp, dx, dg, dv, st);
      case 3: return launch_tile_pl<Prob, WG, WJ, AN, DXM, STG, 1, 1>(e, kp, dx, dg, dv, st);
      default: break;
    }
  }
  if constexpr (!STG && !AN && has_stage<Prob>::value) {
    // engine option "stage_roles": 1 the functor's staged dynamics, 0 whole-function evaluations, -1 (default) staged when the
    // launch is bound by the dynamics and not by its stores — persistent `values` (kp.skip_const).  Measured on the metric
    // problem, 64 iterates per launch: 75.3 -> 69.5 us with the constant block skipped, but 99.2 -> 106.6 us with all stores (21
    // more registers in a kernel that waits for its stores); same bits either way
    if (e.opt_stage_roles == 1 || (e.opt_stage_roles < 0 && (kp.skip_const || stage_always<Prob>::value)))
      return launch_tile_pl<Prob, WG, WJ, AN, DXM, true, JP, CP>(e, kp, dx, dg, dv, st);
  }
  const Device& d = *e.dev;
  constexpr PlShape S = pl_shape(Prob::NX + Prob::NU + 2 + prob_nq<Prob>::value);
  auto kern = rpm_tile_pl_kernel<Prob, S.NH, S.RG, S.NDMA, WG, WJ, AN, DXM, STG, JP, CP>;
  const size_t lds = pl_lds_bytes(Prob::NX, Prob::NU, Prob::NC, prob_nq<Prob>::value, d.kp, DXM);
  hipError_t s = allow_lds(kern, lds);
  if (s != hipSuccess) return s;
  const long long W = (long long)d.kp.n_my_tiles * e.n_instances;
  const long long halves = W < d.pl_slots ? W : d.pl_slots;   // pl_slots: resident halves (occupancy query)
  hipLaunchKernelGGL(kern, dim3(unsigned((halves + S.NH - 1) / S.NH)), dim3(S.NH * 64 * (S.RG + S.NDMA)), lds, st, kp,
                     e.n_instances, e.opt_tile_order, dx, dg, dv);
  return hipGetLastError();
}

// the pipelined kernel pays off once every resident workgroup has at least two tiles to walk
static bool use_pipeline(const Engine& e) {
  const Device& d = *e.dev;
  if (!d.pl_ok || e.opt_pipeline == 0 || d.kp.n_my_tiles <= 0) return false;
  if (e.opt_pipeline == 1) return true;
  // measured on the metric problem: it wins when every half-workgroup walks >= 2 tiles, or when the tiles fill the
  // resident halves exactly once (the prefetch then hides nothing, but the DMA waves still take the constant block);
  // in between, the second pass over a partly filled chip loses to the role-looped kernel
  const long long W = (long long)d.kp.n_my_tiles * e.n_instances;
  return W >= 2LL * d.pl_slots || (W <= d.pl_slots && 4 * W >= 3LL * d.pl_slots);
}

// which of the three layouts the next constraint launch uses: 2 pipelined, 1 role-looped, 0 one role per thread (the layout
// that carries the fused NaN/Inf check)
static int cons_layout(const Engine& e) {
  if (!(e.role_looped && e.tile_nodes == 64)) return 0;
  if (e.opt_dx_mode == 0) return use_pipeline(e) ? 2 : 1;
  return (use_pipeline(e) && pl_dxm_ok(e)) ? 2 : 0;   // dx_mode 1: matrix-core D.X exists in the pipelined and the one-role kernel
}
bool dev_cons_is_one_role(const Engine& e) { return !e.dev || cons_layout(e) == 0; }

int dev_pl_tile_slot(int order, int nh, int nb, int b, int half) { return pl_tile_slot(order, nh, nb, b, half); }

int dev_pipeline_active(const Engine& e) { return e.dev && cons_layout(e) == 2 ? 1 : 0; }

// The template flags of a constraint launch, the same for all three layouts: WG / WJ what the launch writes (a launch that
// writes neither runs the g kernel); AN the analytic node Jacobian (engine option first_derive, functors that have one,
// launches with a Jacobian); DXM D.X on the matrix cores (dx_mode 1, finite differences, launches with g).  `launch` is
// called with the flags as a TileFlags value; these are all the combinations that are instantiated.
template <bool WG_, bool WJ_, bool AN_, bool DXM_>
struct TileFlags { static constexpr bool WG = WG_, WJ = WJ_, AN = AN_, DXM = DXM_; };

template <class Prob, class Launch>
static hipError_t with_tile_flags(const Engine& e, bool wg, bool wj, Launch&& launch) {
  if constexpr (Prob::HAS_ANALYTIC) {
    if (wj && e.first_derive == RPM_DERIVE_ANALYTIC)
      return wg ? launch(TileFlags<true, true, true, false>{}) : launch(TileFlags<false, true, true, false>{});
  }
  if (wg && e.opt_dx_mode == 1)
    return wj ? launch(TileFlags<true, true, false, true>{}) : launch(TileFlags<true, false, false, true>{});
  if (wg && wj) return launch(TileFlags<true, true, false, false>{});
  if (wj) return launch(TileFlags<false, true, false, false>{});
  return launch(TileFlags<true, false, false, false>{});
}

template <class Prob, int T>
static hipError_t launch_tile_T(const Engine& e, const KParams& kp, bool wg, bool wj, const double* dx, double* dg,
                                double* dv, hipStream_t st) {
  const int layout = T == 64 ? cons_layout(e) : 0;
  return with_tile_flags<Prob>(e, wg, wj, [&](auto flags) -> hipError_t {
    using F = decltype(flags);
    if constexpr (T == 64) {
      if (layout == 2) return launch_tile_pl<Prob, F::WG, F::WJ, F::AN, F::DXM>(e, kp, dx, dg, dv, st);
      if constexpr (!F::DXM) {   // cons_layout: the role-looped kernel only with dx_mode 0
        if (layout == 1) return launch_tiles(e, rpm_tile_rl_kernel<Prob, 64, 4, F::WG, F::WJ, F::AN>, 64 * 4, kp, dx, dg, dv, st);
      }
    }
    constexpr int R = F::WJ ? Prob::NX + Prob::NU + 2 + prob_nq<Prob>::value : (Prob::NX > 0 ? Prob::NX : 1);
    constexpr int threads = (T * R + 63) / 64 * 64;
    return launch_tiles(e, rpm_tile_kernel<Prob, T, F::WG, F::WJ, F::AN, F::DXM>, threads, kp, dx, dg, dv, st);
  });
}

// flags: bit0 = g, bit1 = jacobian values
int dev_eval_cons(Engine& e, const double* d_x, double* d_g, double* d_values, int flags, void* stream) {
  if (!e.dev) {
    int rc = device_init(e, 0);
    if (rc) return rc;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool wg = flags & 1, wj = flags & 2;
  // flags bit 2: the caller's g / values arrays use the padded instance strides (device-resident entry points with option
  // "instance_align"); the host-pointer path keeps its staging buffers dense
  KParams kp = e.dev->kp;
  kp.sg = (flags & 4) ? e.stride_g() : e.m;
  kp.sv = (flags & 4) ? e.stride_values() : e.nnz_jac;
  // flags bit 3 (host-pointer path, one-role kernel only): OR "a stored value is NaN/Inf" into the engine's two host-visible words
  kp.chk = ((flags & 8) && dev_cons_is_one_role(e)) ? e.dev->d_flags2 : nullptr;
  // flags bit 4 (persistent `values`, SURVEY 8d's B'): the caller keeps handing the same device array and leaves its constant
  // Doffdiag block alone; the block (55 % of the metric problem's bytes) is written the first time this engine sees the array
  // and skipped afterwards (neither loaded nor stored)
  kp.skip_const = 0;
  if (wj && (flags & 16) && d_values) {
    auto& seen = e.dev->const_filled;
    if (std::find(seen.begin(), seen.end(), d_values) != seen.end()) {
      kp.skip_const = 1;
    } else {
      if (seen.size() >= 4096) seen.clear();
      seen.push_back(d_values);
    }
  }
  hipError_t s = hipErrorInvalidValue;
  with_problem(e.problem_id, [&](auto prob) {
    using P = decltype(prob);
    switch (e.tile_nodes) {
      case 64: s = launch_tile_T<P, 64>(e, kp, wg, wj, d_x, d_g, d_values, st); break;
      case 32: s = launch_tile_T<P, 32>(e, kp, wg, wj, d_x, d_g, d_values, st); break;
      default: s = launch_tile_T<P, 16>(e, kp, wg, wj, d_x, d_g, d_values, st); break;
    }
  });
  if (s != hipSuccess) {
    e.err = std::string("rpm_tile_kernel launch: ") + hipGetErrorString(s);
    return RPM_E_DEVICE;
  }
  return RPM_OK;
}

}  // namespace rpm
