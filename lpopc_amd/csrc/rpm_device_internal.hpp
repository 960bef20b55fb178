// rpm_device_internal.hpp — what the HIP translation units of the engine share: the kernel parameter blocks, the
// device-side state of an engine, the problem registry and small helpers.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "problems/problems.hpp"
#ifdef RPM_USER_PROBLEM_HEADER
#include RPM_USER_PROBLEM_HEADER   // defines struct rpm::UserProblem (same interface as the structs of problems.hpp)
#endif
#include "rpm_device_restore.hpp"
#include "rpm_engine.hpp"

namespace rpm {

struct KParams {
  const PhaseDev* phases;
  const TileDev* tiles;  // the tiles this rank computes, compact
  int n_my_tiles;
  const TaskDev* tasks;  // endpoint work items, one extra workgroup each
  int n_tasks;
  const NodeDev* nodes;
  const double* points;
  const double* weights;
  const double* diag;
  const double* dvals;
  const double* doff_vals;
  const double* consts;
  int consts_stride;                    // doubles between the constants of consecutive instances (0: shared)
  const LinkDev* links;
  const int* alin_j;     // 2 entries per linear row
  const double* alin_v;
  double tol;
  int P, L, n, m, m_nl, nnz, nnz_nl, nnz_lin, nnz_const;
  long long sg, sv;                     // distance between the g / values arrays of consecutive instances (>= m, nnz)
  int max_span, max_drow;
  int max_cshare;                       // largest constant-block share of a tile (c_cnt)
  int skip_const;                       // 1: this launch leaves the constant Doffdiag block of `values` alone (persistent arrays, dev_eval_cons)
  unsigned long long* trace;            // per-workgroup timestamps (diagnostic build with RPM_DIAG_TRACE set), else NULL
  int* chk;                             // host-pointer path: two host-visible words ORed with "a stored g / Jacobian value is NaN/Inf"; else NULL
};

// Dynamic LDS of rpm_tile_kernel and rpm_tile_rl_kernel (tiles of T nodes): offsets in doubles.  The kernels carve their
// arrays by it and device_init sizes the launch by `total`.
struct TileLds {
  int Xs;      // [nx][max_span]  state-matrix rows the tile's D rows touch
  int Us;      // [nu][T]
  int Ds;      // the tile's D rows, row-major per node (max_drow)
  int Fb;      // [nx + nc][T] unperturbed f and c
  int DXs;     // [nx][T] D.X of the tile (matrix-core variant of rpm_tile_kernel; always reserved)
  int total;
  __host__ __device__ constexpr TileLds(int nx, int nu, int nc, int T, int max_span, int max_drow)
      : Xs(0), Us(Xs + nx * max_span), Ds(Us + nu * T), Fb(Ds + max_drow), DXs(Fb + (nx + nc) * T), total(DXs + nx * T) {}
};
// pins: every array starts where the one before it ends, and the total is the formula the launches have always been sized by
constexpr bool tile_lds_pinned(int nx, int nu, int nc, int T, int span, int drow) {
  const TileLds L(nx, nu, nc, T, span, drow);
  return L.Xs == 0 && L.Us == L.Xs + nx * span && L.Ds == L.Us + nu * T && L.Fb == L.Ds + drow && L.DXs == L.Fb + (nx + nc) * T &&
         L.total == L.DXs + nx * T && L.total == nx * span + nu * T + drow + (nx + nc) * T + nx * T;
}
static_assert(tile_lds_pinned(LaunchProblem::NX, LaunchProblem::NU, LaunchProblem::NC, 64, 73, 64 * 9) &&   // odd span: Us on an odd double
                  tile_lds_pinned(QuadrotorProblem::NX, QuadrotorProblem::NU, QuadrotorProblem::NC, 16, 40, 16 * 41),
              "TileLds: an array overlaps its neighbour or the total changed");

struct HParams {
  const HessPairDev* pairs;
  const HessPhaseDev* phases;
  const HessEndDev* ends;
  const HessLinkDev* links;
  const int* tiles;     // per workgroup: phase, k0, cnt
  const int* red_dst;   // I-part offsets of the parameter scalars (HessPhaseDev::red0)
  int n_tiles, th, n_ends, n_links, nnz_h, tmp_len;
};

struct Device {
  int device_id = -1;
  int* d_flags2 = nullptr;      // two non-finite flag words (g, Jacobian) and their page-locked host mirror
  int* h_flags2 = nullptr;
  size_t trace_words = 0;
  hipStream_t stream = nullptr;
  KParams kp{};
  // tables
  PhaseDev* d_phases = nullptr;
  TileDev* d_tiles = nullptr;
  TaskDev* d_tasks = nullptr;
  NodeDev* d_nodes = nullptr;
  double* d_inst_consts = nullptr;   // n_instances x nconst when rpm_set_instance_constants was used
  double *d_points = nullptr, *d_weights = nullptr, *d_diag = nullptr, *d_dvals = nullptr,
         *d_doff = nullptr, *d_consts = nullptr, *d_alin_v = nullptr;
  LinkDev* d_links = nullptr;
  int* d_alin_j = nullptr;
  // staging buffers of the host-pointer TNLP path
  double *d_x = nullptr, *d_g = nullptr, *d_values = nullptr, *d_grad = nullptr, *d_obj = nullptr,
         *d_lambda = nullptr, *d_hess = nullptr;
  double* d_partial = nullptr;  // objective partial sums
  int* d_flag = nullptr;        // non-finite flag of the host-pointer path
  // page-locked staging buffers the engine owns (hipHostMalloc, mapped): caller arrays that are not registered
  // ("pin_host" off, small, refused) are copied through these by the CPU and never reach the HIP runtime
  struct Stage { double* h = nullptr; double* d = nullptr; size_t cap = 0; bool busy = false; };   // busy: a queued H2D copy still reads it
  Stage stage[STAGE_SLOTS];
  bool cache_valid = false;     // d_g / d_values hold the pair of the x last uploaded
  std::vector<const double*> const_filled;   // device `values` arrays whose constant block this engine has written (option "persistent_values")
  size_t lds_bytes = 0;
  int pl_slots = 0;             // resident halves of the pipelined kernel on this device (occupancy query: per CU x CUs)
  size_t pl_lds = 0;
  bool pl_ok = false;           // the mesh fits rpm_tile_pl_kernel's register staging
  // exact-Hessian tables
  HessPairDev* d_hpairs = nullptr;
  HessPhaseDev* d_hphases = nullptr;
  HessEndDev* d_hends = nullptr;
  HessLinkDev* d_hlinks = nullptr;
  int* d_htiles = nullptr;
  int* d_hred = nullptr;
  double* d_htmp = nullptr;
  HParams hp{};
  size_t hess_lds = 0;
  int hess_threads = 0;
  void* host_path = nullptr;    // state of the host-pointer delivery (rpm_host_path.hip)
  void* exchange = nullptr;     // pack / unpack tables of the interval-sharded exchange (rpm_peer.hip)
  void* mesh_batch = nullptr;   // tables and workspace of the batched mesh-error estimate (rpm_post_kernels.hip), built on first use
  void* carry = nullptr;        // launch plans of the batched carry, one per target engine (rpm_carry_kernels.hip), built on first use
  void* extract = nullptr;      // launch plans and workspace of the batched extraction (rpm_extract_kernels.hip), built on first use
  void* rollout = nullptr;      // host-pointer form's block of the batched roll-out (rpm_rollout_kernels.hip), built on first use
  struct SegTable { void* ptr = nullptr; int count = 0; int stride = -1; };
  SegTable segtab[2][2];        // [g|values][pack|unpack] run tables of the interval sharding
};

#define HIP_TRY(e, call)                                                                   \
  do {                                                                                     \
    hipError_t _s = (call);                                                                \
    if (_s != hipSuccess) {                                                                \
      (e).err = std::string(#call) + ": " + hipGetErrorString(_s);                         \
      return RPM_E_DEVICE;                                                                 \
    }                                                                                      \
  } while (0)

// Host-pointer path (K.chk != nullptr): every thread remembers whether a value it stored was NaN/Inf; the verdicts are
// ORed into host-visible words (word 0: g, word 1: Jacobian values, word 3: objective gradient) — no separate scan
// kernel, no extra launch.  An atomic is issued only when something is wrong.
__device__ __forceinline__ bool nonfinite(double v) { return !(fabs(v) <= 1.7976931348623157e308); }   // NaN or Inf: the one predicate
__device__ __forceinline__ void chk_note(bool& bad, double v) { bad |= nonfinite(v); }
__device__ __forceinline__ void chk_report(int* chk, bool bad_g, bool bad_j) {
  if (chk == nullptr) return;
  if (bad_g) atomicOr_system(chk, 1);
  if (bad_j) atomicOr_system(chk + 1, 1);
}

// Value at tau = +1 of the natural cubic spline through (tau_k, Y(k)), k < N (LpGuessChecker::spline_interpolation,
// Core/LpGuessChecker.cpp:208-270, specialised to the last interval: only the forward recurrence's final z is needed because
// c[n-1] = 0).  One definition for rpm_post_spline_kernel and the batched carry (rpm_carry_kernels.hip): same operations, same bits.
template <class YF>
__device__ __forceinline__ double post_spline_end(int N, const double* tau, YF Y) {
  double mu = 0.0, z = 0.0;
  for (int i = 1; i < N - 1; ++i) {
    const double him1 = tau[i] - tau[i - 1], hi = tau[i + 1] - tau[i];
    const double alpha = 3.0 / hi * (Y(i + 1) - Y(i)) - 3.0 / him1 * (Y(i) - Y(i - 1));
    const double li = 2 * (tau[i + 1] - tau[i - 1]) - him1 * mu;
    mu = hi / li;
    z = (alpha - him1 * z) / li;
  }
  const double d2l = (N - 2 >= 1) ? 2 * z : 0.0;   // c[n-2] = z[n-2] - mu[n-2]*c[n-1], doubled for interior knots
  const double h = tau[N - 1] - tau[N - 2];
  const double A = (tau[N - 1] - 1.0) / h, B = (1.0 - tau[N - 2]) / h;
  const double Cc = (pow(A, 3.0) - A) * (h * h) / 6.0, Dd = (pow(B, 3.0) - B) * (h * h) / 6.0;
  return A * Y(N - 2) + B * Y(N - 1) + Cc * d2l + Dd * 0.0;
}

// ------------------------------------------------------------------------------------------
// problem registry: calls fn with a value of the functor type registered under `id`
template <class F>
inline bool with_problem(int id, F&& fn) {
  switch (id) {
#ifndef RPM_ONLY_USER_PROBLEM   // a user library may leave the built-in functors out (6x shorter build)
    case RPM_PROBLEM_LAUNCH: fn(LaunchProblem{}); return true;
    case RPM_PROBLEM_HYPERSENSITIVE: fn(HypersensitiveProblem{}); return true;
    case RPM_PROBLEM_BRYSON_DENHAM: fn(BrysonDenhamProblem{}); return true;
    case RPM_PROBLEM_BRACHISTOCHRONE: fn(BrachistochroneProblem{}); return true;
    case RPM_PROBLEM_MIN_TIME_CLIMB: fn(MinTimeClimbProblem{}); return true;
    case RPM_PROBLEM_QUADROTOR: fn(QuadrotorProblem{}); return true;
    case RPM_PROBLEM_PARAM_SLED: fn(ParamSledProblem{}); return true;
    case RPM_PROBLEM_PARAM_OSC: fn(ParamOscProblem{}); return true;
#endif
#ifdef RPM_USER_PROBLEM_HEADER
    case RPM_PROBLEM_USER: fn(UserProblem{}); return true;
#endif
  }
  return false;
}


template <class T>
inline hipError_t upload(T** dst, const std::vector<T>& src) {
  const size_t bytes = (src.size() ? src.size() : 1) * sizeof(T);
  hipError_t s = hipMalloc(reinterpret_cast<void**>(dst), bytes);
  if (s != hipSuccess) return s;
  if (!src.empty()) s = hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
  return s;
}


// ------------------------------------------------------------------------------------------
// what the entry points of the sweep steps (mesh-error estimate, carry, shift, sampler, roll-out, extraction) share on the
// host; rpm_device.hip.  Every entry point is: the step's check (host only), DeviceRestore, dev_bind, then the step's launch
// (device form) or HostForm::run around it (host-pointer form).
// dev_bind: device_init on device 0 unless the engine has a device, then that device made current.  With a target engine: an
// engine without a device joins the other's, and the target's error is reported on `e`.
int dev_bind(Engine& e, Engine* to = nullptr);
int step_fail(Engine& e, int code, const std::string& msg);   // e.err = msg; returns code
// the launches queued so far (or `before`, when that already failed): RPM_OK, or "<step> launch: <hip string>", RPM_E_DEVICE
int step_launched(Engine& e, const char* step, hipError_t before = hipSuccess);
int step_no_kernels(Engine& e, const char* step);   // with_problem knew no functor: "<step>: this library has no kernels ..."
// "<who>a column of <largest N + extra> <noun> does not fit one workgroup's LDS", RPM_E_UNSUPPORTED (knots: extra 1, nodes: 0)
int step_no_fit(Engine& e, const std::string& who, const char* noun, int extra);
// first_overlap (rpm_engine.hpp) as a refusal: RPM_OK, or "<who><a> and <b> overlap", RPM_E_INVALID
int step_overlap(Engine& e, const std::string& who, const ByteRange* out, int n_out, const ByteRange* in, int n_in);
constexpr size_t kCuLdsBytes = 160 * 1024;   // LDS of one CU of the MI355X
// dynamic LDS above the 64 KiB every kernel may have: raises the kernel's hipFuncAttributeMaxDynamicSharedMemorySize to the
// CU's LDS on the current device (the attribute is per device and only ever raised); below that nothing
hipError_t raise_dynamic_lds(const void* kernel, size_t bytes);
// nonfinite[b] = 1 when v[b * len .. + len) holds a NaN or Inf, else 0, for b < B: rpm_flag_kernel (rpm_post_kernels.hip) on `stream`
void flag_launch(long long len, const double* v, int* nonfinite, int B, hipStream_t stream);

// The host-pointer form of a sweep step: the device block its results land in, the device verdicts and their page-locked
// mirror.  Grown on demand, never shrunk; what growing replaces is freed once the engine's stream is idle.
struct HostForm {
  double* out = nullptr;
  int *flags = nullptr, *h_flags = nullptr;
  size_t out_cap = 0, flag_cap = 0;
  // a copy between a caller's array and dev + off (dev NULL: the block) through staging slot `slot`; host NULL: skipped.  Two
  // copies of one list never share a slot.
  struct Up { double* dev; size_t off; const double* host; size_t count; int slot; };
  struct Down { double* host; const double* dev; size_t off; size_t count; int slot; };
  // The whole host-pointer form, blocking: the block grown to `doubles`, the uploads (one into the engine's d_x first drops what
  // the callbacks cached, host_new_x), launch(block, verdicts or NULL) on the engine's stream, the verdicts' copy queued, the
  // downloads, the stream synchronised and the verdicts handed out.  The first failure ends it.
  int run(Engine& e, size_t doubles, std::initializer_list<Up> ups, const std::function<int(double* block, int* flags)>& launch,
          std::initializer_list<Down> downs, int* nonfinite);
  void release();

 private:
  int ensure(Engine& e, size_t doubles, size_t B);
  int fetch(Engine& e, const int* nonfinite, size_t B);   // queues the verdicts' copy to the mirror (nonfinite NULL: nothing)
  int finish(Engine& e, int* nonfinite, size_t B);        // synchronises the engine's stream, then hands the verdicts out
};

void host_path_destroy(Device* d);   // rpm_host_path.hip
// rpm_device.hip: staging slots (see Device::Stage)
int dev_stage_reserve(Engine& e, int slot, size_t count, double** host, double** alias);
int dev_stage_upload(Engine& e, int slot, double* dev, const double* host, size_t count);
int dev_stage_download(Engine& e, int slot, double* host, const double* dev, size_t count);
void dev_stage_destroy(Device* d);
void host_new_x(Engine& e);
void dev_stage_synced(Engine& e);    // the engine's stream was synchronised: every staging slot may be overwritten
std::string dev_pin_last_error();
void exchange_destroy(Device* d);    // rpm_peer.hip
void mesh_batch_destroy(Device* d);  // rpm_post_kernels.hip
void carry_destroy(Device* d);       // rpm_carry_kernels.hip
void extract_destroy(Device* d);     // rpm_extract_kernels.hip
void rollout_destroy(Device* d);     // rpm_rollout_kernels.hip

// XCD-aware order: workgroups b, b+8, b+16, ... are dealt to the same XCD, so workgroup b of `count` takes place
// xcd_place(b, count) in the tile order and each XCD gets a contiguous run of tiles; neighbouring 128-byte pieces of every
// Jacobian block then meet in one L2 and leave it as longer contiguous write-backs (speed only, correctness does not depend
// on placement)
__host__ __device__ inline int xcd_place(int b, int count) {
  const int per = count >> 3, rem = count & 7, xcd = b & 7;
  return xcd * per + (xcd < rem ? xcd : rem) + (b >> 3);
}

// Tile orders of rpm_tile_pl_kernel (engine option "tile_order").  A launch of nb workgroups x nh halves works in rounds of
// G = nh nb tiles; half `half` of workgroup b takes slot pl_tile_slot(...) of [0, G) in every round, i.e. tiles slot, slot + G,
// ...: a bijection of the halves onto [0, G) for every order, so each tile is visited exactly once, a half's next tile is
// G further (the staged record of the tile after the current one), and half 0's slot is below half 1's, so that half 0 walks
// at least as many tiles (its count is the workgroup's barrier count).
//   0  each XCD a contiguous eighth of the round (xcd_place): one instance per XCD and round on the metric problem
//   1  the round in two groups of four eighths; XCD 4 q + c takes quarter c of every eighth of group q: one phase of four
//      instances per XCD and round on the metric problem.  Needs nb % 8 == 0 and G % 32 == 0; other grids take order 0.
// (tools/ubench/store_sustained.py ranks these and three more by what the write path takes for the kernel's store streams;
// only what it ranked above order 0 is built here.)
__host__ __device__ inline int pl_tile_slot(int order, int nh, int nb, int b, int half) {
  if (order == 1 && (nb & 7) == 0 && ((nh * (nb >> 3)) & 3) == 0) {
    const int S = nh * (nb >> 3), l = nh * (b >> 3) + half, xcd = b & 7;   // slots per XCD, this half's among them
    const int Q = S >> 2, r = l / Q, t = l - r * Q;
    return (xcd >> 2) * 4 * S + r * S + (xcd & 3) * Q + t;
  }
  return nh * xcd_place(b, nb) + half;
}

// Store policies of rpm_tile_pl_kernel (engine option "store_policy" = jacobian + 2 * constant): the Jacobian stream plain (0)
// or non-temporal (1), the constant-block stream non-temporal (0) or write-through + non-temporal (1).  0 is what the kernel
// did before the option existed, 1 the default (fastest in the kernel); the probe ranked write-through
// Jacobian stores and a plain constant stream at or below 0, they are not built.
// (PL_TILE_ORDERS, PL_STORE_POLICIES: rpm_engine.hpp)

// rpm_tile_kernels.hip: occupancy, LDS size and eligibility of the pipelined kernel for this engine (device_init)
void tile_pipeline_setup(Engine& e, Device* d, const ProblemDims& pd, int device_id);

}  // namespace rpm
