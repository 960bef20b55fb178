// rpm_ipm.hpp — row f-2: the caller of the hot path, moved onto the device.  The reference hands the NLP to Ipopt 3.12.3
// (Core/LpNLPSolver.cpp:13-53: tol = "Ipopt-tol", hessian_approximation from the option list); Ipopt is not in the
// reference tree, so what is built here is a restatement of its published algorithm (Waechter & Biegler, Math. Program.
// 106, 2006: primal-dual barrier, fraction-to-the-boundary rule, filter line search, inertia correction) for a batch of
// independent instances of one transcription — the MPC sweep of BASELINE config 5 — with every iterate, multiplier,
// KKT matrix and factor resident in HBM.  Restated beyond the basic iteration: bound_relax_factor, the second-order correction,
// the restoration phase (paper section 3.3, with a Gauss-Newton model of the constraint curvature) and least-squares
// multipliers on leaving it, Ipopt's adaptive barrier update with the LOQO oracle (option "mu_strategy", default 1; 0 = monotone) and its
// gradient-based NLP scaling (option "nlp_scaling", off by default).  Not restated: the quality-function oracle, the watchdog.  See DESIGN.md §f-2.
//
// The KKT matrix of a collocation NLP is banded once the unknowns are ordered along time: node k's states, controls,
// slacks and multipliers sit together, a defect row reaches the nodes of its own mesh interval only.  What does not
// fit the band (final states, t0/tf, events, linkages, linear rows) goes into a dense border ("arrow").  IpmPlan holds
// that ordering and, for every Jacobian / Hessian COO entry, its slot in the band + border storage.
#pragma once
#include <string>
#include <vector>

#include "rpm_engine.hpp"

namespace rpm {

// One dense-ish sub-problem of the factorisation in band + border storage: element (i, j), i >= j, of its lower triangle
// sits at koff + j * CS + (i < Nb ? i - j : b + 1 + i - Nb) of the instance's KKT storage; its right-hand side is the
// slice [roff, roff + Nt) of the instance's vector.
struct KktSubHost {
  int Nt, Nb, nb, b, CS;
  long long koff;
  int roff;
};

struct IpmPlan {
  int n = 0, m = 0, ns = 0, nv = 0;   // variables, rows, slacks (one per inequality row), nv = n + ns
  int Nt = 0, Nb = 0, nb = 0;         // KKT order, banded part, border
  int b = 0, CS = 0;                  // half bandwidth, doubles per stored column (b + 1 + nb, rounded up to even)
  std::vector<int> pos;               // unknown -> position; unknowns: [0,n) x, [n,nv) slacks, [nv,nv+m) multipliers
  std::vector<int> row_slack;         // m: slack index or -1 (equality row)
  std::vector<int> slack_row;         // ns
  std::vector<int> fixed;             // n: 1 where x_l == x_u (kept as identity rows of the KKT system)
  std::vector<int> jac_dst, hes_dst;  // storage offset of every COO entry, -1 = dropped (fixed variable)
  std::vector<int> diag_dst;          // Nt: offset of every unknown's diagonal entry
  std::vector<int> slk_dst;           // ns: offset of the (row, slack) entry (value -1)
  std::vector<int> jt_ptr, jt_ent, jt_row;   // Jacobian by column (deterministic J^T lambda)
  std::vector<int> hg_ptr, hg_src, hg_dst;   // Hessian by storage slot: K[hg_dst[i]] += (sum of hess[hg_src[...]] in COO order) — duplicates
                                             // (I-part / E-part, LpHessian.cpp:598) are summed in a fixed order, not by racing atomics
  // ---- nested dissection by mesh interval (nd = 1) ------------------------------------------------------------------
  // The unknowns of a mesh interval — states of its nodes but the first, controls, slacks, defect / path multipliers —
  // couple only to each other, to the states at the interval's first node ("separator"), to the separator of the NEXT
  // interval (last column of the interval's D block, Core/RPMGenerator.cpp:150-165) and to the border.  Level 1: every
  // interval is a band + border sub-problem of its own (border = its two separators + the global border; the first node's
  // controls, slacks and multipliers are ordered last inside it, see rpm_ipm.cpp), factored up to
  // its corner by a workgroup of its own; the corners are Schur complements that add up (in a fixed order) into level 2:
  // the separators in time order (block tridiagonal, blocks of nx) + the global border, one more band + border problem.
  // A quasi-definite matrix has an LDL^T under every symmetric permutation (Vanderbei 1995), so this ordering needs no
  // pivoting either, and the signs of all the D's still give the inertia.
  int nd = 0;
  int Nt_alloc = 0;                   // length of the right-hand-side vector: Nt plus the level-1 border work spaces
  long long storage_nd = 0;           // doubles of KKT storage per instance (level-1 blocks, then level 2)
  std::vector<KktSubHost> subs;       // level-1 sub-problems, [level-2 groups,] then ONE entry for the last level
  // ---- optional third level (n_l2 > 0): the separator system of a long mesh is itself banded (block tridiagonal), so it is cut
  // again, at the matrix level: consecutive groups of l3_S of its positions, the trailing l3_w (= its half bandwidth) of every
  // group but the last form that group's separator.  Group interiors are level-2 sub-problems (border = the previous
  // group's separator, its own, the global border), factored up to their corners by a workgroup each; all group separators in
  // order + the global border are the last level.  Delta-III 4 x 64 x 16: one chain of 112 block columns -> 8 + 16.
  int n_l2 = 0, l3_S = 0, l3_w = 0, l3_G = 0, l3_Nb2 = 0, l3_base = 0;
  std::vector<int> l3_gb_ptr, l3_gb;     // per group: the global-border unknowns (numbered inside the border) that have rows in its block, ascending
  int n_cg_long = 0, n_cg2_long = 0;   // the corner-gather tables start with the destinations that have >= 32 sources (a wave each on the device)
  std::vector<int> cg2_ptr, cg2_src, cg2_dst, rg2_ptr, rg2_src, rg2_dst, rs2_dst, rs2_src;   // second gather / scatter stage (level 2 -> last level)
  std::vector<int> cg_ptr, cg_src;    // corner gather: level-2 storage offset cg_dst[i] += sum of K[cg_src[cg_ptr[i] .. cg_ptr[i+1])]
  std::vector<int> cg_dst;
  std::vector<int> rg_ptr, rg_src;    // right-hand-side gather: rhs[rg_dst[i]] += sum of rhs[rg_src[...]]  (level-1 border work spaces)
  std::vector<int> rg_dst;
  std::vector<int> rs_dst, rs_src;    // solution scatter: rhs[rs_dst[i]] = rhs[rs_src[i]]
  std::vector<int> gap_pos;           // every position of a level-1 border work space (zeroed before the forward sweep)
  std::vector<int> nd_ivl, nd_loc, nd_sep, nd_sep0, nd_nsep, nd_last, nd_nstate0, nd_sep_state;   // classification kept for ipm_plan_offset
  std::vector<int> nd_gb_ptr, nd_gb;     // per interval: the global-border unknowns (numbered inside the border) that have rows in its block, ascending
  int max_rows = 0;                   // largest 16 + b + nb over all sub-problems (rows of a block column)
  size_t max_factor_lds = 0;
  long long storage() const { return nd ? storage_nd : (long long)Nt * CS; }
  long long at(int pa, int pb) const {        // pa >= pb
    return (long long)pb * CS + (pa < Nb ? pa - pb : b + 1 + pa - Nb);
  }
};

// rpm_ipm.cpp (host only): ordering, band width and the scatter maps from the engine's layout
int build_ipm_plan(Engine& e, IpmPlan& p, std::string* why, int nested = 0);   // nested: 0 one band, 1 by mesh interval, third level when the separator system is long (engine option ipm_nested_group)
void ipm_plan_group_hessian(IpmPlan& p);   // hg_* from hes_dst
// storage offset of the entry between unknowns ua, uc ([0,n) x, [n,nv) slacks, [nv,nv+m) multipliers); -1 if the layout has no slot for it
long long ipm_plan_offset(const IpmPlan& p, int ua, int uc);

// ---- what the host tables below and the kernels that read them share: one definition for the host compiler and for hipcc
#if defined(__HIP__) || defined(__HIPCC__)
#define RPM_IPM_HD __host__ __device__
#else
#define RPM_IPM_HD
#endif

constexpr int IPM_W = 16;               // block width of the factorisation
constexpr int IPM_LONG_COLUMN = 256;    // a Jacobian column of more entries gets a workgroup of its own in ipm_jt_lambda_kernel
constexpr int IPM_FILL_CHUNK = 4096;    // doubles of KKT storage one workgroup of ipm_fill_kernel zeroes and fills at a time (2048: 76 us, 4096: 70 us, 8192: 82 us on the metric problem)
constexpr int IPM_DENSE_SLOTS = 22, IPM_DENSE_TILE_WAVES = 7, IPM_DENSE_LDS_ROW = 18;   // kkt_factor_dense_kernel: tiles per wave, tile waves, doubles per LDS row
constexpr int IPM_DENSE_TILES = IPM_DENSE_SLOTS * IPM_DENSE_TILE_WAVES;
// kkt_factor_dense_kernel keeps the trailing IPM_DENSE_ROWS block rows of a block in registers; a block of up to IPM_DENSE_EARLY more
// eliminates its first ("early") block columns through the storage: their tiles are loaded, used and put back by the wave that owns them
// (4: three tiles per wave and early column wait in registers beside the resident ones; a fourth spills)
constexpr int IPM_DENSE_ROWS = 17, IPM_DENSE_EARLY = 4;
static_assert(IPM_DENSE_ROWS * (IPM_DENSE_ROWS + 1) / 2 <= IPM_DENSE_TILES, "resident tiles");
RPM_IPM_HD inline int ipm_dense_early(int block_rows) { return block_rows > IPM_DENSE_ROWS ? block_rows - IPM_DENSE_ROWS : 0; }
// number of tile (I, Kb), Kb <= I, of a block of `block_rows` block rows: the resident ones (Kb >= early columns) column by column
// from 0 — tile t sits in slot t / 7 of wave t % 7 —, the early ones after them
RPM_IPM_HD inline int ipm_dense_tile(int block_rows, int I, int Kb) {
  const int E = ipm_dense_early(block_rows), R = block_rows - E;
  if (Kb >= E) { const int kr = Kb - E; return kr * R - kr * (kr - 1) / 2 + I - Kb; }
  return R * (R + 1) / 2 + Kb * block_rows - Kb * (Kb - 1) / 2 + I - Kb;
}
RPM_IPM_HD inline int ipm_dense_tiles_of(int block_rows) { return block_rows * (block_rows + 1) / 2; }

// LDS bytes of kkt_factor_kernel for a sub-problem of half bandwidth b and border nb (rpm_kkt_factor.hip)
inline size_t ipm_factor_lds_bytes(int b, int nb) {
  const size_t W = IPM_W;
  return (size_t(b + 24) * W + W * (W + 1) + W * W + W + 2 * size_t(nb) * W + size_t(nb) * (nb + 1) / 2) * sizeof(double);
}

// band + border storage of one instance (IpmPlan::at): element (i, j), i >= j
struct KktGeom {
  int Nt, Nb, nb, b, CS;
  RPM_IPM_HD size_t at(int i, int j) const { return size_t(j) * CS + (i < Nb ? i - j : b + 1 + i - Nb); }
  RPM_IPM_HD int block_rows() const { return (Nb + IPM_W - 1) / IPM_W + (nb + IPM_W - 1) / IPM_W; }   // 16-row blocks: band, then border
};
// one sub-problem of the factorisation as the kernels take it (KktSubHost): its geometry, where its block starts inside an
// instance's KKT storage, where its right-hand side starts inside an instance's vector
struct KktSub {
  KktGeom g;
  int roff;
  long long koff;
};

// ---- rpm_ipm_tables.cpp (host only): the index tables rpm_ipm_create uploads, pure functions of the plan
// The factorisation's sub-problems: the whole band + border matrix, or (nested dissection) n_l1 interval blocks, n_l2 groups of
// separators and the last level.
struct IpmSubList {
  std::vector<KktSub> subs;
  int n_l1 = 0, n_l2 = 0, max_sub_nt = 0;
};
IpmSubList ipm_sub_list(const IpmPlan& p);
std::vector<int> ipm_long_columns(const IpmPlan& p);   // Jacobian columns of more than IPM_LONG_COLUMN entries, ascending

// Every structural slot of the KKT storage in ascending order (IpmDev::as_*): ki = kind << 28 | index — kind 0 Hessian slot hg i,
// 1 Jacobian entry k, 2 slack s, 3 diagonal of variable i (hg: the Hessian slot that shares it, or -1), 4 diagonal of constraint r.
// (decoded by SlotValue, rpm_kkt_slots.hpp).  one_pass: ipm_fill_kernel (rpm_kkt_assemble.hip) can use the list (sizes below 2^28, no two writers of one slot, offsets inside the storage); ptr[c] is
// then the first entry at or beyond chunk c (IPM_FILL_CHUNK doubles), ptr.size() - 1 chunks.
struct IpmFillList {
  std::vector<int> dst, ki, hg, ptr;
  bool one_pass = false;
  int n_chunks() const { return one_pass ? int(ptr.size()) - 1 : 0; }
};
IpmFillList ipm_fill_list(const IpmPlan& p);

// Level 1 assembled by kkt_factor_dense_kernel itself (IpmDev::df_*): per interval block the entries of `fill` inside it — the
// Jacobian entries from ptr[3 s], the Hessian slots from ptr[3 s + 1], slack entries and diagonals from ptr[3 s + 2] — and per lane
// of register tile t the four 16-bit numbers (1-based into the block's list, 0 = a structural zero) of the entries it holds:
// map[(s * tiles + t) * 64 + (column & 3) * 16 + row] >> 16 * (column >> 2).  live: the chunks of `fill` that do not lie inside a
// level-1 block, the only ones ipm_fill_kernel then fills.  built = false (and nothing else filled in): no one-pass list, no level-1
// blocks, a block of more than IPM_DENSE_ROWS + IPM_DENSE_EARLY block rows, more than 0xffff entries in a block, or more entries
// than the LDS of its panel holds.
struct IpmFusedFill {
  bool built = false;
  int tiles = IPM_DENSE_TILES;
  std::vector<int> ptr, ki, hg, live;
  std::vector<unsigned long long> map;
};
IpmFusedFill ipm_fused_fill(const IpmSubList& s, const IpmFillList& fill);

// Solution sensitivities to fixed variables (rpm_ipm_sens.hip): column k answers "how does the solution move with fixed variable
// var_index[k]", so its right-hand side is minus column var_index[k] of the KKT matrix's off-diagonal blocks — the Hessian entries
// {i, var_index[k]} on the rows of the free variables i, the Jacobian entries (r, var_index[k]) on the constraint rows — and zero
// on slacks and fixed unknowns.  The source table: group g writes rhs[par[g]][dst[g]] = -(sum of its sources src[ptr[g] ..
// ptr[g + 1]) in list order); a source is kind << 28 | triplet, kind 0 a Hessian triplet, 1 a Jacobian triplet.  Groups are sorted
// by (parameter, KKT position) — consecutive threads of the gather write ascending positions —, the sources of a group ascend
// (all Hessian triplets, then the Jacobian ones: a group holds one kind only, since a position is a variable's or a row's).
constexpr int IPM_SENS_MAX_PAR = 32;   // parameters of one call (right-hand sides per instance of its substitution)
struct IpmSensTable {
  std::vector<int> ptr, par, dst, src;
  int n_groups() const { return int(dst.size()); }
};
// Checks the parameter list (RPM_E_INVALID with *why: NULL list, n_par outside 1 .. IPM_SENS_MAX_PAR, an index outside [0, n), a
// duplicate, a variable that is free in the plan) and builds the table.  hes_i / hes_j: the nnz_h Hessian triplets (either
// triangle).  A pure function of its arguments.
int ipm_sens_table(const IpmPlan& p, int nnz_h, const int* hes_i, const int* hes_j, int n_par, const int* var_index, IpmSensTable* t,
                   std::string* why);

// Solution sensitivities to the instances' constants (rpm_ipm_constant_sensitivities, rpm_ipm_sens.hip): the right-hand side of a
// constant is minus the central difference of grad f + J' lambda on the rows of the free variables and of g on the constraint rows,
// so its gather walks, per free variable, the Jacobian triplets of that variable's column.  The column table: entry u < n_free is
// free variable var[u] at KKT position var_pos[u] with the triplets ent[ptr[u] .. ptr[u + 1]) — those of its column inside the
// state-dependent block [NL] (triplet index < nnz_nl; the linear and the constant block do not depend on the constants), in
// ascending triplet index — and their rows ent_row[]; row_pos[r] is the KKT position of constraint row r.  Free variables ascend.
struct IpmConstTable {
  std::vector<int> var, var_pos, ptr, ent, ent_row, row_pos;
  int n_free() const { return int(var.size()); }
};
IpmConstTable ipm_const_table(const IpmPlan& p, int nnz_nl);   // a pure function of its arguments
// The list of constants of such a call: RPM_OK, or RPM_E_INVALID with *why — a functor without constants (nconst = 0), a NULL list,
// n_par outside 1 .. IPM_SENS_MAX_PAR, an index outside [0, nconst), a duplicate.  A pure function of its arguments.
int ipm_const_list_check(int nconst, int n_par, const int* const_index, std::string* why);

}  // namespace rpm
