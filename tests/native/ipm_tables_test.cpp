// CPU test of the index tables rpm_ipm_create uploads beside the plan (lpopc_amd/csrc/rpm_ipm_tables.cpp): the ascending fill list
// and the per-interval-block tables of the fused fill, on nested plans of a single-phase problem whose level-1 blocks have no early
// block column, one to four of them, ragged last 16-row blocks, and one that does not fit kkt_factor_dense_kernel.  Compiled
// (with the host-only rpm_setup.cpp, rpm_mesh.cpp, rpm_ipm.cpp, rpm_ipm_tables.cpp) and run by tests/test_ipm_tables_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "../../lpopc_amd/csrc/rpm_ipm.hpp"

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } \
  } while (0)

namespace rpm {
// the registry of the device library, for the one problem id this test uses: 3 states, 1 control, no path constraint
bool problem_dims(int problem_id, ProblemDims* out) {
  if (problem_id != RPM_PROBLEM_BRYSON_DENHAM) return false;
  *out = ProblemDims{3, 1, 0, 8, 0, 0, false, 0};
  return true;
}
}  // namespace rpm

using namespace rpm;

namespace {
constexpr int NX = 3, NU = 1;

// one phase, equal-width intervals of nk[] nodes, x(0) fixed, everything else free, two events
void make_engine(Engine& e, const std::vector<int>& nk) {
  const int K = int(nk.size());
  std::vector<double> mesh(size_t(K) + 1);
  for (int i = 0; i <= K; ++i) mesh[size_t(i)] = i == K ? 1.0 : -1.0 + 2.0 * i / K;
  const double smin[NX * 3] = {0, -10, -10, 1, -10, -10, -10, -10, -10}, smax[NX * 3] = {0, 10, 10, 1, 10, 10, 10, 10, 10};
  const double cmin[NU] = {-5}, cmax[NU] = {5}, emin[2] = {0, -1}, emax[2] = {0, 1};
  const double tg[2] = {0, 1}, sg[NX * 2] = {0, 0, 1, 1, 0, 0}, cg[NU * 2] = {0, 0};
  rpm_phase_desc ph{};
  ph.nx = NX; ph.nu = NU; ph.ne = 2;
  ph.n_intervals = K; ph.mesh_points = mesh.data(); ph.nodes_per_interval = nk.data();
  ph.t0_min = ph.t0_max = 0; ph.tf_min = 0.5; ph.tf_max = 2;
  ph.state_min = smin; ph.state_max = smax; ph.control_min = cmin; ph.control_max = cmax;
  ph.event_min = emin; ph.event_max = emax;
  ph.n_guess = 2; ph.time_guess = tg; ph.state_guess = sg; ph.control_guess = cg;
  rpm_problem_desc d{};
  d.abi_version = RPM_ABI_VERSION;
  d.problem_id = RPM_PROBLEM_BRYSON_DENHAM;
  d.n_phases = 1; d.phases = &ph;
  d.fd_tol = 1e-6;
  d.n_instances = 1;
  d.shard_world = 1;
  const int rc = setup_engine(e, &d);
  if (rc) std::printf("setup_engine: %s\n", e.err.c_str());
  CHECK(rc == RPM_OK);
}

// a lower-triangular pattern of the kind the exact Hessian has: every pair of the variables of one node, tf with each of them,
// the diagonals of the final states and of t0, tf — variable diagonals share their slot with the barrier term (as_hg) — and
// two entries twice
void synthetic_hessian(Engine& e) {
  const PhaseDev& q = e.phd[0];
  e.hes_i.clear(); e.hes_j.clear();
  auto add = [&](int a, int c) { e.hes_i.push_back(a > c ? a : c); e.hes_j.push_back(a > c ? c : a); };
  const int tf = q.x_t0 + 1;
  for (int k = 0; k < q.N; ++k) {
    std::vector<int> at;
    for (int i = 0; i < q.nx; ++i) at.push_back(q.x_state0 + i * (q.N + 1) + k);
    for (int j = 0; j < q.nu; ++j) at.push_back(q.x_control0 + j * q.N + k);
    for (size_t a = 0; a < at.size(); ++a) {
      for (size_t c = 0; c <= a; ++c) add(at[a], at[c]);
      add(tf, at[a]);
    }
    if (k == 1) { add(at[1], at[1]); add(at[2], at[0]); }   // duplicates: one on a diagonal, one off it
  }
  for (int i = 0; i < q.nx; ++i) add(q.x_state0 + i * (q.N + 1) + q.N, q.x_state0 + i * (q.N + 1) + q.N);
  add(q.x_t0, q.x_t0);
  add(tf, tf);
  e.nnz_h = int(e.hes_i.size());
}

std::set<int> rows_met;   // block-row counts of the level-1 blocks seen, built or refused
bool ragged_met = false;   // a built block whose band or border ends inside a 16-row block

// expect_fused: every level-1 block fits kkt_factor_dense_kernel
long check_tables(const std::vector<int>& nk, bool hessian, bool expect_fused) {
  Engine e;
  make_engine(e, nk);
  if (hessian) synthetic_hessian(e);
  IpmPlan p;
  std::string why;
  const int rc = build_ipm_plan(e, p, &why, 1);
  if (rc) std::printf("build_ipm_plan: %s\n", why.c_str());
  CHECK(rc == RPM_OK && p.nd == 1);
  const long long storage = p.storage();

  // ---- sub-problems, long columns
  const IpmSubList s = ipm_sub_list(p);
  CHECK(s.n_l1 == int(nk.size()) && s.n_l1 + s.n_l2 + 1 == int(s.subs.size()));
  int most = 0;
  for (size_t i = 0; i < s.subs.size(); ++i) {
    const KktSub& q = s.subs[i];
    CHECK(q.g.Nt == p.subs[i].Nt && q.g.Nb == p.subs[i].Nb && q.g.nb == p.subs[i].nb && q.g.b == p.subs[i].b && q.g.CS == p.subs[i].CS);
    CHECK(q.koff == p.subs[i].koff && q.roff == p.subs[i].roff);
    most = q.g.Nt > most ? q.g.Nt : most;
  }
  CHECK(s.max_sub_nt == most);
  for (int i : ipm_long_columns(p)) CHECK(p.jt_ptr[size_t(i) + 1] - p.jt_ptr[size_t(i)] > IPM_LONG_COLUMN);

  // ---- the fill list
  const IpmFillList f = ipm_fill_list(p);
  CHECK(f.one_pass);
  const size_t ne = f.dst.size();
  CHECK(f.ki.size() == ne && f.hg.size() == ne);
  for (size_t i = 0; i < ne; ++i) CHECK(f.dst[i] >= 0 && f.dst[i] < storage && (i == 0 || f.dst[i] > f.dst[i - 1]));   // strictly ascending
  std::map<int, int> want;   // ki -> slot: what has to be there exactly once
  std::map<int, int> var_of_slot;
  for (int i = 0; i < p.nv; ++i) var_of_slot[p.diag_dst[size_t(i)]] = i;
  size_t shared = 0;
  for (size_t i = 0; i < p.hg_dst.size(); ++i)
    if (var_of_slot.count(p.hg_dst[i])) ++shared;
    else want[(0 << 28) | int(i)] = p.hg_dst[i];
  for (size_t k = 0; k < p.jac_dst.size(); ++k)
    if (p.jac_dst[k] >= 0) want[(1 << 28) | int(k)] = p.jac_dst[k];
  for (size_t q = 0; q < p.slk_dst.size(); ++q) want[(2 << 28) | int(q)] = p.slk_dst[q];
  for (int i = 0; i < p.nv; ++i) want[(3 << 28) | i] = p.diag_dst[size_t(i)];
  for (int r = 0; r < p.m; ++r) want[(4 << 28) | r] = p.diag_dst[size_t(p.nv + r)];
  CHECK(want.size() == ne);   // with the next line: each exactly once
  std::map<int, int> dst_of_ki;
  size_t shared_seen = 0;
  for (size_t i = 0; i < ne; ++i) {
    const auto it = want.find(f.ki[i]);
    CHECK(it != want.end() && it->second == f.dst[i]);
    CHECK(dst_of_ki.emplace(f.ki[i], f.dst[i]).second);
    if (f.ki[i] >> 28 == 3 && f.hg[i] >= 0) {   // a variable's diagonal that a Hessian slot shares
      CHECK(size_t(f.hg[i]) < p.hg_dst.size() && p.hg_dst[size_t(f.hg[i])] == f.dst[i]);
      ++shared_seen;
    } else {
      CHECK(f.hg[i] == -1);
    }
  }
  CHECK(shared_seen == shared && (shared > 0) == hessian);
  const int nchunk = f.n_chunks();
  CHECK((long long)nchunk * IPM_FILL_CHUNK >= storage && (long long)(nchunk - 1) * IPM_FILL_CHUNK < storage);
  CHECK(f.ptr[0] == 0 && f.ptr[size_t(nchunk)] == int(ne));
  for (int c = 0; c < nchunk; ++c) {   // ptr brackets each chunk
    CHECK(f.ptr[size_t(c)] <= f.ptr[size_t(c) + 1]);
    for (int i = f.ptr[size_t(c)]; i < f.ptr[size_t(c) + 1]; ++i) CHECK(f.dst[size_t(i)] / IPM_FILL_CHUNK == c);
  }

  // ---- the fused fill
  bool fits = true;
  for (int si = 0; si < s.n_l1; ++si) {
    rows_met.insert(s.subs[size_t(si)].g.block_rows());
    fits = fits && s.subs[size_t(si)].g.block_rows() <= IPM_DENSE_ROWS + IPM_DENSE_EARLY;
  }
  CHECK(fits == expect_fused);
  const IpmFusedFill t = ipm_fused_fill(s, f);
  CHECK(t.built == expect_fused);
  if (!t.built) {   // "not built" leaves nothing behind to upload
    CHECK(t.tiles == IPM_DENSE_TILES && t.ptr.empty() && t.ki.empty() && t.hg.empty() && t.live.empty() && t.map.empty());
    CHECK(!ipm_fused_fill(s, IpmFillList{}).built && !ipm_fused_fill(IpmSubList{}, f).built);
    return long(ne);
  }
  CHECK(t.tiles >= IPM_DENSE_TILES && t.ptr.size() == 3 * size_t(s.n_l1) + 1 && t.ki.size() == t.hg.size());
  CHECK(t.map.size() == size_t(s.n_l1) * t.tiles * 64 && t.ptr[0] == 0 && t.ptr.back() == int(t.ki.size()));
  std::vector<char> covered(ne, 0);
  std::map<int, size_t> index_of_ki;
  for (size_t i = 0; i < ne; ++i) index_of_ki[f.ki[i]] = i;
  for (int si = 0; si < s.n_l1; ++si) {
    const KktGeom g = s.subs[size_t(si)].g;
    const long long k0 = s.subs[size_t(si)].koff, k1 = k0 + (long long)g.Nt * g.CS;
    const int nbb = (g.Nb + IPM_W - 1) / IPM_W, NTB = g.block_rows();
    CHECK(ipm_dense_tiles_of(NTB) <= t.tiles);
    ragged_met = ragged_met || g.Nb % IPM_W || g.nb % IPM_W;
    const int first = t.ptr[3 * size_t(si)], last = t.ptr[3 * size_t(si) + 3];
    // the block's list: Jacobian entries, Hessian slots, the rest — each class in ascending slot order, every entry of the block
    long long inside = 0;
    for (size_t i = 0; i < ne; ++i) inside += f.dst[i] >= k0 && f.dst[i] < k1;
    CHECK(last - first == inside && inside <= 0xffff);
    for (int cls = 0; cls < 3; ++cls)
      for (int q = t.ptr[3 * size_t(si) + size_t(cls)]; q < t.ptr[3 * size_t(si) + size_t(cls) + 1]; ++q) {
        const int kind = t.ki[size_t(q)] >> 28;
        CHECK((kind == 1 ? 0 : (kind == 0 ? 1 : 2)) == cls);
        const size_t at = index_of_ki.at(t.ki[size_t(q)]);
        CHECK(t.hg[size_t(q)] == f.hg[at] && f.dst[at] >= k0 && f.dst[at] < k1);
        if (q > t.ptr[3 * size_t(si) + size_t(cls)]) CHECK(f.dst[at] > dst_of_ki.at(t.ki[size_t(q) - 1]));
      }
    // the map, backwards: (sub, tile, lane, quarter) -> (i, j) -> storage slot = the slot of the entry the number points at
    std::vector<std::pair<int, int>> tile_of(size_t(t.tiles), {-1, -1});   // ipm_dense_tile inverted by search
    for (int I = 0; I < NTB; ++I)
      for (int Kb = 0; Kb <= I; ++Kb) {
        const int tile = ipm_dense_tile(NTB, I, Kb);
        CHECK(tile >= 0 && tile < t.tiles && tile_of[size_t(tile)].first < 0);
        tile_of[size_t(tile)] = {I, Kb};
      }
    std::vector<char> numbered(size_t(last - first), 0);
    for (int tile = 0; tile < t.tiles; ++tile)
      for (int lane = 0; lane < 64; ++lane)
        for (int quarter = 0; quarter < 4; ++quarter) {
          const int number = int((t.map[(size_t(si) * t.tiles + tile) * 64 + lane] >> (16 * quarter)) & 0xffff);
          if (!number) continue;
          CHECK(number <= last - first && !numbered[size_t(number) - 1]);
          numbered[size_t(number) - 1] = 1;
          const int I = tile_of[size_t(tile)].first, Kb = tile_of[size_t(tile)].second;
          CHECK(I >= 0);
          const int i = (I < nbb ? IPM_W * I : g.Nb + IPM_W * (I - nbb)) + (lane & 15);
          const int j = (Kb < nbb ? IPM_W * Kb : g.Nb + IPM_W * (Kb - nbb)) + (lane >> 4) + 4 * quarter;
          CHECK(j <= i && i < g.Nt && (I < nbb) == (i < g.Nb) && (Kb < nbb) == (j < g.Nb));
          const size_t at = index_of_ki.at(t.ki[size_t(first + number - 1)]);
          CHECK((long long)g.at(i, j) + k0 == f.dst[at]);
          covered[at] = 1;
        }
    for (char c : numbered) CHECK(c);   // every entry of the block is numbered, none twice (above)
    // the values wait in the panel's LDS space, slot 0 is the zero
    CHECK(size_t(last - first) + 1 <= 2 * size_t(NTB) * IPM_W * IPM_DENSE_LDS_ROW);
  }
  // the live chunks together with the level-1 blocks cover every entry; a chunk that is not live lies inside one block
  for (size_t q = 0; q < t.live.size(); ++q) {
    CHECK(t.live[q] >= 0 && t.live[q] < nchunk && (q == 0 || t.live[q] > t.live[q - 1]));
    for (int i = f.ptr[size_t(t.live[q])]; i < f.ptr[size_t(t.live[q]) + 1]; ++i) covered[size_t(i)] = 1;
  }
  for (size_t i = 0; i < ne; ++i) CHECK(covered[i]);
  const std::set<int> live(t.live.begin(), t.live.end());
  for (int c = 0; c < nchunk; ++c) {
    if (live.count(c)) continue;
    bool in_block = false;
    for (int si = 0; si < s.n_l1; ++si) {
      const KktSub& q = s.subs[size_t(si)];
      in_block = in_block || ((long long)c * IPM_FILL_CHUNK >= q.koff && (long long)(c + 1) * IPM_FILL_CHUNK <= q.koff + (long long)q.g.Nt * q.g.CS);
    }
    CHECK(in_block);
  }

  // ---- the same input again: the same bytes
  const IpmFillList f2 = ipm_fill_list(p);
  CHECK(f2.one_pass == f.one_pass && f2.dst == f.dst && f2.ki == f.ki && f2.hg == f.hg && f2.ptr == f.ptr);
  const IpmFusedFill t2 = ipm_fused_fill(ipm_sub_list(p), f2);
  CHECK(t2.built && t2.tiles == t.tiles && t2.ptr == t.ptr && t2.ki == t.ki && t2.hg == t.hg && t2.live == t.live && t2.map == t.map);
  return long(ne);
}
}  // namespace

int main() {
  // nodes per interval -> 16-row blocks of the interval's sub-problem (7 nk - 3 interior unknowns, a border of 8 or 11):
  // 4 -> 3, 12 -> 7, 38 -> 18 (1 early block column), 40 -> 19 (2), 43 -> 20 (3), 45 -> 21 (4), 48 -> 22 (does not fit)
  const std::vector<std::pair<std::vector<int>, bool>> meshes = {
      {{4, 5, 3}, true}, {{12, 12, 12}, true}, {{38, 4}, true}, {{6, 40, 43}, true}, {{45, 5}, true}, {{4, 48}, false}, {{48}, false}};
  long entries = 0;
  for (const auto& mesh : meshes)
    for (int hessian = 0; hessian < 2; ++hessian) entries += check_tables(mesh.first, hessian != 0, mesh.second);
  std::printf("ok: %zu meshes x 2 Hessian modes, %ld entries, level-1 block rows met:", meshes.size(), entries);
  for (int r : rows_met) std::printf(" %d", r);
  std::printf("\n");
  // no early block column, one to four of them, and a block that does not fit
  int early_met = 0;
  for (int r : rows_met)
    if (r > IPM_DENSE_ROWS && r <= IPM_DENSE_ROWS + IPM_DENSE_EARLY) early_met |= 1 << (r - IPM_DENSE_ROWS);
  CHECK(ragged_met && early_met == 0x1e && *rows_met.begin() <= IPM_DENSE_ROWS && *rows_met.rbegin() > IPM_DENSE_ROWS + IPM_DENSE_EARLY);
  return 0;
}
