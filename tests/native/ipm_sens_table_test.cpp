// CPU test of the source table of the sensitivity right-hand sides (ipm_sens_table, lpopc_amd/csrc/rpm_ipm_tables.cpp) on the plans of
// the shapes tests/test_ipm_pass.py uses: quadrotor 2 x 4 (band and nested; parameters: the 12 initial states and tf), bryson_denham
// 2 x 8 (parameter: t0), launch 2 x 5 (four phases with linkages; parameters: the fixed initial states of phase 1).  Every table
// entry is walked against a brute-force restatement — all triplets that touch the parameter, destinations through pos, nothing on
// fixed rows or slacks, ascending order inside a group — and every refusal is exercised.  Compiled (with the host-only rpm_setup.cpp,
// rpm_mesh.cpp, rpm_ipm.cpp, rpm_ipm_tables.cpp) and run by tests/test_ipm_sens_table_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../../lpopc_amd/csrc/rpm_ipm.hpp"

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } \
  } while (0)

namespace rpm {
// the registry of the device library, for the three problem ids this test uses (static dimensions only)
bool problem_dims(int problem_id, ProblemDims* out) {
  if (problem_id == RPM_PROBLEM_QUADROTOR) *out = ProblemDims{12, 4, 0, 0, 0, 15, false, 0};
  else if (problem_id == RPM_PROBLEM_BRYSON_DENHAM) *out = ProblemDims{3, 1, 0, 8, 0, 0, false, 0};
  else if (problem_id == RPM_PROBLEM_LAUNCH) *out = ProblemDims{7, 3, 1, 5, 7, 22, false, 0};
  else return false;
  return true;
}
}  // namespace rpm

using namespace rpm;

namespace {

// what the table needs of a phase: sizes, which times and initial states are fixed
struct PhaseShape {
  int nx, nu, nc, ne;
  bool t0_fixed, tf_fixed;
  std::vector<int> state0_fixed;   // nx flags
};

void make_engine(Engine& e, int problem_id, int n_consts, const std::vector<PhaseShape>& shapes, int links_of, int K, int nk) {
  const size_t P = shapes.size();
  std::vector<double> mesh(size_t(K) + 1);
  for (int i = 0; i <= K; ++i) mesh[size_t(i)] = i == K ? 1.0 : -1.0 + 2.0 * i / K;
  const std::vector<int> nodes(size_t(K), nk);
  std::vector<std::vector<double>> keep;   // the arrays the descriptions point into
  auto arr = [&](std::vector<double> v) { keep.push_back(std::move(v)); return keep.back().data(); };
  keep.reserve(16 * P + 8);
  std::vector<rpm_phase_desc> ph(P);
  const double tg[2] = {0, 1};
  for (size_t q = 0; q < P; ++q) {
    const PhaseShape& s = shapes[q];
    rpm_phase_desc& d = ph[q];
    d = rpm_phase_desc{};
    d.nx = s.nx; d.nu = s.nu; d.nc = s.nc; d.ne = s.ne;
    d.n_intervals = K; d.mesh_points = mesh.data(); d.nodes_per_interval = nodes.data();
    d.t0_min = double(q); d.t0_max = s.t0_fixed ? double(q) : double(q) + 0.5;
    d.tf_min = double(q) + 1.0; d.tf_max = s.tf_fixed ? double(q) + 1.0 : double(q) + 3.0;
    std::vector<double> smin, smax;
    for (int i = 0; i < s.nx; ++i) {
      const double lo0 = s.state0_fixed[size_t(i)] ? 0.25 : -10.0, hi0 = s.state0_fixed[size_t(i)] ? 0.25 : 10.0;
      smin.insert(smin.end(), {lo0, -10.0, -10.0});
      smax.insert(smax.end(), {hi0, 10.0, 10.0});
    }
    d.state_min = arr(smin); d.state_max = arr(smax);
    d.control_min = arr(std::vector<double>(size_t(s.nu), -1.0)); d.control_max = arr(std::vector<double>(size_t(s.nu), 1.0));
    d.path_min = arr(std::vector<double>(size_t(s.nc) + 1, 1.0)); d.path_max = arr(std::vector<double>(size_t(s.nc) + 1, 1.0));
    d.event_min = arr(std::vector<double>(size_t(s.ne) + 1, 0.0)); d.event_max = arr(std::vector<double>(size_t(s.ne) + 1, 0.0));
    d.n_guess = 2; d.time_guess = tg;
    d.state_guess = arr(std::vector<double>(size_t(s.nx) * 2, 0.0));
    d.control_guess = arr(std::vector<double>(size_t(s.nu) * 2, 0.0));
  }
  std::vector<rpm_link_desc> links;
  const std::vector<double> zeros(size_t(links_of > 0 ? links_of : 1), 0.0);
  for (size_t q = 0; links_of > 0 && q + 1 < P; ++q) links.push_back(rpm_link_desc{int(q) + 1, int(q) + 2, links_of, zeros.data(), zeros.data()});
  const std::vector<double> consts(size_t(n_consts) + 1, 1.0);
  rpm_problem_desc d{};
  d.abi_version = RPM_ABI_VERSION;
  d.problem_id = problem_id;
  d.n_phases = int(P); d.phases = ph.data();
  d.n_links = int(links.size()); d.links = links.data();
  d.n_consts = n_consts; d.consts = consts.data();
  d.fd_tol = 1e-6;
  d.n_instances = 1;
  d.shard_world = 1;
  const int rc = setup_engine(e, &d);
  if (rc) std::printf("setup_engine: %s\n", e.err.c_str());
  CHECK(rc == RPM_OK);
}

// a lower-triangular pattern of the kind the exact Hessian has: every pair of the variables of one node, t0 and tf with each of
// them, the final states' diagonals, the time block; at the first node of every phase three entries twice (a pair of states, a
// control with a state, tf with a state), so that groups of several sources exist wherever an initial state or tf is a parameter
void synthetic_hessian(Engine& e) {
  e.hes_i.clear(); e.hes_j.clear();
  auto add = [&](int a, int c) { e.hes_i.push_back(a > c ? a : c); e.hes_j.push_back(a > c ? c : a); };
  for (const PhaseDev& q : e.phd) {
    const int t0 = q.x_t0, tf = q.x_t0 + 1;
    for (int k = 0; k < q.N; ++k) {
      std::vector<int> at;
      for (int i = 0; i < q.nx; ++i) at.push_back(q.x_state0 + i * (q.N + 1) + k);
      for (int j = 0; j < q.nu; ++j) at.push_back(q.x_control0 + j * q.N + k);
      for (size_t a = 0; a < at.size(); ++a) {
        for (size_t c = 0; c <= a; ++c) add(at[a], at[c]);
        add(tf, at[a]);
        add(t0, at[a]);
      }
      if (k == 0) { add(at[1], at[0]); add(at[size_t(q.nx)], at[0]); add(tf, at[size_t(q.nx)]); add(at[0], at[size_t(q.nx)]); }
    }
    for (int i = 0; i < q.nx; ++i) add(q.x_state0 + i * (q.N + 1) + q.N, q.x_state0 + i * (q.N + 1) + q.N);
    add(t0, t0); add(tf, t0); add(tf, tf);
  }
  e.nnz_h = int(e.hes_i.size());
}

long sources_walked = 0, groups_walked = 0, long_groups = 0;

void check_table(const Engine& e, const IpmPlan& p, const std::vector<int>& params) {
  IpmSensTable t;
  std::string why;
  const int P = int(params.size());
  CHECK(ipm_sens_table(p, e.nnz_h, e.hes_i.data(), e.hes_j.data(), P, params.data(), &t, &why) == RPM_OK);
  CHECK(ipm_sens_table(p, e.nnz_h, e.hes_i.data(), e.hes_j.data(), P, params.data(), nullptr, &why) == RPM_OK);   // check only
  const int G = t.n_groups();
  CHECK(int(t.ptr.size()) == G + 1 && int(t.par.size()) == G && t.ptr[0] == 0 && t.ptr[size_t(G)] == int(t.src.size()));
  std::vector<char> is_fixed_pos(size_t(p.Nt_alloc), 0), is_slack_pos(size_t(p.Nt_alloc), 0);
  for (int i = 0; i < p.n; ++i)
    if (p.fixed[size_t(i)]) is_fixed_pos[size_t(p.pos[size_t(i)])] = 1;
  for (int s = 0; s < p.ns; ++s) is_slack_pos[size_t(p.pos[size_t(p.n + s)])] = 1;
  int g = 0;
  for (int k = 0; k < P; ++k) {
    const int j = params[size_t(k)];
    std::map<int, std::vector<int>> want;   // KKT position -> sources in ascending order: Hessian triplets, then Jacobian ones
    for (int q = 0; q < e.nnz_h; ++q) {
      const int a = e.hes_i[size_t(q)], c = e.hes_j[size_t(q)];
      if (a != j && c != j) continue;
      const int other = a == j ? c : a;
      if (p.fixed[size_t(other)]) continue;   // (the parameter's own diagonal included)
      want[p.pos[size_t(other)]].push_back(q);
    }
    for (int q = 0; q < e.nnz_jac; ++q)
      if (e.jac_j[size_t(q)] == j) want[p.pos[size_t(p.nv + e.jac_i[size_t(q)])]].push_back((1 << 28) | q);
    CHECK(!want.empty());
    for (const auto& w : want) {   // (a map walks its keys in ascending order: the order of the table's groups)
      CHECK(g < G && t.par[size_t(g)] == k && t.dst[size_t(g)] == w.first);
      CHECK(w.first >= 0 && w.first < p.Nt_alloc && !is_fixed_pos[size_t(w.first)] && !is_slack_pos[size_t(w.first)]);
      const std::vector<int> got(t.src.begin() + t.ptr[size_t(g)], t.src.begin() + t.ptr[size_t(g) + 1]);
      CHECK(got == w.second);
      for (size_t i = 1; i < got.size(); ++i) CHECK(got[i] > got[i - 1]);
      sources_walked += long(got.size());
      long_groups += got.size() > 1;
      ++g;
    }
  }
  CHECK(g == G);
  groups_walked += G;
  // the same input again: the same table
  IpmSensTable t2;
  CHECK(ipm_sens_table(p, e.nnz_h, e.hes_i.data(), e.hes_j.data(), P, params.data(), &t2, &why) == RPM_OK);
  CHECK(t2.ptr == t.ptr && t2.par == t.par && t2.dst == t.dst && t2.src == t.src);
}

void check_refusals(const Engine& e, const IpmPlan& p, const std::vector<int>& params) {
  auto refused = [&](int n_par, const int* list, const char* text) {
    IpmSensTable t;
    t.dst.push_back(7);   // a refusal leaves the caller's table alone
    std::string why;
    CHECK(ipm_sens_table(p, e.nnz_h, e.hes_i.data(), e.hes_j.data(), n_par, list, &t, &why) == RPM_E_INVALID);
    if (why.find(text) == std::string::npos) std::printf("message \"%s\" lacks \"%s\"\n", why.c_str(), text);
    CHECK(why.find(text) != std::string::npos && t.dst.size() == 1 && t.ptr.empty());
    CHECK(ipm_sens_table(p, e.nnz_h, e.hes_i.data(), e.hes_j.data(), n_par, list, nullptr, nullptr) == RPM_E_INVALID);
  };
  int free_var = -1;
  for (int i = 0; i < p.n && free_var < 0; ++i)
    if (!p.fixed[size_t(i)]) free_var = i;
  CHECK(free_var >= 0);
  const int j = params[0];
  refused(1, nullptr, "var_index is NULL");
  refused(0, params.data(), "outside 1 .. 32");
  refused(IPM_SENS_MAX_PAR + 1, params.data(), "outside 1 .. 32");
  refused(-3, params.data(), "outside 1 .. 32");
  const int low[1] = {-1}, high[2] = {j, p.n}, twice[3] = {j, j, j}, with_free[2] = {j, free_var};
  refused(1, low, "is outside the");
  refused(2, high, "is outside the");
  refused(2, twice, "listed twice");
  refused(2, with_free, ("variable " + std::to_string(free_var) + " ").c_str());
  refused(2, with_free, "is free in the solver's plan");
}

void run_case(const char* name, int problem_id, int n_consts, const std::vector<PhaseShape>& shapes, int links_of, int K, int nk, int nested,
              const std::vector<int>& param_offsets_phase0, bool with_t0, bool with_tf) {
  Engine e;
  make_engine(e, problem_id, n_consts, shapes, links_of, K, nk);
  synthetic_hessian(e);
  IpmPlan p;
  std::string why;
  const int rc = build_ipm_plan(e, p, &why, nested);
  if (rc) std::printf("build_ipm_plan (%s): %s\n", name, why.c_str());
  CHECK(rc == RPM_OK && p.nd == nested);
  const PhaseDev& q = e.phd[0];
  std::vector<int> params;
  for (int i : param_offsets_phase0) params.push_back(q.x_state0 + i * (q.N + 1));   // the variables rpm_ipm_set_initial_states writes
  if (with_t0) params.push_back(q.x_t0);
  if (with_tf) params.push_back(q.x_t0 + 1);
  for (int j : params) CHECK(p.fixed[size_t(j)]);
  const long before = groups_walked;
  check_table(e, p, params);
  check_refusals(e, p, params);
  // one parameter at a time: the groups of a parameter do not depend on the rest of the list
  for (int j : params) check_table(e, p, std::vector<int>{j});
  std::vector<int> reversed(params.rbegin(), params.rend());
  check_table(e, p, reversed);
  std::printf("%s: n %d, m %d, %zu parameters, %ld groups\n", name, p.n, p.m, params.size(), groups_walked - before);
}
}  // namespace

int main() {
  std::vector<int> all12(12), seven(7);
  for (int i = 0; i < 12; ++i) all12[size_t(i)] = i;
  for (int i = 0; i < 7; ++i) seven[size_t(i)] = i;
  const PhaseShape quad{12, 4, 0, 0, true, true, std::vector<int>(12, 1)};
  run_case("quadrotor 2x4 band", RPM_PROBLEM_QUADROTOR, 15, {quad}, 0, 2, 4, 0, all12, false, true);
  run_case("quadrotor 2x4 nested", RPM_PROBLEM_QUADROTOR, 15, {quad}, 0, 2, 4, 1, all12, false, true);
  const PhaseShape bd{3, 1, 0, 5, true, false, std::vector<int>(3, 0)};
  run_case("bryson_denham 2x8", RPM_PROBLEM_BRYSON_DENHAM, 0, {bd}, 0, 2, 8, 0, {}, true, false);
  // launch: phase 1 starts from fixed states, all times but the last tf are fixed, 7 linkages between consecutive phases
  const PhaseShape l1{7, 3, 1, 0, true, true, std::vector<int>(7, 1)}, l2{7, 3, 1, 0, true, true, std::vector<int>(7, 0)},
      l4{7, 3, 1, 5, true, false, std::vector<int>(7, 0)};
  run_case("launch 2x5 band", RPM_PROBLEM_LAUNCH, 22, {l1, l2, l2, l4}, 7, 2, 5, 0, seven, false, false);
  run_case("launch 2x5 nested", RPM_PROBLEM_LAUNCH, 22, {l1, l2, l2, l4}, 7, 2, 5, 1, seven, false, false);
  CHECK(long_groups > 0);   // sums of several sources were met
  std::printf("ok: %ld groups, %ld sources, %ld groups of more than one source\n", groups_walked, sources_walked, long_groups);
  return 0;
}
