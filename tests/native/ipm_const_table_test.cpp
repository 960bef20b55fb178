// CPU test of the column table of the sensitivities to the constants (ipm_const_table) and of the check of their list
// (ipm_const_list_check), lpopc_amd/csrc/rpm_ipm_tables.cpp, on the plans of quadrotor 2 x 4 (band and nested), launch 2 x 5 (four
// phases with linkages, a path constraint: slacks) and param_sled 4 x 8 (a static parameter, fixed and free).  Every entry is walked
// against a brute-force restatement — per free variable all Jacobian triplets of its column below nnz_nl in ascending order, their
// rows, positions through pos, nothing for a fixed variable — and every refusal is exercised.  With --dump the plan's inputs and
// the table go to stdout as lines of integers, for the numpy restatement of tests/test_ipm_constant_sensitivities.py.  Compiled
// (with the host-only rpm_setup.cpp, rpm_mesh.cpp, rpm_ipm.cpp, rpm_ipm_tables.cpp) and run by that file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../lpopc_amd/csrc/rpm_ipm.hpp"

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } \
  } while (0)

namespace rpm {
// the registry of the device library, for the problem ids this test uses (static dimensions only)
bool problem_dims(int problem_id, ProblemDims* out) {
  if (problem_id == RPM_PROBLEM_QUADROTOR) *out = ProblemDims{12, 4, 0, 0, 0, 15, false, 0};
  else if (problem_id == RPM_PROBLEM_LAUNCH) *out = ProblemDims{7, 3, 1, 5, 7, 22, false, 0};
  else if (problem_id == RPM_PROBLEM_PARAM_SLED) *out = ProblemDims{2, 1, 0, 4, 0, 1, false, 1};
  else return false;
  return true;
}
}  // namespace rpm

using namespace rpm;

namespace {

struct PhaseShape {
  int nx, nu, nq, nc, ne;
  bool tf_fixed, state0_fixed, parameter_fixed;
};

void make_engine(Engine& e, int problem_id, int n_consts, const std::vector<PhaseShape>& shapes, int links_of, int K, int nk) {
  const size_t P = shapes.size();
  std::vector<double> mesh(size_t(K) + 1);
  for (int i = 0; i <= K; ++i) mesh[size_t(i)] = i == K ? 1.0 : -1.0 + 2.0 * i / K;
  const std::vector<int> nodes(size_t(K), nk);
  std::vector<std::vector<double>> keep;   // the arrays the descriptions point into
  auto arr = [&](std::vector<double> v) { keep.push_back(std::move(v)); return keep.back().data(); };
  keep.reserve(20 * P + 8);
  std::vector<rpm_phase_desc> ph(P);
  const double tg[2] = {0, 1};
  for (size_t q = 0; q < P; ++q) {
    const PhaseShape& s = shapes[q];
    rpm_phase_desc& d = ph[q];
    d = rpm_phase_desc{};
    d.nx = s.nx; d.nu = s.nu; d.nq = s.nq; d.nc = s.nc; d.ne = s.ne;
    d.n_intervals = K; d.mesh_points = mesh.data(); d.nodes_per_interval = nodes.data();
    d.t0_min = d.t0_max = double(q);
    d.tf_min = double(q) + 1.0; d.tf_max = s.tf_fixed ? double(q) + 1.0 : double(q) + 3.0;
    std::vector<double> smin, smax;
    for (int i = 0; i < s.nx; ++i) {
      smin.insert(smin.end(), {s.state0_fixed ? 0.25 : -10.0, -10.0, -10.0});
      smax.insert(smax.end(), {s.state0_fixed ? 0.25 : 10.0, 10.0, 10.0});
    }
    d.state_min = arr(smin); d.state_max = arr(smax);
    d.control_min = arr(std::vector<double>(size_t(s.nu), -1.0)); d.control_max = arr(std::vector<double>(size_t(s.nu), 1.0));
    d.parameter_min = arr(std::vector<double>(size_t(s.nq) + 1, 0.5)); d.parameter_max = arr(std::vector<double>(size_t(s.nq) + 1, s.parameter_fixed ? 0.5 : 2.0));
    d.path_min = arr(std::vector<double>(size_t(s.nc) + 1, 0.0)); d.path_max = arr(std::vector<double>(size_t(s.nc) + 1, 1.0));   // inequalities: slacks
    d.event_min = arr(std::vector<double>(size_t(s.ne) + 1, 0.0)); d.event_max = arr(std::vector<double>(size_t(s.ne) + 1, 0.0));
    d.n_guess = 2; d.time_guess = tg;
    d.state_guess = arr(std::vector<double>(size_t(s.nx) * 2, 0.0));
    d.control_guess = arr(std::vector<double>(size_t(s.nu) * 2, 0.0));
    d.parameter_guess = arr(std::vector<double>(size_t(s.nq) + 1, 1.0));
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

bool dump = false;
long entries_walked = 0, columns_with_entries = 0, columns_cut = 0;

void line(const char* key, const std::vector<int>& v) {
  std::printf("%s", key);
  for (int x : v) std::printf(" %d", x);
  std::printf("\n");
}

void run_case(const char* name, int problem_id, int n_consts, const std::vector<PhaseShape>& shapes, int links_of, int K, int nk, int nested) {
  Engine e;
  make_engine(e, problem_id, n_consts, shapes, links_of, K, nk);
  IpmPlan p;
  std::string why;
  const int rc = build_ipm_plan(e, p, &why, nested);
  if (rc) std::printf("build_ipm_plan (%s): %s\n", name, why.c_str());
  CHECK(rc == RPM_OK && p.nd == nested);
  CHECK(e.nnz_nl > 0 && e.nnz_nl < e.nnz_jac);
  const IpmConstTable t = ipm_const_table(p, e.nnz_nl);
  const int F = t.n_free();
  CHECK(int(t.var_pos.size()) == F && int(t.ptr.size()) == F + 1 && t.ptr[0] == 0 && t.ptr[size_t(F)] == int(t.ent.size()));
  CHECK(t.ent_row.size() == t.ent.size() && int(t.row_pos.size()) == p.m);
  int u = 0, n_fixed = 0;
  for (int i = 0; i < p.n; ++i) {
    if (p.fixed[size_t(i)]) { ++n_fixed; continue; }
    CHECK(u < F && t.var[size_t(u)] == i && t.var_pos[size_t(u)] == p.pos[size_t(i)]);
    std::vector<int> want, want_row;
    int in_column = 0;
    for (int q = 0; q < e.nnz_jac; ++q)   // ascending triplet index
      if (e.jac_j[size_t(q)] == i) {
        ++in_column;
        if (q < e.nnz_nl) { want.push_back(q); want_row.push_back(e.jac_i[size_t(q)]); }
      }
    const std::vector<int> got(t.ent.begin() + t.ptr[size_t(u)], t.ent.begin() + t.ptr[size_t(u) + 1]);
    const std::vector<int> got_row(t.ent_row.begin() + t.ptr[size_t(u)], t.ent_row.begin() + t.ptr[size_t(u) + 1]);
    CHECK(got == want && got_row == want_row);
    entries_walked += long(got.size());
    columns_with_entries += !got.empty();
    columns_cut += int(got.size()) < in_column;
    ++u;
  }
  CHECK(u == F && F + n_fixed == p.n && n_fixed > 0);
  std::vector<char> seen(size_t(p.Nt_alloc), 0);
  for (int a = 0; a < F; ++a) { CHECK(!seen[size_t(t.var_pos[size_t(a)])]); seen[size_t(t.var_pos[size_t(a)])] = 1; }
  for (int r = 0; r < p.m; ++r) {
    CHECK(t.row_pos[size_t(r)] == p.pos[size_t(p.nv + r)] && !seen[size_t(t.row_pos[size_t(r)])]);
    seen[size_t(t.row_pos[size_t(r)])] = 1;
  }
  const IpmConstTable t2 = ipm_const_table(p, e.nnz_nl);   // the same input again: the same table
  CHECK(t2.var == t.var && t2.var_pos == t.var_pos && t2.ptr == t.ptr && t2.ent == t.ent && t2.ent_row == t.ent_row && t2.row_pos == t.row_pos);
  CHECK(ipm_const_table(p, 0).ent.empty());                // no state-dependent block: no triplets, the rows all the same
  if (dump) {
    std::printf("case %s\n", name);
    line("sizes", {p.n, p.m, p.nv, e.nnz_nl, e.nnz_jac});
    line("fixed", p.fixed);
    line("pos", p.pos);
    line("jac_i", e.jac_i);
    line("jac_j", e.jac_j);
    line("var", t.var); line("var_pos", t.var_pos); line("ptr", t.ptr); line("ent", t.ent); line("ent_row", t.ent_row); line("row_pos", t.row_pos);
  } else {
    std::printf("%s: n %d (%d fixed), m %d, %zu triplets of %d inside [NL]\n", name, p.n, n_fixed, p.m, t.ent.size(), e.nnz_nl);
  }
}

void check_list_refusals() {
  auto refused = [&](int nconst, int n_par, const int* list, const char* text) {
    std::string why;
    CHECK(ipm_const_list_check(nconst, n_par, list, &why) == RPM_E_INVALID);
    if (why.find(text) == std::string::npos) std::printf("message \"%s\" lacks \"%s\"\n", why.c_str(), text);
    CHECK(why.find(text) != std::string::npos);
    CHECK(ipm_const_list_check(nconst, n_par, list, nullptr) == RPM_E_INVALID);
  };
  std::vector<int> all(IPM_SENS_MAX_PAR + 1);
  for (int i = 0; i <= IPM_SENS_MAX_PAR; ++i) all[size_t(i)] = i;
  std::string why = "untouched";
  CHECK(ipm_const_list_check(40, IPM_SENS_MAX_PAR, all.data(), &why) == RPM_OK && why == "untouched");
  const int one[1] = {0};
  CHECK(ipm_const_list_check(1, 1, one, nullptr) == RPM_OK);
  refused(0, 1, one, "takes no constants");
  refused(15, 1, nullptr, "const_index is NULL");
  refused(40, 0, all.data(), "outside 1 .. 32");
  refused(40, IPM_SENS_MAX_PAR + 1, all.data(), "outside 1 .. 32");
  refused(40, -2, all.data(), "outside 1 .. 32");
  const int low[1] = {-1}, high[2] = {3, 15}, twice[3] = {7, 2, 7};
  refused(15, 1, low, "is outside the 15 constants");
  refused(15, 2, high, "const_index[1] = 15");
  refused(15, 3, twice, "constant 7 is listed twice (const_index[0] and [2])");
}

}  // namespace

int main(int argc, char** argv) {
  dump = argc > 1 && !std::strcmp(argv[1], "--dump");
  const PhaseShape quad{12, 4, 0, 0, 0, true, true, false};
  run_case("quadrotor_band", RPM_PROBLEM_QUADROTOR, 15, {quad}, 0, 2, 4, 0);
  run_case("quadrotor_nested", RPM_PROBLEM_QUADROTOR, 15, {quad}, 0, 2, 4, 1);
  const PhaseShape l1{7, 3, 0, 1, 0, true, true, false}, l2{7, 3, 0, 1, 0, true, false, false}, l4{7, 3, 0, 1, 5, false, false, false};
  run_case("launch_band", RPM_PROBLEM_LAUNCH, 22, {l1, l2, l2, l4}, 7, 2, 5, 0);
  run_case("launch_nested", RPM_PROBLEM_LAUNCH, 22, {l1, l2, l2, l4}, 7, 2, 5, 1);
  run_case("param_sled_fixed", RPM_PROBLEM_PARAM_SLED, 1, {PhaseShape{2, 1, 1, 0, 4, false, false, true}}, 0, 4, 8, 0);
  run_case("param_sled_free", RPM_PROBLEM_PARAM_SLED, 1, {PhaseShape{2, 1, 1, 0, 4, false, true, false}}, 0, 4, 8, 0);
  check_list_refusals();
  CHECK(columns_with_entries > 0 && columns_cut > 0);   // columns that reach into the linear or the constant block were met
  if (!dump) std::printf("ok: %ld triplets, %ld columns with triplets, %ld of them cut at the end of [NL]\n", entries_walked, columns_with_entries, columns_cut);
  else std::printf("ok: dumped\n");
  return 0;
}
