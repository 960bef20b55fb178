// rpm_ipm_tables.cpp — the index tables rpm_ipm_create uploads beside the plan (host side of row f-2, see rpm_ipm.hpp): the
// factorisation's sub-problems, the long Jacobian columns, the ascending list of every structural slot (one-pass fill) and the
// per-interval-block tables of the fill fused into kkt_factor_dense_kernel; and the source table of the sensitivity right-hand sides
// (rpm_ipm_sens.hip), with the check of its parameter list, and the column table of the sensitivities to the constants, with the
// check of theirs.  Pure functions of the plan: no engine, no device.
#include <algorithm>
#include <unordered_map>

#include "rpm_ipm.hpp"

namespace rpm {

IpmSubList ipm_sub_list(const IpmPlan& p) {
  IpmSubList s;
  if (p.nd) {
    for (const KktSubHost& g : p.subs) s.subs.push_back(KktSub{KktGeom{g.Nt, g.Nb, g.nb, g.b, g.CS}, g.roff, g.koff});
    s.n_l2 = p.n_l2;
    s.n_l1 = int(s.subs.size()) - 1 - s.n_l2;
  } else {
    s.subs.push_back(KktSub{KktGeom{p.Nt, p.Nb, p.nb, p.b, p.CS}, 0, 0});
  }
  for (const KktSub& q : s.subs) s.max_sub_nt = std::max(s.max_sub_nt, q.g.Nt);
  return s;
}

std::vector<int> ipm_long_columns(const IpmPlan& p) {
  std::vector<int> cols;
  for (int i = 0; i < p.n; ++i)
    if (p.jt_ptr[size_t(i) + 1] - p.jt_ptr[size_t(i)] > IPM_LONG_COLUMN) cols.push_back(i);
  return cols;
}

IpmFillList ipm_fill_list(const IpmPlan& p) {
  struct Ent { int dst, ki, hg; };
  std::vector<Ent> ents;
  ents.reserve(p.hg_dst.size() + p.jac_dst.size() + p.slk_dst.size() + p.diag_dst.size());
  std::unordered_map<int, int> var_of_slot;
  for (int i = 0; i < p.nv; ++i) var_of_slot.emplace(p.diag_dst[size_t(i)], i);
  std::vector<int> hg_of_var(size_t(p.nv), -1);   // a Hessian slot on a variable's diagonal is written with that diagonal
  bool ok = p.hg_dst.size() < (1u << 28) && p.jac_dst.size() < (1u << 28) && p.diag_dst.size() < (1u << 28) && p.storage() < (1ll << 31);
  for (size_t i = 0; i < p.hg_dst.size(); ++i) {
    auto it = var_of_slot.find(p.hg_dst[i]);
    if (it != var_of_slot.end()) hg_of_var[size_t(it->second)] = int(i);
    else ents.push_back(Ent{p.hg_dst[i], (0 << 28) | int(i), -1});
  }
  for (size_t k = 0; k < p.jac_dst.size(); ++k)
    if (p.jac_dst[k] >= 0) ents.push_back(Ent{p.jac_dst[k], (1 << 28) | int(k), -1});
  for (size_t s = 0; s < p.slk_dst.size(); ++s) ents.push_back(Ent{p.slk_dst[s], (2 << 28) | int(s), -1});
  for (int i = 0; i < p.nv; ++i) ents.push_back(Ent{p.diag_dst[size_t(i)], (3 << 28) | i, hg_of_var[size_t(i)]});
  for (int r = 0; r < p.m; ++r) ents.push_back(Ent{p.diag_dst[size_t(p.nv + r)], (4 << 28) | r, -1});
  std::sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) { return a.dst < b.dst; });
  for (size_t i = 1; i < ents.size() && ok; ++i) ok = ents[i].dst != ents[i - 1].dst;   // two writers of one slot: keep the two-kernel path
  for (const Ent& en : ents) ok = ok && en.dst >= 0 && en.dst < p.storage();

  IpmFillList f;
  f.one_pass = ok;
  f.dst.resize(ents.size()); f.ki.resize(ents.size()); f.hg.resize(ents.size());
  for (size_t i = 0; i < ents.size(); ++i) { f.dst[i] = ents[i].dst; f.ki[i] = ents[i].ki; f.hg[i] = ents[i].hg; }
  if (ok) {
    const int nchunk = int((p.storage() + IPM_FILL_CHUNK - 1) / IPM_FILL_CHUNK);
    f.ptr.assign(size_t(nchunk) + 1, 0);
    size_t e = 0;
    for (int c = 0; c <= nchunk; ++c) {
      while (e < ents.size() && ents[e].dst < (long long)c * IPM_FILL_CHUNK) ++e;
      f.ptr[size_t(c)] = int(e);
    }
    f.ptr[size_t(nchunk)] = int(ents.size());
  }
  return f;
}

IpmFusedFill ipm_fused_fill(const IpmSubList& s, const IpmFillList& fill) {
  IpmFusedFill none, t;
  if (!fill.one_pass || s.n_l1 <= 0) return none;
  for (int si = 0; si < s.n_l1; ++si) {
    const int rows = s.subs[size_t(si)].g.block_rows();
    if (rows > IPM_DENSE_ROWS + IPM_DENSE_EARLY) return none;   // the kernel's register tiles do not hold the block
    t.tiles = std::max(t.tiles, ipm_dense_tiles_of(rows));
  }
  // per block the Jacobian entries first, then the Hessian slots, then the rest (slack entries, diagonals): three plain loops in the kernel
  t.ptr.assign(3 * size_t(s.n_l1) + 1, 0);
  t.map.assign(size_t(s.n_l1) * t.tiles * 64, 0ull);
  std::vector<char> skip(size_t(fill.n_chunks()), 0);
  const size_t n_ent = fill.dst.size();
  size_t e2 = 0;
  for (int si = 0; si < s.n_l1; ++si) {
    const KktGeom g = s.subs[size_t(si)].g;
    const long long k0 = s.subs[size_t(si)].koff, k1 = k0 + (long long)g.Nt * g.CS;
    const int nbb = (g.Nb + IPM_W - 1) / IPM_W, NTB = g.block_rows();
    while (e2 < n_ent && fill.dst[e2] < k0) ++e2;     // (level-1 blocks come first in the storage, in order)
    size_t e3 = e2;
    while (e3 < n_ent && fill.dst[e3] < k1) ++e3;
    int number = 0;
    for (int cls = 0; cls < 3; ++cls) {
      t.ptr[3 * size_t(si) + size_t(cls)] = int(t.ki.size());
      for (size_t q = e2; q < e3; ++q) {
        const int kind = fill.ki[q] >> 28;
        if ((kind == 1 ? 0 : (kind == 0 ? 1 : 2)) != cls) continue;
        const long long o = fill.dst[q] - k0;
        const int j = int(o / g.CS), slot = int(o % g.CS);
        const int i = (j < g.Nb && slot <= g.b) ? j + slot : g.Nb + slot - (g.b + 1);
        const bool band = i < g.Nb;
        if (i < j || i >= g.Nt || (band && (j >= g.Nb || i - j > g.b)) || (long long)g.at(i, j) != o) return none;
        const int I = band ? i / IPM_W : nbb + (i - g.Nb) / IPM_W, Kb = j < g.Nb ? j / IPM_W : nbb + (j - g.Nb) / IPM_W;
        const int lr = i - (I < nbb ? IPM_W * I : g.Nb + IPM_W * (I - nbb)), cc = j - (Kb < nbb ? IPM_W * Kb : g.Nb + IPM_W * (Kb - nbb));
        const int tile = ipm_dense_tile(NTB, I, Kb);
        if (tile >= t.tiles || ++number > 0xffff) return none;
        t.map[(size_t(si) * t.tiles + tile) * 64 + size_t((cc & 3) * 16 + lr)] |= (unsigned long long)number << (16 * (cc >> 2));
        t.ki.push_back(fill.ki[q]);
        t.hg.push_back(fill.hg[q]);
      }
    }
    e2 = e3;
    // the values wait in the panel's LDS space (2 x block rows x 16 rows of IPM_DENSE_LDS_ROW doubles), slot 0 is the zero
    if (size_t(number) + 1 > 2 * size_t(NTB) * IPM_W * IPM_DENSE_LDS_ROW) return none;
    for (long long c = (k0 + IPM_FILL_CHUNK - 1) / IPM_FILL_CHUNK; (c + 1) * IPM_FILL_CHUNK <= k1; ++c) skip[size_t(c)] = 1;
  }
  t.ptr[3 * size_t(s.n_l1)] = int(t.ki.size());
  for (int c = 0; c < fill.n_chunks(); ++c)
    if (!skip[size_t(c)]) t.live.push_back(c);
  t.built = true;
  return t;
}

int ipm_sens_table(const IpmPlan& p, int nnz_h, const int* hes_i, const int* hes_j, int n_par, const int* var_index, IpmSensTable* t,
                   std::string* why) {
  auto refuse = [&](const std::string& msg) { if (why) *why = msg; return int(RPM_E_INVALID); };
  if (!var_index) return refuse("var_index is NULL");
  if (n_par < 1 || n_par > IPM_SENS_MAX_PAR)
    return refuse("n_par = " + std::to_string(n_par) + " is outside 1 .. " + std::to_string(IPM_SENS_MAX_PAR));
  std::vector<int> par_of(size_t(p.n), -1);
  for (int k = 0; k < n_par; ++k) {
    const int j = var_index[k];
    if (j < 0 || j >= p.n) return refuse("var_index[" + std::to_string(k) + "] = " + std::to_string(j) + " is outside the " + std::to_string(p.n) + " variables");
    if (par_of[size_t(j)] >= 0) return refuse("variable " + std::to_string(j) + " is listed twice (var_index[" + std::to_string(par_of[size_t(j)]) + "] and [" + std::to_string(k) + "])");
    if (!p.fixed[size_t(j)]) return refuse("variable " + std::to_string(j) + " (var_index[" + std::to_string(k) + "]) is free in the solver's plan: sensitivities are taken to fixed variables");
    par_of[size_t(j)] = k;
  }
  if (!t) return RPM_OK;   // the list alone was to be checked (the predictor's entry points)
  struct Ent { int par, dst, src; };
  std::vector<Ent> ents;
  // Hessian triplets {i, j_k} with i free, each once per parameter it touches (two fixed ends: nothing, for either)
  for (int e = 0; e < nnz_h; ++e) {
    const int a = hes_i[e], c = hes_j[e];
    if (par_of[size_t(a)] >= 0 && !p.fixed[size_t(c)]) ents.push_back(Ent{par_of[size_t(a)], p.pos[size_t(c)], (0 << 28) | e});
    if (par_of[size_t(c)] >= 0 && !p.fixed[size_t(a)]) ents.push_back(Ent{par_of[size_t(c)], p.pos[size_t(a)], (0 << 28) | e});
  }
  // the Jacobian column of every parameter (jt_*: entries of a column in triplet order)
  for (int k = 0; k < n_par; ++k)
    for (int q = p.jt_ptr[size_t(var_index[k])]; q < p.jt_ptr[size_t(var_index[k]) + 1]; ++q)
      ents.push_back(Ent{k, p.pos[size_t(p.nv + p.jt_row[size_t(q)])], (1 << 28) | p.jt_ent[size_t(q)]});
  std::sort(ents.begin(), ents.end(), [](const Ent& x, const Ent& y) {
    return x.par != y.par ? x.par < y.par : (x.dst != y.dst ? x.dst < y.dst : x.src < y.src);
  });
  IpmSensTable out;
  for (size_t i = 0; i < ents.size(); ++i) {
    if (i == 0 || ents[i].par != ents[i - 1].par || ents[i].dst != ents[i - 1].dst) {
      out.ptr.push_back(int(i));
      out.par.push_back(ents[i].par);
      out.dst.push_back(ents[i].dst);
    }
    out.src.push_back(ents[i].src);
  }
  out.ptr.push_back(int(ents.size()));
  *t = std::move(out);
  return RPM_OK;
}

IpmConstTable ipm_const_table(const IpmPlan& p, int nnz_nl) {
  IpmConstTable t;
  t.ptr.push_back(0);
  for (int i = 0; i < p.n; ++i) {
    if (p.fixed[size_t(i)]) continue;
    t.var.push_back(i);
    t.var_pos.push_back(p.pos[size_t(i)]);
    for (int q = p.jt_ptr[size_t(i)]; q < p.jt_ptr[size_t(i) + 1]; ++q)   // (jt_*: the entries of a column in triplet order)
      if (p.jt_ent[size_t(q)] < nnz_nl) {
        t.ent.push_back(p.jt_ent[size_t(q)]);
        t.ent_row.push_back(p.jt_row[size_t(q)]);
      }
    t.ptr.push_back(int(t.ent.size()));
  }
  for (int r = 0; r < p.m; ++r) t.row_pos.push_back(p.pos[size_t(p.nv + r)]);
  return t;
}

int ipm_const_list_check(int nconst, int n_par, const int* const_index, std::string* why) {
  auto refuse = [&](const std::string& msg) { if (why) *why = msg; return int(RPM_E_INVALID); };
  if (nconst <= 0) return refuse("the problem functor takes no constants");
  if (!const_index) return refuse("const_index is NULL");
  if (n_par < 1 || n_par > IPM_SENS_MAX_PAR)
    return refuse("n_par = " + std::to_string(n_par) + " is outside 1 .. " + std::to_string(IPM_SENS_MAX_PAR));
  std::vector<int> par_of(size_t(nconst), -1);
  for (int k = 0; k < n_par; ++k) {
    const int j = const_index[k];
    if (j < 0 || j >= nconst) return refuse("const_index[" + std::to_string(k) + "] = " + std::to_string(j) + " is outside the " + std::to_string(nconst) + " constants");
    if (par_of[size_t(j)] >= 0) return refuse("constant " + std::to_string(j) + " is listed twice (const_index[" + std::to_string(par_of[size_t(j)]) + "] and [" + std::to_string(k) + "])");
    par_of[size_t(j)] = k;
  }
  return RPM_OK;
}

}  // namespace rpm
