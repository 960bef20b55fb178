// rpm_hess.cpp — exact-Hessian mode, host side: given the per-phase dependency patterns (probed on the
// device by ensure_hessian), build the lower-triangular COO structure and the tables the Hessian kernels
// index with.  Order and counts follow LpHessianCalculator::GetPhaseHessianSparsity (Core/LpHessian.cpp:601-876),
// GetLinkHessianSparsity (:2369-2508) and GetHessianSparsity (:2510-2600) for nq = 0; duplicates between the
// collocation part (I) and the endpoint part (E) are intentional (Ipopt sums them).  Phases with static parameters
// (hessian-approximation = exact-parameters) add the parameter rows in the reference's block order (:810-872, :2405-2507) with
// the indices it means, not the ones it writes.
#include "rpm_engine.hpp"

namespace rpm {

void build_hessian_tables(Engine& e) {
  e.hess_pairs.clear();
  e.hess_phases.assign(e.P, HessPhaseDev{});
  e.hess_ends.clear();
  e.hess_links.clear();
  e.hess_red_dst.clear();
  e.hes_i.clear();
  e.hes_j.clear();
  int v = 0, tmp = 0;
  for (int ip = 0; ip < e.P; ++ip) {
    const PhaseHost& p = e.ph[ip];
    const int nx = p.nx, nu = p.nu, nq = p.nq, nc = p.nc, nv = nx + nu, nout = nx + nc, N = p.N, sh = p.var0;
    const std::vector<int>& dep = e.hess_dep[ip];
    // H = dep' * dep with unit diagonal (LpHessian.cpp:899-903)
    std::vector<int> H(size_t(nv) * nv, 0);
    int nnzH = 0;
    for (int a = 0; a < nv; ++a)
      for (int b = 0; b < nv; ++b) {
        int acc = 0;
        for (int r = 0; r < nout; ++r) acc += dep[r + size_t(a) * nout] * dep[r + size_t(b) * nout];
        if (a == b) acc = 1;
        H[a + size_t(b) * nv] = acc;
        if (acc) ++nnzH;
      }
    HessPhaseDev& q = e.hess_phases[ip];
    q.pair0 = int(e.hess_pairs.size());
    q.v0 = v;
    q.nI = N * ((nnzH - nx - nu) / 2 + nx + nu) + 2 * (nx + nu) * N + 3;
    q.nE = (2 * nx) * (2 * nx - 1) / 2 + 2 * nx + 4 * nx + 3;
    // parameter rows, always dense (:907-910)
    q.nI += nq * ((nx + nu) * N + 2) + nq * (nq + 1) / 2;
    q.nE += nq * (2 * nx + 2) + nq * (nq + 1) / 2;
    q.end0 = int(e.hess_ends.size());
    q.tt_tmp = tmp;
    q.red0 = int(e.hess_red_dst.size());
    q.n_red = 2 * nq + nq * (nq + 1) / 2;
    tmp += (3 + q.n_red) * N;
    // pair records in the fixed role order a*(a+1)/2 + b over [x.., u.., t, p..]
    const int NV = nv + 1 + nq;
    std::vector<HessPairDev> pairs(size_t(NV) * (NV + 1) / 2);
    for (int a = 0; a < NV; ++a)
      for (int b = 0; b <= a; ++b) pairs[size_t(a) * (a + 1) / 2 + b] = HessPairDev{a, b, 0, 0, 0};
    auto pair_of = [&](int a, int b) -> HessPairDev& { return pairs[size_t(a) * (a + 1) / 2 + b]; };
    std::vector<int> I_i(q.nI), I_j(q.nI), E_i(q.nE), E_j(q.nE);
    int sI = 0, sE = 0;
    auto block = [&](int rowstart, int colstart) {
      for (int k = 0; k < N; ++k) { I_i[sI] = sh + rowstart + k; I_j[sI++] = sh + colstart + k; }
    };
    auto rowblock = [&](int row, int colstart) {
      for (int k = 0; k < N; ++k) { I_i[sI] = sh + row; I_j[sI++] = sh + colstart + k; }
    };
    auto end_entry = [&](int a, int b, int da, int db, int row, int col) {
      e.hess_ends.push_back(HessEndDev{ip, a, b, da, db, q.nI + sE});
      E_i[sE] = sh + row;
      E_j[sE++] = sh + col;
    };
    for (int i = 0; i < nx; ++i)
      for (int j = 0; j <= i; ++j) {
        const int rs = i * (N + 1), cs = j * (N + 1);
        if (H[i + size_t(j) * nv]) {
          pair_of(i, j).kind = 1;
          pair_of(i, j).dst0 = sI;
          block(rs, cs);
        }
        end_entry(i, j, i, j, rs, cs);                         // x0_i, x0_j
        if (i != j) end_entry(i, nx + j, i, nx + i, rs, cs + N);   // x0_i, xf_j  (den pertx0(i)*pertxf(i), :1588)
        end_entry(nx + i, j, nx + i, j, rs + N, cs);           // xf_i, x0_j
        end_entry(nx + i, nx + j, nx + i, nx + i, rs + N, cs + N); // xf_i, xf_j  (den pertxf(i)*pertxf(i), :1612)
      }
    const int rowshift = nx * (N + 1);
    for (int i = 0; i < nu; ++i) {
      const int rs = rowshift + i * N;
      for (int j = 0; j < nx; ++j)
        if (H[(i + nx) + size_t(j) * nv]) {
          pair_of(nx + i, j).kind = 1;
          pair_of(nx + i, j).dst0 = sI;
          block(rs, j * (N + 1));
        }
      for (int j = 0; j <= i; ++j)
        if (H[(i + nx) + size_t(j + nx) * nv]) {
          pair_of(nx + i, nx + j).kind = 1;
          pair_of(nx + i, nx + j).dst0 = sI;
          block(rs, rowshift + j * N);
        }
    }
    const int trow = nx * (N + 1) + nu * N, T0 = 2 * nx, TF = 2 * nx + 1;
    for (int r = 0; r < 2; ++r) {
      const int row = trow + r, tv = r == 0 ? T0 : TF;
      for (int i = 0; i < nx; ++i) {
        HessPairDev& pr = pair_of(nv, i);
        pr.kind = 2;
        (r == 0 ? pr.dst0 : pr.dst1) = sI;
        rowblock(row, i * (N + 1));
        end_entry(tv, i, tv, i, row, i * (N + 1));
        end_entry(tv, nx + i, tv, nx + i, row, i * (N + 1) + N);
      }
      for (int i = 0; i < nu; ++i) {
        HessPairDev& pr = pair_of(nv, nx + i);
        pr.kind = 2;
        (r == 0 ? pr.dst0 : pr.dst1) = sI;
        rowblock(row, nx * (N + 1) + i * N);
      }
      if (r == 0) {
        q.tt_dst[0] = sI;
        I_i[sI] = sh + row; I_j[sI++] = sh + trow;
        end_entry(T0, T0, T0, T0, row, trow);
      } else {
        q.tt_dst[1] = sI;
        I_i[sI] = sh + row; I_j[sI++] = sh + trow;
        end_entry(TF, T0, TF, T0, row, trow);
        q.tt_dst[2] = sI;
        I_i[sI] = sh + row; I_j[sI++] = sh + trow + 1;
        end_entry(TF, TF, TF, TF, row, trow + 1);
      }
    }
    pair_of(nv, nv).kind = 3;
    // parameter rows (:810-872): per state N collocation entries and the two endpoint entries, per control N, then t0, tf and
    // the parameters up to the row's own, each once in the I-part (a sum over the nodes) and once in the E-part
    for (int i = 0; i < nq; ++i) {
      const int row = trow + 2 + i, pa = nv + 1 + i, PE = 2 * nx + 2;
      for (int j = 0; j < nx; ++j) {
        pair_of(pa, j).kind = 1;
        pair_of(pa, j).dst0 = sI;
        rowblock(row, j * (N + 1));
        end_entry(PE + i, j, PE + i, j, row, j * (N + 1));
        end_entry(PE + i, nx + j, PE + i, nx + j, row, j * (N + 1) + N);
      }
      for (int j = 0; j < nu; ++j) {
        pair_of(pa, nx + j).kind = 1;
        pair_of(pa, nx + j).dst0 = sI;
        rowblock(row, rowshift + j * N);
      }
      auto scalar = [&](int col, int end_b) {   // one reduced I entry (its scratch row is returned) and its E twin
        const int r = 3 + int(e.hess_red_dst.size()) - q.red0;
        e.hess_red_dst.push_back(sI);
        I_i[sI] = sh + row; I_j[sI++] = sh + col;
        end_entry(PE + i, end_b, PE + i, end_b, row, col);
        return r;
      };
      HessPairDev& pt = pair_of(pa, nv);
      pt.kind = 4;
      pt.dst0 = scalar(trow, T0);
      pt.dst1 = scalar(trow + 1, TF);
      for (int j = 0; j <= i; ++j) {
        HessPairDev& pp = pair_of(pa, nv + 1 + j);
        pp.kind = 5;
        pp.dst0 = scalar(trow + 2 + j, PE + j);
      }
    }
    q.n_end = int(e.hess_ends.size()) - q.end0;
    e.hess_pairs.insert(e.hess_pairs.end(), pairs.begin(), pairs.end());
    e.hes_i.insert(e.hes_i.end(), I_i.begin(), I_i.end());
    e.hes_j.insert(e.hes_j.end(), I_j.begin(), I_j.end());
    e.hes_i.insert(e.hes_i.end(), E_i.begin(), E_i.end());
    e.hes_j.insert(e.hes_j.end(), E_j.begin(), E_j.end());
    v += q.nI + q.nE;
  }
  for (int ip = 0; ip < e.L; ++ip) {
    const LinkDev& l = e.links[ip];
    const PhaseHost& pl = e.ph[l.left];
    const PhaseHost& pr = e.ph[l.right];
    const int nxl = pl.nx, nxr = pr.nx, nql = pl.nq, nqr = pr.nq;
    // link variables [xfL.., x0R.., pL.., pR..]; rows in the order xfL, pL, x0R, pR (:2405-2507)
    const int PL = nxl + nxr, PR = PL + nql;
    // the reference indexes the right phase's columns with nnodesLeft (:2463): kept where no phase has parameters
    const int NR = (nql == 0 && nqr == 0) ? pl.N : pr.N;
    auto xf_l = [&](int j) { return pl.var0 + (pl.N + 1) * (j + 1) - 1; };
    auto p_l = [&](int j) { return pl.var0 + pl.nx * (pl.N + 1) + pl.nu * pl.N + 2 + j; };
    auto p_r = [&](int j) { return pr.var0 + pr.nx * (pr.N + 1) + pr.nu * pr.N + 2 + j; };
    auto entry = [&](int a, int b, int row, int col) {
      e.hess_links.push_back(HessLinkDev{ip, a, b, v++});
      e.hes_i.push_back(row);
      e.hes_j.push_back(col);
    };
    for (int i = 0; i < nxl; ++i)
      for (int j = 0; j <= i; ++j) entry(i, j, xf_l(i), xf_l(j));
    for (int i = 0; i < nql; ++i) {
      for (int j = 0; j < nxl; ++j) entry(PL + i, j, p_l(i), xf_l(j));
      for (int j = 0; j <= i; ++j) entry(PL + i, PL + j, p_l(i), p_l(j));
    }
    for (int i = 0; i < nxr; ++i) {
      const int row = pr.var0 + (pr.N + 1) * i;
      for (int j = 0; j < nxl; ++j) entry(j, nxl + i, row, xf_l(j));   // hLink_xfL_x0R(j,i): first xfL_j, then x0R_i
      for (int j = 0; j < nql; ++j) entry(nxl + i, PL + j, row, p_l(j));
      for (int j = 0; j <= i; ++j) entry(nxl + i, nxl + j, row, pr.var0 + (NR + 1) * j);
    }
    for (int i = 0; i < nqr; ++i) {
      for (int j = 0; j < nxl; ++j) entry(PR + i, j, p_r(i), xf_l(j));
      for (int j = 0; j < nql; ++j) entry(PR + i, PL + j, p_r(i), p_l(j));
      for (int j = 0; j < nxr; ++j) entry(PR + i, nxl + j, p_r(i), pr.var0 + (pr.N + 1) * j);   // the reference loops j < nxL
      for (int j = 0; j <= i; ++j) entry(PR + i, PR + j, p_r(i), p_r(j));
    }
  }
  e.nnz_h = v;
  e.hess_tmp_len = tmp;
  e.hess_ready = true;
}

}  // namespace rpm
