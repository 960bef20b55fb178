"""Reference of the pivot-free LDL^T of rpm_kkt_factor.hip / rpm_kkt_solve.hip, in numpy long double, and the growth-aware rule
its tests judge the device by.  Everything here works on a symmetric matrix ALREADY in elimination order
(Kp = P K P'): tests/test_kkt_factor_error.py and tests/test_ipm_pass.py permute with rpm_ipm_get_permutation.

    P K P' = L D L'  without pivoting,      E = |L| |D| |L'|
    rho_E(x) = max_i |K x - b|_i / ((E |x|)_i + |b|_i)
    G        = max over every window w of 16 consecutive positions of  || |L_w^-1| |L_w| ||_inf
    bound    = 8 (3 Nt + 1) G 2^-53

3 Nt + 1 is the constant of a factorisation and two substitutions (Higham, Accuracy and Stability, Theorem 10.4 with gamma_{3n+1});
G enters because the kernels apply the explicit inverse of every 16 x 16 diagonal block (Mi, Dg), whose block partition — in any
layout, at any level — is a set of such windows; the 8 is the project's usual allowance.  No condition number enters: a dropped or
misplaced product shows as rho_E of order 1e-8 .. 1, the bound is of order 1e-12 G.

The float64 twin is the same scalar elimination, same loop, same order, in np.float64: it sets no bound; its figures are printed
beside the device's to tell "the algorithm grows" from "a kernel drops a term".
"""
import numpy as np

from _ipm_pass_reference import LD, relative_residual   # noqa: F401  (the old |K||x| + |rhs| measure, kept where it was)

W = 16                      # IPM_W: the width of a diagonal block
U53 = 2.0 ** -53
G_MAX = 1e4                 # the input condition of every case
MARGIN_MIN = 100.0          # a pivot whose margin is below this is undecided


def bound(nt, G):
    return 8.0 * (3 * nt + 1) * float(G) * U53


def ldlt(Kp, dtype=LD, skip=None):
    """Unpivoted LDL' of a symmetric matrix, column by column, the rank-1 update of a column vectorised over the rows and columns
    the column reaches -> (L unit lower triangular, D).  Only the lower triangle is read.  skip = (k, r0, r1): the deliberately
    broken form — column k's update of the rows r0 .. r1 - 1 is left out (one panel update skipped)."""
    A = np.tril(np.array(Kp, dtype=dtype))
    n = A.shape[0]
    L, D = np.eye(n, dtype=dtype), np.zeros(n, dtype=dtype)
    for k in range(n):
        d = A[k, k]
        D[k] = d
        col = A[k + 1:, k]
        nz = np.nonzero(col)[0]
        if nz.size == 0:
            continue
        rows = k + 1 + nz
        a = col[nz]
        l = a / d
        L[rows, k] = l
        upd = np.tril(np.outer(l, a))                      # l_i d l_j, i >= j
        if skip is not None and skip[0] == k:
            upd[(rows >= skip[1]) & (rows < skip[2]), :] = 0
        A[np.ix_(rows, rows)] -= upd
    return L, D


def solve(L, D, b):
    """x of L D L' x = b by the two substitutions, in the factors' type"""
    n = D.size
    y = np.array(b, dtype=L.dtype)
    for k in range(n - 1):
        if y[k] != 0:
            y[k + 1:] -= L[k + 1:, k] * y[k]
    y = y / D
    for k in range(n - 2, -1, -1):
        y[k] -= L[k + 1:, k] @ y[k + 1:]
    return y


def growth_diagonal(L, D):
    """diag(E): E_kk = sum_j L_kj^2 |D_j|"""
    return (np.abs(L) ** 2) @ np.abs(D)


def growth(L, D):
    """E = |L| |D| |L'|, dense.  (A sum of non-negative terms: the product runs in float64, whose relative error (Nt + 2) 2^-53 is
    far inside the 8 of the bound; long double matrix products have no BLAS.)"""
    aL = np.abs(L).astype(np.float64)
    return LD((aL * np.abs(D).astype(np.float64)) @ aL.T)


def growth_times(L, D, x):
    """E |x| without forming E, in long double"""
    aL = np.abs(LD(L))
    return aL @ (np.abs(LD(D)) * (aL.T @ np.abs(LD(x))))


def block_gain(L):
    """G: the largest || |L_w^-1| |L_w| ||_inf over every window of W consecutive positions (every offset: whatever 16-wide block
    partition a layout has is among them; a shorter last block is the leading part of a window, whose rows it shares)."""
    L = LD(L)
    n = L.shape[0]
    w = min(W, n)
    starts = np.arange(n - w + 1)
    idx = starts[:, None] + np.arange(w)[None, :]
    Lw = L[idx[:, :, None], idx[:, None, :]]               # (windows, w, w)
    X = np.zeros_like(Lw)
    for i in range(w):                                     # forward substitution, all windows at once: X = L_w^-1
        X[:, i, :] = -np.einsum("nk,nkj->nj", Lw[:, i, :i], X[:, :i, :])
        X[:, i, i] += 1
    return float(np.einsum("nik,nkj->ni", np.abs(X), np.abs(Lw)).max())


def unit_lower_inverse(M, majorant=False):
    """inverse of a unit lower triangular block in long double (the device's L11^-1 back to L11).  majorant: the inverse of the
    comparison matrix (unit diagonal, -|M_ij| below it) instead, which bounds |M^-1| entrywise and is a sum of non-negative paths:
    it is positive wherever rounding can leave anything in the inverse."""
    M = np.abs(LD(M)) if majorant else -LD(M)
    w = M.shape[0]
    X = np.zeros_like(M)
    for i in range(w):
        X[i, :] = M[i, :i] @ X[:i, :]
        X[i, i] += 1
    return X


def band_border_factors(store, nt, Nb, b):
    """One instance's band + border storage after the factorisation (column j: slot i - j for a band row, b + 1 + i - Nb for a border
    row; rpm_ipm_debug_storage, or K of a stage-3 pass) -> (L_dev, D_dev) in elimination order, long double: d on the diagonal, L
    below it, and below the diagonal of every 16 x 16 diagonal block (counted from column 0 of the band part and again from column 0
    of the corner) L11^-1, which is inverted back here.  Where the exact L11 has a structural zero the stored inverse, rounded to
    float64 entry by entry, does not invert back to an exact zero: an entry of the re-inverted block below 16 * 2^-53 times the
    same entry of the inverse of the comparison matrix (unit_lower_inverse(majorant=True): every path counted with its magnitude,
    the most 16 roundings of the stored entries can leave) is such a zero and is set to 0, so that E_dev = |L_dev||D_dev||L_dev'|
    is the issue's plain one."""
    store = np.asarray(store)
    cs = store.size // nt
    L = np.zeros((nt, nt), dtype=LD)
    li, lj = np.tril_indices(nt)
    ok = ((li < Nb) & (li - lj <= b)) | (li >= Nb)
    li, lj = li[ok], lj[ok]
    L[li, lj] = store[lj * cs + np.where(li < Nb, li - lj, b + 1 + li - Nb)]
    D = np.diagonal(L).copy()
    L[np.arange(nt), np.arange(nt)] = 1
    for lo_, hi_ in ((0, Nb), (Nb, nt)):
        for c0 in range(lo_, hi_, W):
            c1 = min(c0 + W, hi_)
            M = L[c0:c1, c0:c1]
            X = unit_lower_inverse(M)
            X[np.abs(X) <= W * U53 * unit_lower_inverse(M, majorant=True)] = 0
            X[np.arange(c1 - c0), np.arange(c1 - c0)] = 1
            L[c0:c1, c0:c1] = X
    return L, D


def rho_E(Kp, bp, xp, L, D):
    """max_i |K x - b|_i / ((E |x|)_i + |b|_i) in long double; a row with a residual over a zero denominator counts as inf"""
    Kp, bp, xp = LD(Kp), LD(bp), LD(xp)
    num = np.abs(Kp @ xp - bp)
    den = growth_times(L, D, xp) + np.abs(bp)
    if not np.isfinite(np.asarray(xp, dtype=np.float64)).all():
        return float("inf")
    ok = den > 0
    if (num[~ok] > 0).any():
        return float("inf")
    return float((num[ok] / den[ok]).max()) if ok.any() else 0.0


def inertia(D, E, gamma):
    """(n_pos, n_neg, n_zero) from the signs of D and the smallest pivot margin |D_k| / (gamma E_kk): E the matrix or its diagonal,
    gamma the bound.  A margin far above 1 means no rounding of a correct factorisation can flip the sign."""
    D = LD(D)
    Ed = LD(E)
    Ed = np.diagonal(Ed) if Ed.ndim == 2 else Ed
    margin = float((np.abs(D) / (LD(gamma) * Ed)).min())
    return (int((D > 0).sum()), int((D < 0).sum()), int((D == 0).sum())), margin


def reconstruction_error(L, D, Kp):
    """max over the lower triangle of |L D L' - K|_ij / E_ij, E = |L||D||L'| of the SAME factors, both accumulated column by column
    over the entries a column holds (long double); an entry with E_ij = 0 must be reproduced exactly (inf otherwise)."""
    L, D, Kp = LD(L), LD(D), LD(Kp)
    n = D.size
    R, E = np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=LD)
    for k in range(n):
        rows = k + np.nonzero(L[k:, k])[0]
        l = L[rows, k]
        o = np.outer(l, l * D[k])
        R[np.ix_(rows, rows)] += o
        E[np.ix_(rows, rows)] += np.abs(o)
    low = np.tril(np.ones((n, n), dtype=bool))
    diff = np.abs(R - Kp)
    if (diff[low & (E == 0)] > 0).any():
        return float("inf")
    ok = low & (E > 0)
    return float((diff[ok] / E[ok]).max())


def twin_solve(Kp, bp, skip=None):
    """the float64 twin: factor and solve in np.float64 -> (x, L, D)"""
    L, D = ldlt(Kp, dtype=np.float64, skip=skip)
    return solve(L, D, np.asarray(bp, dtype=np.float64)), L, D


def both_measures(Kp, bp, xp, L, D):
    """(rho_E, the old figure) of a solution"""
    return rho_E(Kp, bp, xp, L, D), relative_residual(Kp, xp, bp)


# ---------------------------------------------------------------------------------------------------- matrices
def envelope_band_border(Nb, b, nb):
    """lower-triangle mask of a band + border envelope"""
    nt = Nb + nb
    ii, jj = np.tril_indices(nt, -1)
    inside = np.zeros((nt, nt), dtype=bool)
    keep = ((ii < Nb) & (ii - jj <= b)) | (ii >= Nb)
    inside[ii[keep], jj[keep]] = True
    return inside


def graded_kkt(inside, sign, rng, lo=-8.0, hi=12.0, delta_c=1e-9, keep_unlike=0.5):
    """The graded quasi-definite recipe, in unknown order: test_ipm.py's fill (every pair of unlike sign inside the envelope and 30 %
    of the others, half of them kept, values in (-1, 1)); the dual diagonal -delta_c (the production value, not a dominant one);
    the primal diagonal (the sum of the magnitudes of the row's primal entries + a margin in (0.5, 2)) + Sigma_i, Sigma_i =
    10^U(lo, hi): the grading z / d of a barrier matrix.  The dual x dual block is -delta_c I as in (13): the fill leaves it out
    (with -1e-9 on the diagonal an entry there makes the block indefinite and the matrix no longer quasi-definite).  Inertia
    (primal count, dual count) in any order (Vanderbei 1995)."""
    nt = sign.size
    ii, jj = np.tril_indices(nt, -1)
    ins = inside[ii, jj]
    unlike = sign[ii] != sign[jj]
    keep = ins & (unlike | (rng.rand(ii.size) < 0.3)) & (rng.rand(ii.size) < np.where(unlike, keep_unlike, 0.5))
    keep &= (sign[ii] > 0) | (sign[jj] > 0)
    A = np.zeros((nt, nt))
    A[ii[keep], jj[keep]] = rng.uniform(-1, 1, size=int(keep.sum()))
    A = A + A.T
    prim = sign > 0
    dom = (np.abs(A) * (prim[:, None] & prim[None, :])).sum(axis=1) + rng.uniform(0.5, 2.0, size=nt)
    sigma = 10.0 ** rng.uniform(lo, hi, size=nt)
    A[np.arange(nt), np.arange(nt)] = np.where(prim, dom + sigma, -delta_c)
    return A


def permuted(K, order):
    return np.asarray(K)[np.ix_(order, order)]
