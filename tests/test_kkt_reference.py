"""The reference of the KKT factorisation tests (tests/_kkt_reference.py) on its own, without a GPU: the long-double LDL'
reproduces its matrix, its inertia is that of the eigenvalues, a correct float64 implementation of the same elimination (the
twin) meets the growth-aware bound  rho_E <= 8 (3 Nt + 1) G 2^-53  with G <= 1e4 on the graded quasi-definite recipe the device
tests use — so bound and input condition can be met — and a twin with one panel update skipped misses it by more than 1e6."""
import numpy as np
import pytest

import _kkt_reference as kr

LD = kr.LD
NB, HB, NBORDER = 150, 20, 9            # a synthetic band + border envelope: Nb % 16 != 0, b > 16, nb < 16
SIGMA_RANGE = (-8.0, 2.0)               # exponents of Sigma_i (the device tests record theirs)
SEEDS = [0, 1, 2, 3]


def _envelope():
    """the envelope and the signs in elimination order: per node 6 primal unknowns then 4 dual ones, as the solver orders a
    collocation node (variables, slacks, multipliers); the border 5 primal, 4 dual"""
    inside = kr.envelope_band_border(NB, HB, NBORDER)
    sign = np.ones(NB + NBORDER)
    sign[:NB] = np.tile([1.0] * 6 + [-1.0] * 4, NB // 10)
    sign[NB:] = [1, 1, 1, 1, 1, -1, -1, -1, -1]
    return inside, sign


@pytest.fixture(scope="module")
def graded():
    """the graded matrices, their long-double factors and G, once for the module"""
    inside, sign = _envelope()
    out = []
    for seed in SEEDS:
        rng = np.random.RandomState(seed)
        K = kr.graded_kkt(inside, sign, rng, *SIGMA_RANGE)
        b = rng.uniform(-1, 1, size=sign.size)
        L, D = kr.ldlt(K)
        out.append(dict(K=K, b=b, L=L, D=D, G=kr.block_gain(L), sign=sign))
    return out


def test_ldlt_reproduces_its_matrix(graded):
    for c in graded:
        K, L, D = LD(c["K"]), c["L"], c["D"]
        E = kr.growth(L, D)
        err = np.abs((L * D) @ L.T - K)
        # every entry is a sum of at most Nt products, each rounded once in long double (2^-64), and the updates of the elimination
        assert (err <= 4 * K.shape[0] * 2.0 ** -64 * E).all(), float((err / np.maximum(E, LD(1e-300))).max())
        assert kr.reconstruction_error(L, D, K) <= 4 * K.shape[0] * 2.0 ** -64
        assert np.array_equal(np.triu(L, 1), np.zeros_like(L)) and (np.diagonal(L) == 1).all()
        x = kr.solve(L, D, c["b"])
        assert kr.rho_E(K, c["b"], x, L, D) <= 8 * (3 * K.shape[0] + 1) * 2.0 ** -64


def test_inertia_is_that_of_the_eigenvalues(graded):
    rng = np.random.RandomState(5)
    # well-scaled symmetric matrices with clear margins: quasi-definite with k primal signs flipped
    inside, sign = _envelope()
    for flips in (0, 1, 3):
        K = kr.graded_kkt(inside, sign, rng, -1.0, 1.0, delta_c=0.5)
        idx = rng.choice(np.nonzero(sign > 0)[0], size=flips, replace=False)
        K[idx, idx] *= -1.0
        L, D = kr.ldlt(K)
        G = kr.block_gain(L)
        counts, margin = kr.inertia(D, kr.growth_diagonal(L, D), kr.bound(sign.size, G))
        w = np.linalg.eigvalsh(K)
        assert margin >= kr.MARGIN_MIN and np.abs(w).min() > 1e-6 * np.abs(w).max(), (margin, np.abs(w).min())
        assert counts == (int((w > 0).sum()), int((w < 0).sum()), 0), (flips, counts)
        counts2, margin2 = kr.inertia(D, kr.growth(L, D), kr.bound(sign.size, G))                # E as a matrix (a float64 product)
        assert counts2 == counts and abs(margin2 - margin) <= 1e-12 * margin
    for c in graded:                 # the graded ones are quasi-definite: (primal, dual) whatever the order
        counts, margin = kr.inertia(c["D"], kr.growth_diagonal(c["L"], c["D"]), kr.bound(c["sign"].size, c["G"]))
        assert counts == (int((c["sign"] > 0).sum()), int((c["sign"] < 0).sum()), 0) and margin >= kr.MARGIN_MIN, (counts, margin)


def test_block_gain_of_known_blocks():
    assert kr.block_gain(np.eye(40)) == 1.0
    L = np.eye(20)
    L[5, 4] = 1e3                    # one large multiplier: |L^-1||L| has 2e3 in that row, + the unit diagonal
    assert abs(kr.block_gain(L) - (2e3 + 1)) < 1e-9
    L = np.eye(40)
    L[30, 10] = 1e6                  # 20 positions apart: inside no window of 16
    assert kr.block_gain(L) == 1.0
    M = np.tril(np.random.RandomState(1).uniform(-1, 1, (16, 16)), -1) + np.eye(16)
    assert np.abs(kr.unit_lower_inverse(M) @ LD(M) - np.eye(16)).max() < 1e-15


def test_twin_meets_the_bound_and_a_broken_twin_does_not(graded):
    print()
    for seed, c in zip(SEEDS, graded):
        nt = c["b"].size
        assert c["G"] <= kr.G_MAX, (seed, c["G"])                       # the input condition, from the reference alone
        limit = kr.bound(nt, c["G"])
        x, _, _ = kr.twin_solve(c["K"], c["b"])
        r, old = kr.both_measures(c["K"], c["b"], x, c["L"], c["D"])
        # one panel update skipped: column 40's update of the rows 48 .. 63, which the envelope couples to it
        assert np.count_nonzero(c["L"][48:64, 40]) >= 4
        xb, _, _ = kr.twin_solve(c["K"], c["b"], skip=(40, 48, 64))
        rb, oldb = kr.both_measures(c["K"], c["b"], xb, c["L"], c["D"])
        print("seed %d: Nt %d G %.2e bound %.2e | twin rho_E %.2e old %.2e | broken twin rho_E %.2e old %.2e"
              % (seed, nt, c["G"], limit, r, old, rb, oldb))
        assert r <= limit, (seed, r, limit)
        assert rb > 1e6 * limit, (seed, rb, limit)
