"""A sweep's constraint multipliers carried onto another mesh (rpm_carry_multipliers_batch*, rpm_sweep_carry_multipliers).

The reference is written here, in numpy with np.longdouble: per instance and phase the knots 2 (time[k] - time[0]) / (time[N] -
time[0]) - 1 from x's t0 and tf, the costate columns c_k = -(1 / w_k) lambda[g0 + s N + k] with c_N = -D(:, N)' lambda_s, the
path-multiplier densities p_k = (1 / w_k) lambda[g0 + N nx + j N + k] with their value at tau = 1 from the natural spline through
the N points, the natural cubic spline through the N + 1 knots evaluated at the target's points, and the target's weight put back
on.  The device runs the solution carry's own spline in double (cubes A * A * A), the reference's cubes are exact, so the
comparison is by the bound test_sweep_carry.py applies to this spline, 1e-12 * max(1, max|reference column|), per column and as
densities lambda'_j / w'_j.  Event rows and the rows after the last phase are copies: bit for bit.  Every other comparison
(carry_tile values, batch against single instances, host against device form, a replayed graph, shares) is bit for bit.
Inputs: the seeded iterates of test_sweep_carry.py and lambda = RandomState(100 + b).standard_normal(m); nothing depends on a solve.

Measured worst |carried - reference| / max(1, max|reference column|) on the MI355X (bound 1e-12): hypersensitive 1x2 -> 1x5
1.2e-16; oscillator -> 1x2 per phase 5.4e-14, -> its own mesh 5.2e-14; quadrotor 4x6 -> ragged 1.1e-14, -> coarse 8.9e-15;
launch 8x8 -> ragged 1.2e-13.
"""
import ctypes as C

import numpy as np
import pytest

import test_sweep_carry as sc
from lpopc_amd import problems
from lpopc_amd.engine import ABI_SYMBOLS, NLPEngine, RpmError, lib
from lpopc_amd.group import SweepGroup

LD = np.longdouble
NEW_SYMBOLS = ["rpm_carry_multipliers_batch_dev", "rpm_carry_multipliers_batch", "rpm_carry_multipliers_layout", "rpm_sweep_carry_multipliers"]
TILES = (0, 1, 2, 4, 8)
CASES = [("hypersensitive", "one_by_five"), ("oscillator", "one_by_two"), ("oscillator", "same"), ("quadrotor", "ragged"),
         ("quadrotor", "coarse"), ("launch", "ragged")]


# ---- layout and inputs ------------------------------------------------------------------------------------------
def _rows(eng):
    """Per phase (g0, N, nx, nc, ne), from the problem description alone; and the first row after the phases."""
    out, g0 = [], 0
    for p in range(eng.n_phases):
        d = eng._desc.phases[p]
        N = int(sum(d.nodes_per_interval[i] for i in range(d.n_intervals)))
        out.append((g0, N, d.nx, d.nc, d.ne))
        g0 += N * (d.nx + d.nc) + d.ne
    return out, g0


def _lambdas(B, m):
    lam = np.stack([np.random.RandomState(100 + b).standard_normal(m) for b in range(B)])
    lam.setflags(write=False)
    return lam


def _d_last_column(t, N):
    """D(:, N) of a phase as a dense N-vector from the triplets of phase_tables"""
    r, c, v = t["d_rows"].astype(np.int64), t["d_cols"].astype(np.int64), t["d_vals"]
    if c.max() == N + 1:              # 1-based triplets
        r, c = r - 1, c - 1
    assert c.max() == N and r.max() == N - 1
    col = np.zeros(N)
    col[r[c == N]] = v[c == N]
    return col


# ---- the long-double reference ----------------------------------------------------------------------------------
def _d2(xk, Y):
    """second derivatives of the natural cubic splines through (xk, Y[:, c])"""
    M = len(xk)
    mu, z = np.zeros(M, dtype=LD), np.zeros_like(Y)
    for i in range(1, M - 1):
        him1, hi = xk[i] - xk[i - 1], xk[i + 1] - xk[i]
        alpha = LD(3) / hi * (Y[i + 1] - Y[i]) - LD(3) / him1 * (Y[i] - Y[i - 1])
        li = 2 * (xk[i + 1] - xk[i - 1]) - him1 * mu[i - 1]
        mu[i] = hi / li
        z[i] = (alpha - him1 * z[i - 1]) / li
    c = np.zeros_like(Y)
    for j in range(M - 2, -1, -1):
        c[j] = z[j] - mu[j] * c[j + 1]
    return 2 * c


def _eval(xk, Y, d2, x):
    M = len(xk)
    k = np.clip(np.searchsorted(xk, x, side="right"), 1, M - 1)
    h = (xk[k] - xk[k - 1])[:, None]
    A, Bc = (xk[k][:, None] - x[:, None]) / h, (x[:, None] - xk[k - 1][:, None]) / h
    return A * Y[k - 1] + Bc * Y[k] + ((A ** 3 - A) * d2[k - 1] + (Bc ** 3 - Bc) * d2[k]) * (h * h) / 6


def _reference(src, to, xs, lam):
    """-> B x to.m in long double, rows of the defect and path blocks as DENSITIES lambda' / w' (other rows: NaN)"""
    rf, _ = _rows(src)
    rt, _ = _rows(to)
    xcols = sc._layout(src)
    B = len(xs)
    ref = np.full((B, to.m), np.nan, dtype=LD)
    for p in range(src.n_phases):
        tf_, tt_ = src.phase_tables(p), to.phase_tables(p)
        g0, N, nx, nc, ne = rf[p]
        g0t, Nt, _, _, _ = rt[p]
        off, Nx, nx_, nu, nq = xcols[p]
        assert (Nx, nx_) == (N, nx)
        pts, w, tpts = tf_["points"].astype(LD), tf_["weights"].astype(LD), tt_["points"].astype(LD)
        dN = _d_last_column(tf_, N).astype(LD)
        it0 = off + nx * (N + 1) + nu * N
        for b in range(B):
            t0, tf = LD(xs[b, it0]), LD(xs[b, it0 + 1])
            time = (tf - t0) * (np.append(pts, LD(1)) + 1) / 2 + t0
            knots = 2 * (time - time[0]) / (time[N] - time[0]) - 1
            lb = lam[b].astype(LD)
            Y = np.zeros((N + 1, nx + nc), dtype=LD)
            for s in range(nx):
                ls = lb[g0 + s * N:g0 + (s + 1) * N]
                Y[:N, s] = -(ls / w)
                Y[N, s] = -np.sum(dN * ls)
            for j in range(nc):
                lj = lb[g0 + N * nx + j * N:g0 + N * nx + (j + 1) * N]
                Y[:N, nx + j] = lj / w
            if nc:        # the value at tau = 1: the natural spline through the N points, its last piece continued
                P = Y[:N, nx:]
                Y[N, nx:] = _eval(pts, P, _d2(pts, P), np.array([1], dtype=LD))[0]
            V = _eval(knots, Y, _d2(knots, Y), tpts)                  # Nt x (nx + nc)
            for s in range(nx):
                ref[b, g0t + s * Nt:g0t + (s + 1) * Nt] = -V[:, s]    # density of lambda' = -w' c: lambda' / w' = -c
            for j in range(nc):
                ref[b, g0t + Nt * nx + j * Nt:g0t + Nt * nx + (j + 1) * Nt] = V[:, nx + j]
    return ref


_REF = {}


def _case(case, target):
    """-> (src, to, xs, lam, reference densities); the reference is computed once per case and shared"""
    src, to, xs = sc._pair(case, target)
    lam = _lambdas(len(xs), src.m)
    if (case, target) not in _REF:
        ref = _reference(src, to, xs, lam)
        ref.setflags(write=False)
        _REF[(case, target)] = ref
    return src, to, xs, lam, _REF[(case, target)]


def _blocks(eng):
    """-> (list of (slice of a defect / path column, phase), indices of the copied rows: events and the tail)"""
    rows, tail0 = _rows(eng)
    cols, copied = [], []
    for p, (g0, N, nx, nc, ne) in enumerate(rows):
        cols += [(slice(g0 + c * N, g0 + (c + 1) * N), p) for c in range(nx + nc)]
        copied += list(range(g0 + N * (nx + nc), g0 + N * (nx + nc) + ne))
    copied += list(range(tail0, eng.m))
    return cols, np.array(copied, dtype=np.int64)


# ---- without a device -------------------------------------------------------------------------------------------
def test_symbols_exist_and_are_listed(built):
    L = lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    assert L.rpm_carry_multipliers_batch_dev.argtypes == [vp, vp, vp, vp, vp, vp, vp]
    assert L.rpm_carry_multipliers_batch.argtypes == [vp, vp, dp, dp, dp, ip]


@pytest.mark.parametrize("make,B", [(sc._ragged_oscillator, 9), (lambda: problems.launch(8, 8), 5), (lambda: problems.quadrotor(4, 6), 3)])
def test_row_map_adds_up_to_m(built, make, B):
    """from == to: phase rows + the rows after the phases = m, and every block sits where the description says"""
    eng = NLPEngine(make(), n_instances=B)
    lay = eng.carry_multipliers_layout()
    rows, tail0 = _rows(eng)
    total = 0
    for p, (g0, N, nx, nc, ne) in enumerate(rows):
        assert list(lay[p]) == [g0, g0 + N * nx, g0 + N * (nx + nc), g0 + N * (nx + nc) + ne]
        assert p == 0 or lay[p][0] == lay[p - 1][3]
        total += lay[p][3] - lay[p][0]
    assert list(lay[-1]) == [tail0, tail0, tail0, eng.m] and lay[-1][0] == lay[-2][3]
    n_links = sum(eng._desc.links[i].n_links for i in range(eng._desc.n_links))
    assert eng.m - tail0 >= n_links                     # the linkage rows (and the duration / linear rows) follow the phases
    assert total + (eng.m - tail0) == eng.m
    cols, copied = _blocks(eng)
    covered = np.zeros(eng.m, dtype=int)
    for c, _ in cols:
        covered[c] += 1
    covered[copied] += 1
    assert (covered == 1).all()                         # every row is carried exactly once
    with pytest.raises(RpmError):
        eng._check(eng._L.rpm_carry_multipliers_layout(eng._h, eng.n_phases + 1, lay[0].ctypes.data_as(C.POINTER(C.c_int))))
    eng.close()


def test_argument_errors_are_decided_on_the_host(built):
    L = lib()
    dp = C.POINTER(C.c_double)
    quad = NLPEngine(problems.quadrotor(3, 5), n_instances=4)
    fine = NLPEngine(problems.quadrotor(4, 6), n_instances=4)
    xf, lf, lt = np.zeros(4 * quad.n), np.zeros(4 * quad.m), np.zeros(4 * fine.m)
    px, pf, pt = (a.ctypes.data_as(dp) for a in (xf, lf, lt))

    def refused(fn, code, text, frm=quad):
        with pytest.raises(RpmError) as ei:
            fn()
        assert ei.value.code == code and text in str(ei.value), str(ei.value)
        assert text in frm.last_error()

    assert L.rpm_carry_multipliers_batch(quad._h, fine._h, px, None, pt, None) == 1 and "lambda_from is NULL" in quad.last_error()
    assert L.rpm_carry_multipliers_batch(quad._h, fine._h, px, pf, None, None) == 1 and "lambda_to is NULL" in quad.last_error()
    assert L.rpm_carry_multipliers_batch(quad._h, fine._h, None, pf, pt, None) == 1 and "x_from is NULL" in quad.last_error()
    assert L.rpm_carry_multipliers_batch(quad._h, None, px, pf, pt, None) == 1 and "target engine is NULL" in quad.last_error()
    assert L.rpm_carry_multipliers_batch_dev(quad._h, fine._h, C.c_void_p(8), None, C.c_void_p(8), None, None) == 1
    assert "d_lambda_from is NULL" in quad.last_error()
    assert L.rpm_carry_multipliers_batch_dev(quad._h, fine._h, C.c_void_p(8), C.c_void_p(8), None, None, None) == 1
    assert "d_lambda_to is NULL" in quad.last_error()
    assert L.rpm_carry_multipliers_batch(None, fine._h, px, pf, pt, None) == 1
    assert L.rpm_sweep_carry_multipliers(None, None, px, pf, pt, None) == 1
    # engines that do not match
    fewer = NLPEngine(problems.quadrotor(4, 6), n_instances=3)
    refused(lambda: quad.carry_multipliers_batch(fewer, xf, lf), 1, "n_instances differs (4 and 3)")
    hyper = NLPEngine(problems.hypersensitive([-1.0, 1.0], [4]), n_instances=4)
    refused(lambda: quad.carry_multipliers_batch(hyper, xf, lf), 1, "nx differs in phase 1")
    bd, br = NLPEngine(problems.bryson_denham(2, 4), n_instances=2), NLPEngine(problems.brachistochrone(2, 4), n_instances=2)
    refused(lambda: bd.carry_multipliers_batch(br, np.zeros(2 * bd.n), np.zeros(2 * bd.m)), 1, "different problems", bd)
    # overlapping lambda arrays, host and device pointers alike; in place
    assert L.rpm_carry_multipliers_batch_dev(quad._h, fine._h, C.c_void_p(8), C.c_void_p(4096), C.c_void_p(4096 + 8 * (4 * quad.m - 1)),
                                             None, None) == 1 and "overlap" in quad.last_error()
    assert L.rpm_carry_multipliers_batch_dev(quad._h, quad._h, C.c_void_p(8), C.c_void_p(4096), C.c_void_p(4096), None, None) == 1
    # interval sharding, a column that cannot fit, an unknown tile
    sh, whole = NLPEngine(problems.launch(8, 8), shard_mode=1, shard_rank=1, shard_world=2), NLPEngine(problems.launch(8, 8))
    refused(lambda: sh.carry_multipliers_batch(whole, np.zeros(sh.n), np.zeros(sh.m)), 2, "interval sharding", sh)
    quad.set_option("carry_lds_bytes", 8 * 16 * 3)
    refused(lambda: quad.carry_multipliers_batch(fine, xf, lf), 2, "a column of 16 knots does not fit one workgroup's LDS")
    quad.set_option("carry_lds_bytes", 0)
    with pytest.raises(RpmError):
        quad.set_option("carry_tile", 3)
    with pytest.raises(RpmError):
        quad.carry_multipliers_batch(fine, xf, lf[:-1])
    for e in (quad, fine, fewer, hyper, bd, br, sh, whole):
        e.close()


# ---- on the device ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case,target", CASES)
def test_against_the_long_double_reference(built, case, target):
    src, to, xs, lam, ref = _case(case, target)
    got, flags = src.carry_multipliers_batch(to, xs, lam)
    assert got.shape == (len(xs), to.m) and not flags.any() and np.isfinite(got).all()
    cols, copied = _blocks(to)
    _, copied_src = _blocks(src)
    assert np.array_equal(got[:, copied], lam[:, copied_src])               # events, linkages, the rest: to the bit
    if case in ("oscillator", "launch"):
        assert copied.size > 0 and any(r[3] for r in _rows(src)[0])         # events, linkages and a path constraint are covered
    W = [to.phase_tables(p)["weights"] for p in range(to.n_phases)]
    worst = 0.0
    for b in range(len(xs)):
        for c, p in cols:
            dens, want = got[b, c].astype(LD) / W[p].astype(LD), ref[b, c]
            scale = max(1.0, float(np.abs(want).max()))
            d = float(np.abs(dens - want).max())
            worst = max(worst, d / scale)
            assert d <= 1e-12 * scale, (case, target, b, c, d, scale)
    print("%s -> %s: worst |carried - long-double reference| / max(1, max|column|) = %.3e (bound 1e-12)" % (case, target, worst))
    if target == "same":                                                    # the spline returns its own knots
        for b in range(len(xs)):
            for c, p in cols:
                a, s = got[b, c] / W[p], lam[b, c] / W[p]
                assert np.abs(a - s).max() <= 1e-12 * max(1.0, np.abs(s).max()), (case, b, c)
    src.close()
    to.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case,target", CASES)
def test_every_tile_and_both_forms_give_the_same_bits(built, case, target):
    import torch
    src, to, xs = sc._pair(case, target)
    B = len(xs)
    lam = _lambdas(B, src.m)
    base, flags0 = src.carry_multipliers_batch(to, xs, lam)
    s = torch.cuda.Stream()
    d_x, d_l = torch.from_numpy(np.array(xs)).cuda(), torch.from_numpy(np.array(lam)).cuda()
    d_out = torch.empty((B, to.m), dtype=torch.float64, device="cuda")
    d_flag = torch.empty(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for tile in TILES:
        src.set_option("carry_tile", tile)
        got, flags = src.carry_multipliers_batch(to, xs, lam)
        assert np.array_equal(got, base) and np.array_equal(flags, flags0), tile
        d_out.fill_(float("nan"))
        d_flag.fill_(7)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            src.carry_multipliers_batch_dev(to, d_x, d_l, d_out, d_flag, stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), base) and np.array_equal(d_flag.cpu().numpy(), flags0), tile
    # the solution carry next to it is untouched by the multipliers' plan
    x_to, _ = src.carry_solution_batch(to, xs)
    assert np.isfinite(x_to).all()
    src.close()
    to.close()


@pytest.mark.gpu
def test_captured_graph_replayed_on_new_inputs(built):
    import torch
    src, to, xs = sc._pair("quadrotor", "ragged")
    B = len(xs)
    lam = _lambdas(B, src.m)
    s = torch.cuda.Stream()
    d_x, d_l = torch.from_numpy(np.array(xs)).cuda(), torch.from_numpy(np.array(lam)).cuda()
    d_out = torch.empty((B, to.m), dtype=torch.float64, device="cuda")
    d_flag = torch.empty(B, dtype=torch.int32, device="cuda")
    src.carry_multipliers_batch_dev(to, d_x, d_l, d_out, d_flag, stream=s.cuda_stream)      # the first call on the pair: the plan goes up
    s.synchronize()
    direct = d_out.cpu().numpy().copy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        src.carry_multipliers_batch_dev(to, d_x, d_l, d_out, d_flag, stream=s.cuda_stream)
    d_out.fill_(float("nan"))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), direct)
    lam2 = np.stack([np.random.RandomState(700 + b).standard_normal(src.m) for b in range(B)])
    d_l.copy_(torch.from_numpy(lam2).cuda())
    d_out.fill_(float("nan"))
    d_flag.fill_(7)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    want, flags = src.carry_multipliers_batch(to, xs, lam2)
    assert np.array_equal(d_out.cpu().numpy(), want) and np.array_equal(d_flag.cpu().numpy(), flags)
    del g
    src.close()
    to.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case,target", [("launch", "ragged"), ("oscillator", "one_by_two")])
def test_a_batch_equals_its_instances_carried_alone(built, case, target):
    src, to, xs = sc._pair(case, target)
    lam = _lambdas(len(xs), src.m)
    base, _ = src.carry_multipliers_batch(to, xs, lam)
    makers, _ = sc._source(case)
    tprobs = sc._target_probs(case, target)
    for b in range(len(xs)):
        a, t = NLPEngine(makers[b](), device=0), NLPEngine(tprobs[b], device=0)
        alone, flag = a.carry_multipliers_batch(t, xs[b], lam[b])
        assert np.array_equal(alone[0], base[b]) and flag[0] == 0, (case, b)
        a.close()
        t.close()
    src.close()
    to.close()


@pytest.mark.gpu
def test_sweep_group_equals_one_engine(built):
    makers, xs = sc._source("quadrotor")
    B = 7
    probs, tprobs = [m() for m in makers[:B]], sc._target_probs("quadrotor", "ragged")[:B]
    src, to = sc._batched(probs), sc._batched(tprobs)
    lam = _lambdas(B, src.m)
    want, flags = src.carry_multipliers_batch(to, xs[:B], lam)
    g_from, g_to = SweepGroup(probs[0], [0, 0, 0], B), SweepGroup(tprobs[0], [0, 0, 0], B)
    got, gflags = g_from.carry_multipliers(g_to, xs[:B], lam)
    assert np.array_equal(got, want) and np.array_equal(gflags, flags)
    two = SweepGroup(tprobs[0], [0, 0], B)
    with pytest.raises(RpmError) as ei:
        g_from.carry_multipliers(two, xs[:B], lam)
    assert ei.value.code == 1 and "different shares" in str(ei.value)
    for o in (g_from, g_to, two, src, to):
        o.close()


@pytest.mark.gpu
def test_a_nan_in_lambda_is_flagged_and_disturbs_nobody(built):
    src, to, xs = sc._pair("quadrotor", "coarse")
    B = len(xs)
    lam = _lambdas(B, src.m)
    clean, flags = src.carry_multipliers_batch(to, xs, lam)
    assert not flags.any()
    bad = np.array(lam)
    bad[17, 5] = np.nan
    bad[30, src.m - 1] = np.inf                      # a copied row
    got, flags = src.carry_multipliers_batch(to, xs, bad)
    want = np.zeros(B, dtype=np.int32)
    want[[17, 30]] = 1
    assert np.array_equal(flags, want)
    others = want == 0
    assert np.array_equal(got[others], clean[others])
    assert np.isnan(got[17]).any() and np.isinf(got[30]).any()
    src.close()
    to.close()
