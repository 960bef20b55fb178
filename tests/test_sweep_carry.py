"""A sweep's solutions carried onto another mesh (rpm_carry_solution_batch*, rpm_sweep_carry_solution).

The reference is the one-instance route that exists without the batched call: rpm_nlp2op_control per phase, the extracted
time / state / control / parameter arrays installed as the guess of a fresh problem on the target mesh (install_guess), a new
engine, rpm_get_starting_point.  The device repeats that route operation by operation except for the two cubes of every
spline evaluation (A * A * A on the device, glibc's pow(A, 3) on the host), so the comparison with it is by the project's
bound for quantities that pass through libm, 1e-12 * max(1, max|reference column|) per state and control column; t0, tf and
the static parameters must be equal to the bit.  Every other comparison (layouts, forms, streams, graphs, shares, batch
against single instances, the column split) is bit for bit.  On the same mesh the carried columns must also return the
source's own values at the source's own points within the same bound: the spline interpolates its knots, and the knots
2 (time[k] - time[0]) / (time[N] - time[0]) - 1 differ from the LGR points by a few ulp only.

The oracle pins the reference itself (no device): Oracle.nlp2op -> guess -> Oracle.starting_point on the same mesh returns
x to 4 * 2^-52 * max(1, |x_i|); measured worst on quadrotor 4x6 and launch 8x8, seeds 100 and 101: 2.2e-16 absolute and
relative.  Inputs are seeded iterates, a different seed per instance: nothing depends on a solve converging."""
import ctypes as C

import numpy as np
import pytest

from _hessian_cases import ragged_mesh
from lpopc_amd import problems
from lpopc_amd.engine import ABI_SYMBOLS, NLPEngine, RpmError, lib
from lpopc_amd.group import SweepGroup
from lpopc_amd.mesh import MeshRefiner, install_guess, install_sweep_mesh
from lpopc_amd.problem import Options

EPS = 2.0 ** -52
NEW_SYMBOLS = ["rpm_carry_solution_batch_dev", "rpm_carry_solution_batch", "rpm_sweep_carry_solution"]
TILES = (0, 1, 2, 4, 8)


# ---- problems, meshes, inputs -----------------------------------------------------------------------------------
def _ragged_oscillator():
    """The two-phase parameter oscillator (nq = 2) on ragged meshes: unequal widths, 3 to 19 nodes per interval."""
    p = problems.param_oscillator()
    _set_meshes(p, [([-1, -0.7, 0.2, 1], [4, 19, 3]), ([-1, 0.1, 1], [17, 5])])
    return p


def _set_meshes(prob, meshes):
    for i, (mesh, nodes) in enumerate(meshes):
        ph = prob.GetPhase(i)
        ph.meshpoints = [float(v) for v in mesh]
        ph.nodesperinterval = [int(v) for v in nodes]
    return prob


def _quadrotor_prefs(B):
    rng = np.random.RandomState(11)
    return [tuple(rng.uniform(-1.5, 1.5, size=3)) for _ in range(B)]


def _makers(name):
    """-> list of B callables, each building instance b's problem on the source mesh"""
    if name == "quadrotor":
        return [lambda p=p: problems.quadrotor(4, 6, pref=p) for p in _quadrotor_prefs(37)]
    if name == "launch":
        return [lambda: problems.launch(8, 8)] * 5
    if name == "oscillator":
        return [_ragged_oscillator] * 9
    return [lambda: problems.hypersensitive([-1.0, 1.0], [2])] * 3


ONE_BY_TWO = ([-1.0, 1.0], [2])
# target meshes per phase; "refined" is what ph_refine_sweep returns (needs the device), "same" the source's own mesh
TARGETS = {
    "quadrotor": {"refined": None, "same": None,
                  "ragged": [([-1.0, -0.6, -0.1, 0.3, 1.0], [5, 2, 7, 3])],      # holds a 2-node interval
                  "coarse": [([-1.0, 0.2, 1.0], [5, 5])]},                        # N' = 10 < N = 24
    "launch": {"ragged": [ragged_mesh(n) for n in ([5, 2], [8], [4, 5, 3], [6, 7, 6])]},
    "oscillator": {"one_by_two": [ONE_BY_TWO, ONE_BY_TWO]},
    "hypersensitive": {"one_by_two": [ONE_BY_TWO], "one_by_five": [([-1.0, 1.0], [5])]},
}
CASE_TARGETS = [(c, t) for c in TARGETS for t in TARGETS[c]]


def _batched(probs, device=0):
    eng = NLPEngine(probs[0], n_instances=len(probs), device=device)
    for b in range(1, len(probs)):
        c = probs[b].GetOpimalProblemFuns().consts
        if len(c):
            eng.set_instance_constants(b, c)
    return eng


def _iterates(probs, seed0=100):
    one = NLPEngine(probs[0])
    xl, xu, _, _ = one.get_bounds_info()
    x0 = one.get_starting_point()
    one.close()
    return np.stack([problems.seeded_iterate(x0, xl, xu, seed0 + b) for b in range(len(probs))])


def _layout(eng):
    """Per phase (offset of the phase in x, N, nx, nu, nq)."""
    out, off = [], 0
    for p in range(eng.n_phases):
        d = eng._desc.phases[p]
        N = eng.phase_tables(p)["points"].size
        out.append((off, N, d.nx, d.nu, d.nq))
        off += d.nx * (N + 1) + d.nu * N + 2 + d.nq
    assert off == eng.n
    return out


def _columns(eng):
    """-> (list of slices, one per state and control column; indices of t0, tf and the parameters; of the parameters alone)"""
    cols, scal, par = [], [], []
    for off, N, nx, nu, nq in _layout(eng):
        cols += [slice(off + s * (N + 1), off + (s + 1) * (N + 1)) for s in range(nx)]
        u0 = off + nx * (N + 1)
        cols += [slice(u0 + j * N, u0 + (j + 1) * N) for j in range(nu)]
        scal += list(range(u0 + nu * N, u0 + nu * N + 2 + nq))
        par += list(range(u0 + nu * N + 2, u0 + nu * N + 2 + nq))
    return cols, np.array(scal), np.array(par, dtype=np.int64)


_SRC, _MESH, _REF = {}, {}, {}


def _source(case):
    """-> (makers, xs): built once per case and never changed"""
    if case not in _SRC:
        makers = _makers(case)
        xs = _iterates([m() for m in makers])
        xs.setflags(write=False)
        _SRC[case] = (makers, xs)
    return _SRC[case]


def _meshes(case, target):
    if (case, target) not in _MESH:
        makers, xs = _source(case)
        probs = [m() for m in makers]
        if target == "refined":
            eng = _batched(probs)
            res = eng.ph_refine_sweep(xs, 1e-6, 4, 16)
            eng.close()
            meshes = [(m.tolist(), [int(v) for v in n]) for _, m, n, _ in res]
            assert sum(meshes[0][1]) > 24                    # it really asks for more nodes
        elif target == "same":
            meshes = [(list(probs[0].GetPhase(i).GetMeshPoints()), list(probs[0].GetPhase(i).GetNodesPerInterval()))
                      for i in range(probs[0].GetPhaseNum())]
        else:
            meshes = TARGETS[case][target]
        _MESH[(case, target)] = meshes
    return _MESH[(case, target)]


def _target_probs(case, target):
    makers, _ = _source(case)
    return [_set_meshes(m(), _meshes(case, target)) for m in makers]


def _reference(case, target):
    """The one-instance route of the parent commit, instance by instance -> B x to.n; computed once and shared."""
    if (case, target) not in _REF:
        makers, xs = _source(case)
        meshes = _meshes(case, target)
        rows = []
        for b, make in enumerate(makers):
            one = NLPEngine(make(), device=0)
            fresh = make()
            install_guess(one, fresh, x=xs[b], lam=np.zeros(one.m))
            _set_meshes(fresh, meshes)
            nxt = NLPEngine(fresh)
            rows.append(nxt.get_starting_point())
            nxt.close()
            one.close()
        ref = np.stack(rows)
        ref.setflags(write=False)
        _REF[(case, target)] = ref
    return _REF[(case, target)]


def _pair(case, target):
    makers, xs = _source(case)
    src = _batched([m() for m in makers])
    to = _batched(_target_probs(case, target))
    return src, to, xs


# ---- without a device -------------------------------------------------------------------------------------------
def test_symbols_exist_and_are_listed(built):
    L = lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in ABI_SYMBOLS, s


def test_argument_errors_are_decided_on_the_host(built):
    L = lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    quad = NLPEngine(problems.quadrotor(3, 5), n_instances=4)
    fine = NLPEngine(problems.quadrotor(4, 6), n_instances=4)
    xf, xt = np.zeros(4 * quad.n), np.zeros(4 * fine.n)
    pf, pt = xf.ctypes.data_as(dp), xt.ctypes.data_as(dp)

    def refused(fn, code, text, frm=quad):
        with pytest.raises(RpmError) as ei:
            fn()
        assert ei.value.code == code and text in str(ei.value), str(ei.value)
        assert text in frm.last_error()

    # NULL arrays and a NULL target, both forms
    assert L.rpm_carry_solution_batch(quad._h, fine._h, None, pt, None) == 1 and "x_from is NULL" in quad.last_error()
    assert L.rpm_carry_solution_batch(quad._h, fine._h, pf, None, None) == 1 and "x_to is NULL" in quad.last_error()
    assert L.rpm_carry_solution_batch(quad._h, None, pf, pt, None) == 1 and "target engine is NULL" in quad.last_error()
    assert L.rpm_carry_solution_batch_dev(quad._h, fine._h, None, C.c_void_p(8), None, None) == 1 and "d_x_from is NULL" in quad.last_error()
    assert L.rpm_carry_solution_batch_dev(quad._h, fine._h, C.c_void_p(8), None, None, None) == 1 and "d_x_to is NULL" in quad.last_error()
    assert L.rpm_carry_solution_batch(None, fine._h, pf, pt, None) == 1
    assert L.rpm_sweep_carry_solution(None, None, pf, pt, None) == 1
    # engines that do not match
    fewer = NLPEngine(problems.quadrotor(4, 6), n_instances=3)
    refused(lambda: quad.carry_solution_batch(fewer, xf), 1, "n_instances differs (4 and 3)")
    hyper = NLPEngine(problems.hypersensitive([-1.0, 1.0], [4]), n_instances=4)
    refused(lambda: quad.carry_solution_batch(hyper, xf), 1, "nx differs in phase 1")
    sled, osc = NLPEngine(problems.param_sled(2, 4), n_instances=2), NLPEngine(_ragged_oscillator(), n_instances=2)
    assert (sled._desc.phases[0].nx, sled._desc.phases[0].nu) == (osc._desc.phases[0].nx, osc._desc.phases[0].nu)
    assert (sled._desc.phases[0].nq, osc._desc.phases[0].nq) == (1, 2)
    refused(lambda: sled.carry_solution_batch(osc, np.zeros(2 * sled.n)), 1, "nq differs in phase 1", sled)
    refused(lambda: osc.carry_solution_batch(sled, np.zeros(2 * osc.n)), 1, "nq differs in phase 1", osc)
    bd, br = NLPEngine(problems.bryson_denham(2, 4), n_instances=2), NLPEngine(problems.brachistochrone(2, 4), n_instances=2)
    refused(lambda: bd.carry_solution_batch(br, np.zeros(2 * bd.n)), 1, "different problems", bd)
    # overlapping arrays (host and device pointers alike: the ranges are compared before anything else happens)
    both = np.zeros(4 * (quad.n + fine.n))
    p0 = both.ctypes.data
    ov = C.cast(C.c_void_p(p0 + 8 * (4 * quad.n - 1)), dp)        # x_to starts on x_from's last double
    assert L.rpm_carry_solution_batch(quad._h, fine._h, both.ctypes.data_as(dp), ov, None) == 1 and "overlap" in quad.last_error()
    assert L.rpm_carry_solution_batch_dev(quad._h, fine._h, C.c_void_p(4096), C.c_void_p(4096 + 8 * (4 * quad.n - 1)), None, None) == 1
    assert "overlap" in quad.last_error()
    assert L.rpm_carry_solution_batch_dev(quad._h, quad._h, C.c_void_p(4096), C.c_void_p(4096), None, None) == 1     # in place
    # interval sharding, on either side
    sh = NLPEngine(problems.launch(8, 8), shard_mode=1, shard_rank=1, shard_world=2)
    whole = NLPEngine(problems.launch(8, 8))
    refused(lambda: sh.carry_solution_batch(whole, np.zeros(sh.n)), 2, "interval sharding", sh)
    refused(lambda: whole.carry_solution_batch(sh, np.zeros(whole.n)), 2, "interval sharding", whole)
    # a column that cannot fit one workgroup's LDS (the budget is an option for exactly this and the column split)
    assert quad.get_option("carry_groups") == 1
    quad.set_option("carry_lds_bytes", 8 * 16 * 3)           # N + 1 = 16 knots, padded to 17: one column needs 5 rows
    assert quad.get_option("carry_groups") == 0
    refused(lambda: quad.carry_solution_batch(fine, xf), 2, "a column of 16 knots does not fit one workgroup's LDS")
    quad.set_option("carry_lds_bytes", 8 * 17 * 5)           # exactly one column of one instance
    assert quad.get_option("carry_groups") == 16
    quad.set_option("carry_lds_bytes", 0)
    with pytest.raises(RpmError):
        quad.set_option("carry_tile", 3)
    for e in (quad, fine, fewer, hyper, sled, osc, bd, br, sh, whole):
        e.close()


def test_no_gpu_means_loud_failure_not_fallback(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    a, b = NLPEngine(problems.quadrotor(3, 5), n_instances=2), NLPEngine(problems.quadrotor(4, 6), n_instances=2)
    with pytest.raises(RpmError) as ei:
        a.carry_solution_batch(b, np.zeros(2 * a.n))
    assert ei.value.code == 3 and "no CPU fallback" in str(ei.value)
    a.close()
    b.close()


def test_the_planner_splits_columns_before_it_refuses(built):
    """Host only: the number of workgroups per tile of instances under a shrinking LDS budget (quadrotor 4 x 6: 25 knots,
    row stride 25 doubles, 16 columns; a workgroup holds 1 + 2 TB + 2 TB c rows for c columns of TB instances)."""
    eng = NLPEngine(problems.quadrotor(4, 6), n_instances=37)
    rows = lambda tb, c: 1 + 2 * tb + 2 * tb * c        # noqa: E731
    for tile, budget_rows, groups in ((2, rows(2, 16), 1), (2, rows(2, 16) - 1, 2), (2, rows(2, 8), 2), (2, rows(2, 2), 8),
                                      (8, rows(8, 3), 6), (8, rows(8, 1) - 1, 8),       # 8 do not fit: 4 instances, 2 columns
                                      (1, rows(1, 1), 16), (1, rows(1, 1) - 1, 0)):
        eng.set_option("carry_tile", tile)
        eng.set_option("carry_lds_bytes", 8 * 25 * budget_rows)
        assert eng.get_option("carry_groups") == groups, (tile, budget_rows)
    eng.close()


class _Recorded:
    """What MeshRefiner.RefineMesh asks its engine: ph_refine_mesh per phase, answered from a recording."""

    def __init__(self, result):
        self.result = result

    def ph_refine_mesh(self, phase, tol, nmin, nmax, x=None):
        return self.result[phase]


@pytest.mark.parametrize("done", [(False, True, False, True), (True, True, True, True)])
def test_install_sweep_mesh_writes_what_refine_mesh_writes(done):
    result = []
    for i, nodes in enumerate(([5, 2], [8], [4, 5, 3], [6, 7, 6])):
        mesh, nk = ragged_mesh(nodes)
        result.append((done[i], np.array(mesh), np.array(nk, dtype=np.int32), np.zeros(len(nk))))
    a, b = problems.launch(8, 8), problems.launch(8, 8)
    no_more = MeshRefiner(Options()).RefineMesh(_Recorded(result), a)
    assert install_sweep_mesh(b, result) == no_more == all(done)
    for i in range(4):
        pa, pb = a.GetPhase(i), b.GetPhase(i)
        assert pa.GetMeshPoints() == pb.GetMeshPoints() and pa.GetNodesPerInterval() == pb.GetNodesPerInterval()
        assert [type(v) for v in pb.GetMeshPoints()] == [float] * len(pb.GetMeshPoints())
        assert [type(v) for v in pb.GetNodesPerInterval()] == [int] * len(pb.GetNodesPerInterval())
    # the engines built from the two problems are the same transcription
    ea, eb = NLPEngine(a), NLPEngine(b)
    assert (ea.n, ea.m) == (eb.n, eb.m) and np.array_equal(ea.get_starting_point(), eb.get_starting_point())
    ea.close()
    eb.close()
    with pytest.raises(Exception):
        install_sweep_mesh(b, result[:3])


class _OracleRoute:
    """install_guess's view of an engine, answered by the oracle."""

    def __init__(self, orc):
        self.orc = orc

    def nlp2op_control(self, phase, x=None, lam=None):
        return self.orc.nlp2op(phase, x, lam)


@pytest.mark.parametrize("name", ["quadrotor", "launch"])      # nq = 0 only: Oracle.nlp2op is not built for parameters
def test_the_reference_chain_returns_x_on_the_same_mesh(built, name):
    from oracle.oracle import Oracle
    make = (lambda: problems.quadrotor(4, 6)) if name == "quadrotor" else (lambda: problems.launch(8, 8))
    xs = _iterates([make(), make()])
    worst_abs = worst_rel = 0.0
    for x in xs:
        orc = Oracle(make())
        fresh = make()
        install_guess(_OracleRoute(orc), fresh, x=x, lam=np.zeros(orc.m))
        back = Oracle(fresh).starting_point()
        d = np.abs(back - x)
        worst_abs, worst_rel = max(worst_abs, d.max()), max(worst_rel, (d / np.maximum(1.0, np.abs(x))).max())
        assert np.all(d <= 4 * EPS * np.maximum(1.0, np.abs(x))), (name, d.max())
    print("%s: nlp2op -> guess -> starting point on the same mesh: worst |error| %.3e, relative to max(1, |x|) %.3e" % (name, worst_abs, worst_rel))


# ---- on the device ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case,target", CASE_TARGETS)
def test_against_the_one_instance_path(built, case, target):
    src, to, xs = _pair(case, target)
    ref = _reference(case, target)
    got, flags = src.carry_solution_batch(to, xs)
    assert got.shape == ref.shape == (len(xs), to.n)
    assert not flags.any() and np.isfinite(got).all()
    cols, scal, par = _columns(to)
    assert np.array_equal(got[:, scal], ref[:, scal])                       # t0, tf, static parameters: to the bit
    worst = 0.0
    for b in range(len(xs)):
        for c in cols:
            scale = max(1.0, np.abs(ref[b, c]).max())
            d = np.abs(got[b, c] - ref[b, c]).max()
            worst = max(worst, d / scale)
            assert d <= 1e-12 * scale, (case, target, b, c, d, scale)
    print("%s -> %s: worst |carried - one-instance path| / max(1, max|column|) = %.3e (bound 1e-12)" % (case, target, worst))
    assert np.array_equal(got[:, par], xs[:, _columns(src)[2]])             # the parameters are the source's
    assert par.size == (4 if case == "oscillator" else 0)
    if target == "same":                                                    # the spline returns its own knots
        for b in range(len(xs)):
            for c in cols:
                assert np.abs(got[b, c] - xs[b, c]).max() <= 1e-12 * max(1.0, np.abs(xs[b, c]).max()), (case, b, c)
    src.close()
    to.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case,target", [("quadrotor", "refined"), ("quadrotor", "coarse"), ("launch", "ragged"),
                                         ("oscillator", "one_by_two"), ("hypersensitive", "one_by_five")])
def test_every_layout_and_both_forms_give_the_same_bits(built, case, target):
    import torch
    src, to, xs = _pair(case, target)
    B = len(xs)
    base, flags0 = src.carry_solution_batch(to, xs)
    s = torch.cuda.Stream()
    d_x = torch.from_numpy(np.array(xs)).cuda()
    d_out = torch.empty((B, to.n), dtype=torch.float64, device="cuda")
    d_flag = torch.empty(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for tile in TILES:
        src.set_option("carry_tile", tile)
        assert src.get_option("carry_tile") == tile
        got, flags = src.carry_solution_batch(to, xs)
        assert np.array_equal(got, base) and np.array_equal(flags, flags0), tile
        for _ in range(2):                                   # outputs pre-filled with NaN, twice
            d_out.fill_(float("nan"))
            d_flag.fill_(7)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                src.carry_solution_batch_dev(to, d_x, d_out, d_flag, stream=s.cuda_stream)
            s.synchronize()
            assert np.array_equal(d_out.cpu().numpy(), base) and np.array_equal(d_flag.cpu().numpy(), flags0), tile
        d_out.fill_(float("nan"))
        torch.cuda.synchronize()
        src.carry_solution_batch_dev(to, d_x, d_out, None, stream=s.cuda_stream)        # without the verdicts
        s.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), base)
    src.close()
    to.close()


@pytest.mark.gpu
def test_captured_graph_replayed_on_new_x(built):
    import torch
    src, to, xs = _pair("quadrotor", "refined")
    B = len(xs)
    s = torch.cuda.Stream()
    d_x = torch.from_numpy(np.array(xs)).cuda()
    d_out = torch.empty((B, to.n), dtype=torch.float64, device="cuda")
    d_flag = torch.empty(B, dtype=torch.int32, device="cuda")
    prev = torch.cuda.current_device()
    src.carry_solution_batch_dev(to, d_x, d_out, d_flag, stream=s.cuda_stream)      # the first call on the pair: the plan goes up
    s.synchronize()
    assert torch.cuda.current_device() == prev
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        src.carry_solution_batch_dev(to, d_x, d_out, d_flag, stream=s.cuda_stream)
    makers, _ = _source("quadrotor")
    xs2 = _iterates([m() for m in makers], 500)
    assert not np.array_equal(xs2, xs)
    d_x.copy_(torch.from_numpy(xs2).cuda())
    d_out.fill_(float("nan"))
    d_flag.fill_(7)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    want, flags = src.carry_solution_batch(to, xs2)
    assert np.array_equal(d_out.cpu().numpy(), want) and np.array_equal(d_flag.cpu().numpy(), flags)
    del g
    src.close()
    to.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case,target", [("quadrotor", "refined"), ("launch", "ragged"), ("oscillator", "one_by_two")])
def test_a_batch_equals_its_instances_carried_alone(built, case, target):
    src, to, xs = _pair(case, target)
    base, _ = src.carry_solution_batch(to, xs)
    makers, _ = _source(case)
    tprobs = _target_probs(case, target)
    for b in range(len(xs)):
        a, t = NLPEngine(makers[b](), device=0), NLPEngine(tprobs[b], device=0)
        alone, flag = a.carry_solution_batch(t, xs[b])
        assert np.array_equal(alone[0], base[b]) and flag[0] == 0, (case, b)
        a.close()
        t.close()
    # to == from is legal: the same mesh
    again, _ = src.carry_solution_batch(src, xs)
    same_to = _batched([m() for m in makers])
    other, _ = src.carry_solution_batch(same_to, xs)
    assert np.array_equal(again, other)
    src.close()
    to.close()
    same_to.close()


@pytest.mark.gpu
def test_sweep_group_equals_one_engine(built):
    makers, xs = _source("quadrotor")
    B = 7
    probs, tprobs = [m() for m in makers[:B]], _target_probs("quadrotor", "refined")[:B]
    src, to = _batched(probs), _batched(tprobs)
    want, flags = src.carry_solution_batch(to, xs[:B])
    g_from, g_to = SweepGroup(probs[0], [0, 0, 0], B), SweepGroup(tprobs[0], [0, 0, 0], B)
    assert g_from.shares() == g_to.shares() == [(0, 2), (2, 2), (4, 3)]
    got, gflags = g_from.carry_solution(g_to, xs[:B])
    assert np.array_equal(got, want) and np.array_equal(gflags, flags)
    # and the 7 are the first 7 of the 37
    full_src, full_to, _ = _pair("quadrotor", "refined")
    assert np.array_equal(full_src.carry_solution_batch(full_to, xs)[0][:B], want)
    two = SweepGroup(tprobs[0], [0, 0], B)
    with pytest.raises(RpmError) as ei:
        g_from.carry_solution(two, xs[:B])
    assert ei.value.code == 1 and "different shares" in str(ei.value)
    for o in (g_from, g_to, two, src, to, full_src, full_to):
        o.close()


@pytest.mark.gpu
def test_a_nan_instance_and_a_zero_length_horizon_are_flagged_and_disturb_nobody(built):
    src, to, xs = _pair("quadrotor", "refined")
    B = len(xs)
    clean, flags = src.carry_solution_batch(to, xs)
    assert not flags.any()
    bad = np.array(xs)
    bad[17, 5] = np.nan                          # a state value of instance 17
    t0 = _columns(src)[1][0]
    bad[3, t0 + 1] = bad[3, t0]                  # tf == t0 in instance 3: its knots are 0 / 0
    bad[30, t0 + 1] = np.inf
    got, flags = src.carry_solution_batch(to, bad)
    want = np.zeros(B, dtype=np.int32)
    want[[3, 17, 30]] = 1
    assert np.array_equal(flags, want)
    others = want == 0
    assert np.array_equal(got[others], clean[others])
    for b in (3, 17, 30):
        assert not np.isfinite(got[b]).all()
    assert np.isnan(got[17]).any()
    src.close()
    to.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [0, 8])
def test_columns_split_over_workgroups_change_no_bit(built, tile):
    src, to, xs = _pair("quadrotor", "refined")
    src.set_option("carry_tile", tile)
    base, flags0 = src.carry_solution_batch(to, xs)
    assert src.get_option("carry_groups") == 1
    tb = tile if tile else 2
    seen = set()
    for cols_per_group in (8, 5, 1):
        src.set_option("carry_lds_bytes", 8 * 25 * (1 + 2 * tb + 2 * tb * cols_per_group))
        groups = src.get_option("carry_groups")
        assert groups == -(-16 // cols_per_group) and groups >= 2
        seen.add(groups)
        got, flags = src.carry_solution_batch(to, xs)
        assert np.array_equal(got, base) and np.array_equal(flags, flags0), (tile, cols_per_group)
    assert seen == {2, 4, 16}
    src.close()
    to.close()
