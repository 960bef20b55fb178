"""Solution extraction for a whole sweep (rpm_nlp2op_batch_layout, rpm_nlp2op_batch*, rpm_sweep_nlp2op).

The reference is the one-instance route that exists without the batched call: one one-instance NLPEngine per instance, built
from that instance's own problem so that it has its own constants, and nlp2op_control(phase, x=x_b, lam=lam_b) for every phase.
That route runs entirely on the device (rpm_post_spline_kernel + rpm_post_kernel + rpm_post_cost_kernel) and the batched kernels
repeat it operation by operation, so every comparison here is np.array_equal on every field, the two scalars included; there is
no tolerance anywhere in this file.  Inputs are seeded iterates, a different seed per instance, and multipliers drawn from
RandomState(seed).uniform(-1, 1, m): nothing depends on a solve converging.

The zero-length horizon is tested on the parameter oscillator, not on the quadrotor: tf == t0 makes a block non-finite only
through a field that divides by tf - t0, and that is the path multipliers (2 (1 / w) lambda / (tf - t0)); the quadrotor has
none (nc = 0), so all of its fields stay finite for tf == t0 and it has nothing to flag."""
import ctypes as C

import numpy as np
import pytest

from _hessian_cases import launch_with
from lpopc_amd import problems
from lpopc_amd.engine import ABI_SYMBOLS, EXTRACT_FIELDS, NLPEngine, RpmError, lib
from lpopc_amd.group import SweepGroup

NEW_SYMBOLS = ["rpm_nlp2op_batch_layout", "rpm_nlp2op_batch_dev", "rpm_nlp2op_batch", "rpm_sweep_nlp2op"]
TILES = (0, 1, 2, 4, 8)
LAUNCH_NODES = ([5, 2], [8, 7], [4, 5, 3], [6, 7, 6])     # 7, 15, 12 and 19 nodes; last intervals 2 and 7 (and 3, 6) nodes wide


# ---- problems, meshes, inputs -----------------------------------------------------------------------------------
def _ragged_oscillator():
    """The two-phase parameter oscillator (nq = 2, nc = 1) on test_sweep_carry.py's ragged meshes: 3 to 19 nodes per interval."""
    p = problems.param_oscillator()
    for i, (mesh, nodes) in enumerate([([-1, -0.7, 0.2, 1], [4, 19, 3]), ([-1, 0.1, 1], [17, 5])]):
        ph = p.GetPhase(i)
        ph.meshpoints = [float(v) for v in mesh]
        ph.nodesperinterval = [int(v) for v in nodes]
    return p


def _ragged_launch():
    return launch_with(LAUNCH_NODES)


def _quadrotor_prefs(B):
    rng = np.random.RandomState(11)
    return [tuple(rng.uniform(-1.5, 1.5, size=3)) for _ in range(B)]


def _makers(name):
    """-> list of B callables, each building instance b's problem"""
    if name == "quadrotor":
        return [lambda p=p: problems.quadrotor(4, 6, pref=p) for p in _quadrotor_prefs(37)]
    if name == "launch":
        return [_ragged_launch] * 5
    if name == "oscillator":
        return [_ragged_oscillator] * 9
    if name == "two_point":                                    # one interval of 2 nodes: the two-point spline, nu = 1, nc = 0
        return [lambda: problems.hypersensitive([-1.0, 1.0], [2])] * 3
    assert name == "wrap"                                      # N = 260 > 256: the partial sums of lagrange_cost wrap
    return [lambda: problems.hypersensitive([float(v) for v in np.linspace(-1.0, 1.0, 14)], [20] * 13)] * 2


CASES = ["two_point", "oscillator", "launch", "quadrotor", "wrap"]


def _batched(probs, device=0):
    eng = NLPEngine(probs[0], n_instances=len(probs), device=device)
    for b in range(1, len(probs)):
        c = probs[b].GetOpimalProblemFuns().consts
        if len(c):
            eng.set_instance_constants(b, c)
    return eng


def _inputs(probs, seed0=100):
    one = NLPEngine(probs[0])
    xl, xu, _, _ = one.get_bounds_info()
    x0 = one.get_starting_point()
    m = one.m
    one.close()
    xs = np.stack([problems.seeded_iterate(x0, xl, xu, seed0 + b) for b in range(len(probs))])
    lams = np.stack([np.random.RandomState(7000 + seed0 + b).uniform(-1, 1, m) for b in range(len(probs))])
    return xs, lams


_SRC, _REF = {}, {}


def _source(case):
    """-> (makers, xs, lams): built once per case and never changed"""
    if case not in _SRC:
        makers = _makers(case)
        xs, lams = _inputs([m() for m in makers])
        xs.setflags(write=False)
        lams.setflags(write=False)
        _SRC[case] = (makers, xs, lams)
    return _SRC[case]


def _one_instance_route(makers, xs, lams):
    """The parent commit's route, instance by instance -> per phase a dict of stacked fields"""
    per = []
    for b, make in enumerate(makers):
        one = NLPEngine(make(), device=0)
        per.append([one.nlp2op_control(p, x=xs[b], lam=lams[b]) for p in range(one.n_phases)])
        one.close()
    return [{k: np.stack([np.asarray(per[b][p][k]) for b in range(len(makers))]) for k in EXTRACT_FIELDS} for p in range(len(per[0]))]


def _reference(case):
    """Computed once per case, shared by the tests that need it and left unchanged."""
    if case not in _REF:
        ref = _one_instance_route(*_source(case))
        for d in ref:
            for a in d.values():
                a.setflags(write=False)
        _REF[case] = ref
    return _REF[case]


def _same(got, want, where=""):
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w) == set(EXTRACT_FIELDS)
        for k in EXTRACT_FIELDS:
            assert g[k].shape == w[k].shape, (where, p, k, g[k].shape, w[k].shape)
            assert np.array_equal(g[k], w[k], equal_nan=True), (where, p, k, np.argwhere(g[k] != w[k])[:4])


def _flat(eng, phases):
    """per-phase dicts -> B x EB in the library's layout (what the _dev form writes)"""
    offs, EB = eng.nlp2op_batch_layout()
    B = phases[0]["time"].shape[0]
    out = np.zeros((B, EB))
    for p, d in enumerate(phases):
        for f, k in enumerate(EXTRACT_FIELDS):
            a = d[k].reshape(B, -1)
            out[:, offs[p, f]:offs[p, f] + a.shape[1]] = a
    return out


def _expected_layout(eng):
    """The formula of include/rpm_hip.h from the phase shapes: per phase time M, state M nx, control M nu, costate M nx,
    pathmult M nc, hamiltonian M, mayer_cost 1, lagrange_cost 1, the phases one after the other."""
    offs, off = [], 0
    for p in range(eng.n_phases):
        d = eng._desc.phases[p]
        M = eng.phase_tables(p)["points"].size + 1
        row = []
        for length in (M, M * d.nx, M * d.nu, M * d.nx, M * d.nc, M, 1, 1):
            row.append(off)
            off += length
        offs.append(row)
    return np.array(offs, dtype=np.int64), off


# ---- without a device -------------------------------------------------------------------------------------------
def test_symbols_exist_and_are_listed(built):
    L = lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in ABI_SYMBOLS, s


@pytest.mark.parametrize("make,B", [(_ragged_launch, 5), (_ragged_oscillator, 9), (lambda: problems.quadrotor(4, 6), 37)])
def test_layout_is_the_documented_formula(built, make, B):
    eng = NLPEngine(make(), n_instances=B)
    offs, EB = eng.nlp2op_batch_layout()
    want, want_EB = _expected_layout(eng)
    assert np.array_equal(offs, want) and EB == want_EB
    # phases of different node counts, so the offsets are not a multiple of one phase's length
    if eng.n_phases > 1:
        assert len({eng.phase_tables(p)["points"].size for p in range(eng.n_phases)}) == eng.n_phases
    # either output may be NULL; a phase out of range is refused
    L, eb = lib(), C.c_longlong()
    assert L.rpm_nlp2op_batch_layout(eng._h, 0, None, C.byref(eb)) == 0 and eb.value == EB
    assert L.rpm_nlp2op_batch_layout(eng._h, eng.n_phases - 1, (C.c_longlong * 8)(), None) == 0
    for bad in (-1, eng.n_phases):
        assert L.rpm_nlp2op_batch_layout(eng._h, bad, None, C.byref(eb)) == 1 and "out of range" in eng.last_error()
    assert L.rpm_nlp2op_batch_layout(None, 0, None, C.byref(eb)) == 1
    eng.close()


def test_argument_errors_are_decided_on_the_host(built):
    L = lib()
    dp = C.POINTER(C.c_double)
    quad = NLPEngine(problems.quadrotor(3, 5), n_instances=4)
    _, EB = quad.nlp2op_batch_layout()
    x, lam, out = np.zeros(4 * quad.n), np.zeros(4 * quad.m), np.zeros(4 * EB)
    px, pl, po = (a.ctypes.data_as(dp) for a in (x, lam, out))

    def refused(fn, code, text, eng=quad):
        with pytest.raises(RpmError) as ei:
            fn()
        assert ei.value.code == code and text in str(ei.value), str(ei.value)
        assert text in eng.last_error()

    assert L.rpm_nlp2op_batch(quad._h, None, pl, po, None) == 1 and "x is NULL" in quad.last_error()
    assert L.rpm_nlp2op_batch(quad._h, px, None, po, None) == 1 and "lambda is NULL" in quad.last_error()
    assert L.rpm_nlp2op_batch(quad._h, px, pl, None, None) == 1 and "out is NULL" in quad.last_error()
    v8 = C.c_void_p(8)
    assert L.rpm_nlp2op_batch_dev(quad._h, None, v8, v8, None, None) == 1 and "d_x is NULL" in quad.last_error()
    assert L.rpm_nlp2op_batch_dev(quad._h, v8, None, v8, None, None) == 1 and "d_lambda is NULL" in quad.last_error()
    assert L.rpm_nlp2op_batch_dev(quad._h, v8, v8, None, None, None) == 1 and "d_out is NULL" in quad.last_error()
    assert L.rpm_nlp2op_batch(None, px, pl, po, None) == 1
    assert L.rpm_sweep_nlp2op(None, px, pl, po, None) == 1
    with pytest.raises(RpmError) as ei:                        # the wrapper's own size checks
        quad.nlp2op_batch(x, lam[:-1])
    assert ei.value.code == 1 and "lambda has" in str(ei.value)
    with pytest.raises(RpmError):
        quad.nlp2op_batch(x[:-1], lam)
    # interval sharding, both forms
    sh = NLPEngine(problems.launch(8, 8), shard_mode=1, shard_rank=1, shard_world=2)
    refused(lambda: sh.nlp2op_batch(np.zeros(sh.n), np.zeros(sh.m)), 2, "interval sharding", sh)
    assert L.rpm_nlp2op_batch_dev(sh._h, v8, v8, v8, None, None) == 2 and "interval sharding" in sh.last_error()
    # a column that cannot fit one workgroup's LDS (the budget is an option for exactly this and the column split)
    assert quad.get_option("extract_groups") == 0
    quad.set_option("extract_tile", 1)
    quad.set_option("extract_lds_bytes", 8 * (3 * 15 + 1) - 8)      # N = 15: points, weights and one column of 15, one end value
    assert quad.get_option("extract_groups") == -1
    refused(lambda: quad.nlp2op_batch(x, lam), 2, "a column of 15 nodes does not fit one workgroup's LDS")
    assert L.rpm_nlp2op_batch_dev(quad._h, v8, v8, v8, None, None) == 2
    quad.set_option("extract_lds_bytes", 8 * (3 * 15 + 1))           # exactly one column of one instance
    assert quad.get_option("extract_groups") == 4
    quad.set_option("extract_lds_bytes", 0)
    assert quad.get_option("extract_lds_bytes") == 0
    for bad in (3, 16, -1):
        with pytest.raises(RpmError):
            quad.set_option("extract_tile", bad)
    with pytest.raises(RpmError):
        quad.set_option("extract_lds_bytes", -8)
    # the one-instance call keeps its refusal for a batched engine
    with pytest.raises(RpmError) as ei:
        quad.nlp2op_control(0, x=x, lam=lam)
    assert ei.value.code == 2 and "one instance per engine" in str(ei.value)
    quad.close()
    sh.close()


def test_no_gpu_means_loud_failure_not_fallback(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    a = NLPEngine(problems.quadrotor(3, 5), n_instances=2)
    with pytest.raises(RpmError) as ei:
        a.nlp2op_batch(np.zeros(2 * a.n), np.zeros(2 * a.m))
    assert ei.value.code == 3 and "no CPU fallback" in str(ei.value)
    a.close()


def test_the_planner_halves_the_tile_then_deals_the_columns(built):
    """Host only.  Quadrotor 4 x 6: N = 24, rows 25 doubles apart, 4 spline columns.  Next to the partial sums a fused workgroup
    of TB instances stages TB Lagrangian rows, points, weights, 4 TB columns and 4 TB end values: 25 (5 TB + 2) + 4 TB doubles;
    a workgroup of the spline launch with c columns 25 (2 + c TB) + c TB."""
    eng = NLPEngine(problems.quadrotor(4, 6), n_instances=37)
    fused = lambda tb: 25 * (5 * tb + 2) + 4 * tb             # noqa: E731
    split = lambda tb, c: 25 * (2 + c * tb) + c * tb          # noqa: E731
    for tile, doubles, groups in ((2, fused(2), 0), (2, fused(2) - 1, 0),      # 2 do not fit: 1 instance, still one launch
                                  (8, fused(1), 0), (2, fused(1) - 1, 2),      # dealt: 2 columns of 2 instances per workgroup
                                  (2, split(2, 2), 2), (2, split(2, 2) - 1, 4), (2, split(2, 1), 4),
                                  (2, split(2, 1) - 1, 4),                     # 1 instance, 1 column
                                  (8, fused(1) - 1, 4),                        # 8 do not fit: 4 instances, 1 column
                                  (1, split(1, 1), 4), (1, split(1, 1) - 1, -1)):
        eng.set_option("extract_tile", tile)
        eng.set_option("extract_lds_bytes", 8 * doubles)
        assert eng.get_option("extract_groups") == groups, (tile, doubles)
    eng.close()


# ---- on the device ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_against_the_one_instance_route(built, case):
    makers, xs, lams = _source(case)
    ref = _reference(case)
    eng = _batched([m() for m in makers])
    got, flags = eng.nlp2op_batch(xs, lams)
    _same(got, ref, case)
    assert not flags.any() and all(np.isfinite(a).all() for d in got for a in d.values())
    assert len(got) == {"launch": 4, "oscillator": 2}.get(case, 1)
    if case == "oscillator":        # the path multipliers of phase 2 come from the unshifted index, not from the phase's own rows
        N1, N2, lam, d = eng.phase_tables(0)["points"].size, eng.phase_tables(1)["points"].size, lams[0], eng._desc.phases[0]
        t0 = d.nx * (N1 + 1) + d.nu * N1 + 2 + d.nq + d.nx * (N2 + 1) + d.nu * N2        # phase 2's t0 in x
        w, tspan = eng.phase_tables(1)["weights"], xs[0, t0 + 1] - xs[0, t0]
        assert np.array_equal(got[1]["pathmult"][0, :N2], 2 * ((1 / w) * lam[2 * N2:3 * N2]) / tspan)
        assert eng._desc.phases[0].nc == 1 and eng.phase_tables(0)["points"].size != N2
    if case == "wrap":
        assert eng.phase_tables(0)["points"].size == 260
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["oscillator", "launch", "quadrotor"])
def test_every_tile_and_both_forms_give_the_same_bits(built, case):
    import torch
    makers, xs, lams = _source(case)
    eng = _batched([m() for m in makers])
    B, (_, EB) = len(xs), eng.nlp2op_batch_layout()
    assert eng.get_option("extract_tile") == 0
    base, flags0 = eng.nlp2op_batch(xs, lams)
    flat = _flat(eng, base)
    s = torch.cuda.Stream()
    d_x, d_lam = torch.from_numpy(np.array(xs)).cuda(), torch.from_numpy(np.array(lams)).cuda()
    d_out = torch.empty((B, EB), dtype=torch.float64, device="cuda")
    d_flag = torch.empty(B, dtype=torch.int32, device="cuda")
    prev = torch.cuda.current_device()
    for tile in TILES:
        eng.set_option("extract_tile", tile)
        assert eng.get_option("extract_tile") == tile and eng.get_option("extract_groups") == 0
        got, flags = eng.nlp2op_batch(xs, lams)
        _same(got, base, (case, tile))
        assert np.array_equal(flags, flags0)
        for _ in range(2):                                   # outputs pre-filled with NaN, twice: every double is written
            d_out.fill_(float("nan"))
            d_flag.fill_(7)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                eng.nlp2op_batch_dev(d_x, d_lam, d_out, d_flag, stream=s.cuda_stream)
            s.synchronize()
            assert np.array_equal(d_out.cpu().numpy(), flat) and np.array_equal(d_flag.cpu().numpy(), flags0), tile
        d_out.fill_(float("nan"))
        torch.cuda.synchronize()
        eng.nlp2op_batch_dev(d_x, d_lam, d_out, None, stream=s.cuda_stream)            # without the verdicts
        s.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), flat)
    assert torch.cuda.current_device() == prev
    eng.close()


@pytest.mark.gpu
def test_sweep_group_with_three_shares_equals_one_engine(built):
    L = lib()
    # shared constants, two phases: 9 instances in shares of 3
    makers, xs, lams = _source("oscillator")
    eng = _batched([m() for m in makers])
    want, wflags = eng.nlp2op_batch(xs, lams)
    grp = SweepGroup(makers[0](), [0, 0, 0], len(xs))
    assert grp.shares() == [(0, 3), (3, 3), (6, 3)]
    got, flags = grp.nlp2op(xs, lams)
    _same(got, want, "oscillator shares")
    assert np.array_equal(flags, wflags)
    eng.close()
    grp.close()
    # per-instance constants: the first 7 quadrotor instances in shares of 2, 2 and 3
    makers, xs, lams = _source("quadrotor")
    B = 7
    probs = [m() for m in makers[:B]]
    eng = _batched(probs)
    want, wflags = eng.nlp2op_batch(xs[:B], lams[:B])
    _same(want, [{k: a[:B] for k, a in d.items()} for d in _reference("quadrotor")], "the 7 are the first 7 of the 37")
    grp = SweepGroup(probs[0], [0, 0, 0], B)
    assert grp.shares() == [(0, 2), (2, 2), (4, 3)]
    for r, (first, count) in enumerate(grp.shares()):
        h = L.rpm_sweep_engine(grp._h, r)
        for i in range(count):
            c = np.ascontiguousarray(probs[first + i].GetOpimalProblemFuns().consts, dtype=np.float64)
            assert L.rpm_set_instance_constants(h, i, c.ctypes.data_as(C.POINTER(C.c_double)), c.size) == 0
    got, flags = grp.nlp2op(xs[:B], lams[:B])
    _same(got, want, "quadrotor shares")
    assert np.array_equal(flags, wflags)
    with pytest.raises(RpmError) as ei:
        grp.nlp2op(xs[:B], lams[:B - 1])
    assert ei.value.code == 1
    eng.close()
    grp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["oscillator", "launch", "quadrotor"])
def test_a_batch_equals_its_instances_extracted_as_batches_of_one(built, case):
    makers, xs, lams = _source(case)
    eng = _batched([m() for m in makers])
    base, _ = eng.nlp2op_batch(xs, lams)
    eng.close()
    for b in range(0, len(xs), 4 if case == "quadrotor" else 1):
        one = NLPEngine(makers[b](), device=0)
        alone, flag = one.nlp2op_batch(xs[b], lams[b])
        _same(alone, [{k: a[b:b + 1] for k, a in d.items()} for d in base], (case, b))
        assert flag.shape == (1,) and flag[0] == 0
        one.close()


@pytest.mark.gpu
def test_captured_graph_replayed_on_new_inputs(built):
    import torch
    makers, xs, lams = _source("quadrotor")
    eng = _batched([m() for m in makers])
    B, (_, EB) = len(xs), eng.nlp2op_batch_layout()
    s = torch.cuda.Stream()
    d_x, d_lam = torch.from_numpy(np.array(xs)).cuda(), torch.from_numpy(np.array(lams)).cuda()
    d_out = torch.empty((B, EB), dtype=torch.float64, device="cuda")
    d_flag = torch.empty(B, dtype=torch.int32, device="cuda")
    eng.nlp2op_batch_dev(d_x, d_lam, d_out, d_flag, stream=s.cuda_stream)      # the first call on the engine: the plan is made
    s.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), _flat(eng, _reference("quadrotor")))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):                                        # one stream: a chain, no parallel branches
        eng.nlp2op_batch_dev(d_x, d_lam, d_out, d_flag, stream=s.cuda_stream)
    xs2, lams2 = _inputs([m() for m in makers], 500)
    assert not np.array_equal(xs2, xs) and not np.array_equal(lams2, lams)
    d_x.copy_(torch.from_numpy(xs2).cuda())
    d_lam.copy_(torch.from_numpy(lams2).cuda())
    d_out.fill_(float("nan"))
    d_flag.fill_(7)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    want = _flat(eng, _one_instance_route(makers, xs2, lams2))                 # the new instances' reference
    assert np.array_equal(d_out.cpu().numpy(), want) and not d_flag.cpu().numpy().any()
    del g
    eng.close()


@pytest.mark.gpu
def test_nan_instances_and_a_zero_length_horizon_are_flagged_and_disturb_nobody(built):
    makers, xs, lams = _source("oscillator")
    eng = _batched([m() for m in makers])
    B = len(xs)
    clean, flags = eng.nlp2op_batch(xs, lams)
    assert not flags.any()
    bad_x, bad_lam = np.array(xs), np.array(lams)
    bad_x[2, 5] = np.nan                                     # a state value of instance 2
    bad_lam[5, eng.m // 2] = np.nan                          # a multiplier of instance 5
    N1, d = eng.phase_tables(0)["points"].size, eng._desc.phases[0]
    t0 = d.nx * (N1 + 1) + d.nu * N1                         # phase 1's t0 in x
    assert xs[7, t0 + 1] != xs[7, t0]
    bad_x[7, t0 + 1] = bad_x[7, t0]                          # tf == t0 in instance 7: its path multipliers divide by 0
    got, flags = eng.nlp2op_batch(bad_x, bad_lam)
    want = np.zeros(B, dtype=np.int32)
    want[[2, 5, 7]] = 1
    assert np.array_equal(flags, want)
    others = want == 0
    _same([{k: a[others] for k, a in dd.items()} for dd in got], [{k: a[others] for k, a in dd.items()} for dd in clean], "clean instances")
    for b in (2, 5, 7):
        assert not all(np.isfinite(dd[k][b]).all() for dd in got for k in EXTRACT_FIELDS)
    assert np.isnan(got[0]["state"][2]).any() and not np.isfinite(got[0]["pathmult"][7]).all()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case,tile,doubles,groups", [("quadrotor", 2, 25 * 7 + 4 - 1, 2), ("quadrotor", 8, 25 * 7 + 4 - 1, 4),
                                                      ("quadrotor", 1, 25 * 3 + 1, 4), ("oscillator", 2, 27 * 5 + 2 - 1, 4)])
def test_columns_dealt_over_workgroups_change_no_bit(built, case, tile, doubles, groups):
    """The LDS budget just under what one instance's fused workgroup stages (quadrotor: N = 24, 4 columns; oscillator phase 1:
    N = 26, 2 columns, one of them a path multiplier), so the spline columns get a launch of their own, dealt over `groups`
    workgroups per tile of instances, and the Lagrangian goes through the workspace."""
    makers, xs, lams = _source(case)
    eng = _batched([m() for m in makers])
    eng.set_option("extract_tile", tile)
    base, flags0 = eng.nlp2op_batch(xs, lams)
    assert eng.get_option("extract_groups") == 0
    eng.set_option("extract_lds_bytes", 8 * doubles)
    assert eng.get_option("extract_groups") == groups
    got, flags = eng.nlp2op_batch(xs, lams)
    _same(got, base, (case, tile))
    _same(got, _reference(case), (case, tile, "reference"))
    assert np.array_equal(flags, flags0)
    eng.close()
