"""The mesh-error estimate and the ph refinement decision for a whole sweep (rpm_solution_error_batch*,
rpm_sweep_solution_error): every instance's result is, bit for bit, what the one-instance path computes for it, because
the batched kernels perform the same operations in the same order with contraction off.  Against the CPU oracle the
tolerance is the one the project already uses for this quantity, 1e-12 * max(1, |ref|.max()) (the dynamics call libm on
both sides).  Inputs are seeded iterates, a different seed per instance: nothing depends on a solve converging."""
import ctypes as C
import itertools

import numpy as np
import pytest

from lpopc_amd import problems
from lpopc_amd.engine import ABI_SYMBOLS, NLPEngine, RpmError, lib
from lpopc_amd.group import SweepGroup

TRIPLES = [(1e-6, 4, 16), (1e-3, 3, 8), (1e-9, 2, 5)]      # the (tol, nmin, nmax) of test_solution_error_and_ph_refine


def _ragged_oscillator():
    """The two-phase parameter oscillator (nq > 0) on ragged meshes: unequal widths, 3 to 19 nodes per interval."""
    p = problems.param_oscillator()
    for i, (mesh, nodes) in enumerate([([-1, -0.7, 0.2, 1], [4, 19, 3]), ([-1, 0.1, 1], [17, 5])]):
        ph = p.GetPhase(i)
        ph.GetMeshPoints().clear()
        ph.GetNodesPerInterval().clear()
        problems.set_mesh(ph, mesh, nodes)
    return p


def _quadrotor_prefs(B):
    rng = np.random.RandomState(11)
    return [tuple(rng.uniform(-1.5, 1.5, size=3)) for _ in range(B)]


def _case(name):
    """-> (list of B problems (instance b's own), B)"""
    if name == "quadrotor":
        return [problems.quadrotor(4, 6, pref=p) for p in _quadrotor_prefs(37)]
    if name == "launch":
        return [problems.launch(8, 8) for _ in range(5)]
    return [_ragged_oscillator() for _ in range(9)]


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


def _py_sizes(prob):
    kt = rt = 0
    for i in range(prob.GetPhaseNum()):
        ph = prob.GetPhase(i)
        nodes = list(ph.GetNodesPerInterval())
        nx = ph.get_optimal_info()[0]
        kt += len(nodes)
        rt += (sum(nodes) + len(nodes) + 1) * nx
    return kt, rt


# ---- without a device -------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["rpm_solution_error_batch_sizes", "rpm_solution_error_batch_dev", "rpm_solution_error_batch",
               "rpm_sweep_solution_error"]


@pytest.mark.parametrize("name", ["quadrotor", "launch", "ragged_oscillator"])
def test_symbols_and_sizes(built, name):
    L = lib()          # not a second CDLL of its own: the library shares the HIP runtime torch has mapped (engine.lib)
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
    prob = {"quadrotor": lambda: problems.quadrotor(8, 8), "launch": lambda: problems.launch(8, 8),
            "ragged_oscillator": _ragged_oscillator}[name]()
    eng = NLPEngine(prob, n_instances=3)
    assert eng.solution_error_batch_sizes() == _py_sizes(prob)
    if name == "quadrotor":
        assert eng.solution_error_batch_sizes() == (8, (64 + 8 + 1) * 12)
    eng.close()


def test_argument_errors_are_decided_on_the_host(built):
    prob = problems.quadrotor(3, 5)
    eng = NLPEngine(prob, n_instances=4)
    L = lib()
    KT, RT = eng.solution_error_batch_sizes()
    x, mx = np.zeros(4 * eng.n), np.zeros(RT)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    assert L.rpm_solution_error_batch(eng._h, None, None, None, mx.ctypes.data_as(dp), None, None) == 1
    assert "x is NULL" in eng.last_error()
    assert L.rpm_solution_error_batch_dev(eng._h, None, None, None, None, None, None, None) == 1
    with pytest.raises(RpmError) as ei:                       # every instance masked out and rel_err_max asked for
        eng.solution_error_batch(x, mask=[0, 0, 0, 0])
    assert ei.value.code == 1 and "excludes every instance" in str(ei.value)
    with pytest.raises(RpmError) as ei:
        eng.solution_error_batch(x, mask=[1, 0])              # wrong mask length never reaches the library
    assert ei.value.code == 1
    eng.close()
    sh = NLPEngine(problems.launch(8, 8), shard_mode=1, shard_rank=1, shard_world=2)
    with pytest.raises(RpmError) as ei:
        sh.solution_error_batch(np.zeros(sh.n))
    assert ei.value.code == 2 and "interval sharding" in str(ei.value)
    assert L.rpm_solution_error_batch_dev(sh._h, C.c_void_p(16), None, None, None, None, None, None) == 2
    sh.close()
    # the one-instance entry points keep their refusal
    eng = NLPEngine(prob, n_instances=2)
    rows = C.c_int()
    assert L.rpm_solution_error(eng._h, 0, x.ctypes.data_as(dp), mx.ctypes.data_as(dp), C.byref(rows)) == 2
    assert "one instance per engine" in eng.last_error()
    eng.close()


def test_no_gpu_means_loud_failure_not_fallback(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    eng = NLPEngine(problems.quadrotor(3, 5), n_instances=2)
    with pytest.raises(RpmError) as ei:
        eng.solution_error_batch(np.zeros(2 * eng.n))
    assert ei.value.code == 3 and "no CPU fallback" in str(ei.value)
    assert eng.solution_error_batch_sizes()[0] == 3            # the sizes need no device
    eng.close()


# ---- on the device ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["quadrotor", "launch", "ragged_oscillator"])
def test_bit_identical_to_the_one_instance_path_and_close_to_the_oracle(built, name):
    probs = _case(name)
    B = len(probs)
    xs = _iterates(probs)
    eng = _batched(probs)
    est = eng.solution_error_batch(xs, full=True)
    assert not est["nonfinite"].any()
    peaks = np.zeros(B)
    for b in range(B):
        one = NLPEngine(probs[b], device=0)
        one.finalize_solution(0, xs[b], np.zeros(one.m), 0.0)      # solution_error's row query wants a stored solution
        orc = None
        if name != "ragged_oscillator":       # the oracle's estimate hands the dynamics no parameters: nq = 0 problems only
            from oracle.oracle import Oracle
            orc = Oracle(probs[b])
        for ph in range(eng.n_phases):
            ref = one.solution_error(ph, xs[b])
            got = est["rel_err"][ph][b]
            assert got.shape == ref.shape and np.array_equal(got, ref), (name, b, ph, np.abs(got - ref).max())
            iv = one.ph_refine_mesh(ph, 1e-6, 4, 16, x=xs[b])[3]
            assert np.array_equal(est["interval_error"][ph][b], iv), (name, b, ph)
            peaks[b] = max(peaks[b], got.max())
            if orc is not None:
                o = orc.solution_error(ph, xs[b])
                assert np.isfinite(o).all()
                d = np.abs(got - o).max()
                print("%s instance %d phase %d: |device - oracle| max %.3e, bound %.3e" % (name, b, ph, d, 1e-12 * max(1.0, np.abs(o).max())))
                assert d <= 1e-12 * max(1.0, np.abs(o).max()), (name, b, ph, d)
        one.close()
    assert len(set(peaks)) > 1                # the instances really differ
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["quadrotor", "launch", "ragged_oscillator"])
def test_maximum_over_the_included_instances_and_the_sweeps_next_mesh(built, name):
    probs = _case(name)
    B = len(probs)
    xs = _iterates(probs)
    eng = _batched(probs)
    est = eng.solution_error_batch(xs, full=True)
    worst = int(np.argmax([max(est["rel_err"][ph][b].max() for ph in range(eng.n_phases)) for b in range(B)]))
    mask = np.ones(B, dtype=np.int32)
    mask[worst] = 0
    mask[(worst + 3) % B] = 0
    part = eng.solution_error_batch(xs, mask=mask, full=True)
    for ph in range(eng.n_phases):
        assert np.array_equal(est["rel_err_max"][ph], np.maximum.reduce(est["rel_err"][ph], axis=0))
        keep = np.maximum.reduce(part["rel_err"][ph][mask != 0], axis=0)
        assert np.array_equal(part["rel_err_max"][ph], keep)
        # an excluded instance is still estimated and reported
        assert np.array_equal(part["rel_err"][ph], est["rel_err"][ph])
        assert np.array_equal(part["interval_error"][ph], est["interval_error"][ph])
    top = lambda e: max(m.max() for m in e["rel_err_max"])   # noqa: E731
    assert top(part) < top(est)               # the instance holding the largest error left: the maximum dropped
    for m, label in ((None, est), (mask, part)):
        for tol, nmin, nmax in TRIPLES:
            got = eng.ph_refine_sweep(xs, tol, nmin, nmax, mask=m)
            for ph in range(eng.n_phases):
                d2, m2, n2, e2 = eng.ph_refine_from_error(ph, label["rel_err_max"][ph], tol, nmin, nmax)
                d1, m1, n1, e1 = got[ph]
                assert d1 == d2 and np.array_equal(m1, m2) and np.array_equal(n1, n2) and np.array_equal(e1, e2)
                # the worst instance decides: the sweep's interval errors are the maxima of the instances'
                sel = np.ones(B, dtype=bool) if m is None else m != 0
                assert np.array_equal(e1, label["interval_error"][ph][sel].max(axis=0))
    eng.close()


@pytest.mark.gpu
def test_maximum_of_a_large_sweep_takes_two_passes_and_changes_nothing(built):
    """More than 64 instances: the maximum is formed per chunk of instances first, then over the chunks.  A maximum is
    exact in any order, so the result is still numpy's over the full matrices, also when whole chunks are excluded."""
    B = 203
    prob = problems.quadrotor(3, 5)
    eng = NLPEngine(prob, n_instances=B, device=0)
    xs = _iterates([prob] * B)
    rng = np.random.RandomState(3)
    masks = [None, (rng.uniform(size=B) < 0.5).astype(np.int32), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)]
    masks[2][20:40] = 1                        # chunks of 7 instances: 0, 1 and most others hold no included instance
    masks[3][B - 1] = 1
    for mask in masks:
        est = eng.solution_error_batch(xs, mask=mask, full=True)
        sel = np.ones(B, dtype=bool) if mask is None else mask != 0
        for ph in range(eng.n_phases):
            assert np.array_equal(est["rel_err_max"][ph], np.maximum.reduce(est["rel_err"][ph][sel], axis=0))
    eng.close()


@pytest.mark.gpu
def test_a_nan_instance_is_flagged_and_disturbs_nobody(built):
    probs = _case("quadrotor")
    B = len(probs)
    xs = _iterates(probs)
    eng = _batched(probs)
    clean = eng.solution_error_batch(xs, full=True)
    bad = xs.copy()
    bad[17, 5] = np.nan                        # a state value of instance 17, phase 0
    est = eng.solution_error_batch(bad, full=True)
    flags = np.zeros(B, dtype=np.int32)
    flags[17] = 1
    assert np.array_equal(est["nonfinite"], flags) and not clean["nonfinite"].any()
    others = np.arange(B) != 17
    for ph in range(eng.n_phases):
        assert np.array_equal(est["rel_err"][ph][others], clean["rel_err"][ph][others])
        assert np.array_equal(est["interval_error"][ph][others], clean["interval_error"][ph][others])
        assert np.isnan(est["rel_err"][ph][17]).any()
        assert np.isnan(est["rel_err_max"][ph]).any()          # visible in the maximum, not swallowed
    masked = eng.solution_error_batch(bad, mask=others.astype(np.int32))
    only = eng.solution_error_batch(xs, mask=others.astype(np.int32))
    for ph in range(eng.n_phases):
        assert np.array_equal(masked["rel_err_max"][ph], only["rel_err_max"][ph])
    assert masked["nonfinite"][17] == 1
    eng.close()


@pytest.mark.gpu
def test_device_resident_form_on_a_stream_and_in_a_graph(built):
    import torch
    probs = _case("quadrotor")
    B = len(probs)
    xs = _iterates(probs)
    eng = _batched(probs)
    KT, RT = eng.solution_error_batch_sizes()
    mask = np.ones(B, dtype=np.int32)
    mask[::5] = 0
    host = eng.solution_error_batch(xs, mask=mask, full=True)
    flat = lambda parts, lead: np.concatenate([p.swapaxes(-1, -2).reshape(lead + (-1,)) for p in parts], axis=-1)   # noqa: E731
    h_rel, h_max = flat(host["rel_err"], (B,)), flat(host["rel_err_max"], ())
    h_iv = np.concatenate(host["interval_error"], axis=1)
    s = torch.cuda.Stream()
    f64 = dict(dtype=torch.float64, device="cuda")
    d_x = torch.from_numpy(xs).cuda()
    d_mask = torch.from_numpy(mask).cuda()
    d_iv, d_max, d_rel = torch.empty((B, KT), **f64), torch.empty(RT, **f64), torch.empty((B, RT), **f64)
    d_flag = torch.empty(B, dtype=torch.int32, device="cuda")

    def check():
        assert np.array_equal(d_iv.cpu().numpy(), h_iv) and np.array_equal(d_max.cpu().numpy(), h_max)
        assert np.array_equal(d_rel.cpu().numpy(), h_rel) and np.array_equal(d_flag.cpu().numpy(), host["nonfinite"])

    torch.cuda.synchronize()
    for _ in range(2):
        for t in (d_iv, d_max, d_rel):
            t.fill_(float("nan"))
        d_flag.fill_(7)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            eng.solution_error_batch_dev(d_x, d_mask, d_iv, d_max, d_rel, d_flag, stream=s.cuda_stream)
        s.synchronize()
        check()
    # every combination of absent outputs, with and without a mask
    for want in itertools.product([0, 1], repeat=5):
        for t in (d_iv, d_max, d_rel):
            t.fill_(float("nan"))
        d_flag.fill_(7)
        torch.cuda.synchronize()
        eng.solution_error_batch_dev(d_x, d_mask if want[0] else None, d_iv if want[1] else None, d_max if want[2] else None,
                                     d_rel if want[3] else None, d_flag if want[4] else None, stream=s.cuda_stream)
        s.synchronize()
        if want[1]:
            assert np.array_equal(d_iv.cpu().numpy(), h_iv)
        if want[2]:
            ref = h_max if want[0] else np.maximum.reduce(h_rel, axis=0)
            assert np.array_equal(d_max.cpu().numpy(), ref)
        if want[3]:
            assert np.array_equal(d_rel.cpu().numpy(), h_rel)
        if want[4]:
            assert np.array_equal(d_flag.cpu().numpy(), host["nonfinite"])
    # every instance excluded: the device form cannot know, its maximum is all zeros
    eng.solution_error_batch_dev(d_x, torch.zeros(B, dtype=torch.int32, device="cuda"), None, d_max, None, None, stream=s.cuda_stream)
    s.synchronize()
    assert not d_max.cpu().numpy().any()
    # captured once, replayed on other x values written into the same tensor
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        eng.solution_error_batch_dev(d_x, d_mask, d_iv, d_max, d_rel, d_flag, stream=s.cuda_stream)
    xs2 = _iterates(probs, 500)
    assert not np.array_equal(xs2, xs)
    d_x.copy_(torch.from_numpy(xs2).cuda())
    for t in (d_iv, d_max, d_rel):
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    host = eng.solution_error_batch(xs2, mask=mask, full=True)
    h_rel, h_max = flat(host["rel_err"], (B,)), flat(host["rel_err_max"], ())
    h_iv = np.concatenate(host["interval_error"], axis=1)
    check()
    del g
    eng.close()


@pytest.mark.gpu
def test_sweep_group_equals_one_engine(built):
    prefs = _quadrotor_prefs(7)
    probs = [problems.quadrotor(4, 6, pref=p) for p in prefs]
    xs = _iterates(probs)
    eng = _batched(probs)
    grp = SweepGroup(probs[0], [0, 0, 0], 7)
    L = lib()
    for r, (first, count) in enumerate(grp.shares()):
        for b in range(count):
            c = np.ascontiguousarray(probs[first + b].GetOpimalProblemFuns().consts, dtype=np.float64)
            assert L.rpm_set_instance_constants(L.rpm_sweep_engine(grp._h, r), b, c.ctypes.data_as(C.POINTER(C.c_double)), c.size) == 0
    assert grp.shares() == [(0, 2), (2, 2), (4, 3)]
    for mask in (None, np.array([1, 1, 0, 0, 1, 0, 1], dtype=np.int32)):     # the second empties the middle share
        a, b = eng.solution_error_batch(xs, mask=mask, full=True), grp.solution_error(xs, mask=mask, full=True)
        assert np.array_equal(a["nonfinite"], b["nonfinite"])
        for ph in range(eng.n_phases):
            for k in ("interval_error", "rel_err_max", "rel_err"):
                assert np.array_equal(a[k][ph], b[k][ph]), (k, ph)
        for tol, nmin, nmax in TRIPLES:
            for (d1, m1, n1, e1), (d2, m2, n2, e2) in zip(eng.ph_refine_sweep(xs, tol, nmin, nmax, mask=mask),
                                                           grp.ph_refine(xs, tol, nmin, nmax, mask=mask)):
                assert d1 == d2 and np.array_equal(m1, m2) and np.array_equal(n1, n2) and np.array_equal(e1, e2)
    with pytest.raises(RpmError) as ei:
        grp.solution_error(xs, mask=np.zeros(7, dtype=np.int32))
    assert ei.value.code == 1
    grp.close()
    eng.close()
