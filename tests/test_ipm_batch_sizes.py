"""The batched interior-point solver at sweep batch sizes: an instance's result must not depend on how many other instances share
the batch, where in the batch it sits, or what the others do ("An instance of a batch, as if alone").

Every kernel of the solve loop is launched for every instance in every round and decides inside, from the instance record, whether
the instance takes part; launch geometry and kernel choice change with the batch size B (the table in DESIGN.md).  The tests here
run the production entry points and the two factor-and-solve hooks at B = 33 ... 260 in batches whose instances are in different
states in the same round (finished, stopped with NaN, backtracking, restoration phase), and compare — bit for bit unless a case
says otherwise — with the solver's own one-instance solve ("solo", set up to run the batch's kernels), with the same batch in
another order, and with the same batch after one instance's start moved by one bit.  Solo is pinned to the numpy restatement by
the other test_ipm*.py files; four instances of the large batches are compared with the restatement here as well.

"Result": x, lambda, obj, status, iterations, kkt_error, bound multipliers, the trace and the restoration count.
"""
import numpy as np
import pytest

import _ipm_batch_cases as bc
from lpopc_amd import problems
from lpopc_amd.problem import Options
from oracle import ipm_oracle
from oracle import oracle as orc

SWEEP_OPTS = dict(max_iter=200, trace=200)


# ------------------------------------------------------------------------------------------- CPU: the seeds of the sweep
@pytest.mark.parametrize("B", [33, 260])
def test_restatement_finds_the_quadrotor_sweep_mixed(B):
    """The restatement on the finite picks of the heterogeneous sweep: they all converge, in at least three different iteration
    counts, and the instance that starts at its own solution is done at least 5 iterations before the slowest.  (The device
    tests assert the same of the device's own counts.)"""
    s = bc.quadrotor_sweep(B)
    its = {}
    for bi in bc.picks(B, bc.SPECIAL):
        if bi in (bc.NAN_X0, bc.NAN_BOUND):
            continue
        r = bc.restatement(s, bi, max_iter=200)
        assert r["status"] == 0, bi
        its[bi] = r["iterations"]
    print("restatement iterations:", its)
    assert len(set(its.values())) >= 3
    assert its[bc.EARLY] <= max(its.values()) - 5
    # the same instance whatever the batch size
    small = bc.quadrotor_sweep(40)
    for k in ("XL", "XU", "X0"):
        assert bc.same_bits(small[k][:33], s[k][:33])
    assert bc.picks(260, bc.SPECIAL) == [0, 1, 5, 17, 31, 32, 63, 64, 255, 256, 258, 259]


# ------------------------------------------------------------------------------------------- 1. evaluations
@pytest.mark.gpu
@pytest.mark.parametrize("layout,B", [("default", 260), ("role_looped", 260), ("automatic", 4096)], ids=["default_260", "role_looped_260", "automatic_4096"])
def test_evaluations_at_sweep_sizes(built, layout, B):
    """f, grad f, (g, Jacobian) and the Hessian (sigma = 1) of B quadrotor(2, 4) instances with their own constants, on the
    device-pointer entry points the solver consumes, against one-instance engines built from each pick's problem: bit for bit.
    Layout options are untouched on both sides of "default" and "automatic".  At this mesh (8 nodes) the automatic switch to the
    role-looped tile layout (nodes * B / 64 >= 512) needs B >= 4096: 260 instances run the one-role layout, as one instance does;
    4096 run the role-looped one (asserted), against one-instance engines on the one-role layout.  "role_looped": 260 instances
    given the layout a large sweep gets (role_loop = 1, 64-node tiles).  No difference in summation order between the layouts
    shows, so the later tests leave role_loop and tile_nodes alone."""
    import torch
    from lpopc_amd.engine import NLPEngine
    s = bc.quadrotor_sweep(B, special=False)
    eng = bc.engine_with_constants(bc.quadrotor_problem(), bc.exact(), B, s["consts"], role_loop=1 if layout == "role_looped" else None)
    assert eng.get_option("tile_nodes") == (16 if layout == "default" else 64)
    xl, xu, _, _ = eng.get_bounds_info()
    guess = eng.get_starting_point()[:eng.n]
    xs = np.stack([problems.seeded_iterate(guess, xl, xu, 40 + bi) for bi in range(B)])
    lam = np.random.RandomState(6).uniform(-1, 1, (B, eng.m))
    sg, sv = eng.get_option("stride_g"), eng.get_option("stride_values")
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    d_x, d_lam = torch.from_numpy(xs).cuda(), torch.from_numpy(lam).cuda()
    d_f, d_grad, d_g, d_v, d_h = nan(B), nan(B, eng.n), nan(B, sg), nan(B, sv), nan(B, eng.nnz_h)
    eng.eval_f_dev(d_x, d_f)
    eng.eval_grad_f_dev(d_x, d_grad)
    eng.eval_pair_dev(d_x, d_g, d_v)
    eng.eval_h_dev(d_x, 1.0, d_lam, d_h)
    torch.cuda.synchronize()
    f, grad, g, v, h = (t.cpu().numpy() for t in (d_f, d_grad, d_g, d_v, d_h))
    assert np.isfinite(f).all() and np.isfinite(grad).all() and np.isfinite(h).all()
    assert np.isfinite(g[:, :eng.m]).all() and np.isfinite(v[:, :eng.nnz_jac]).all()
    assert len(set(np.round(f, 9))) == B
    for bi in bc.picks(B):
        one = NLPEngine(bc.quadrotor_problem(s["prefs"][bi]), bc.exact(), device=0)
        o_x, o_lam = torch.from_numpy(xs[bi].copy()).cuda(), torch.from_numpy(lam[bi].copy()).cuda()
        o_f, o_grad, o_g, o_v, o_h = nan(1), nan(one.n), nan(one.m), nan(one.nnz_jac), nan(one.nnz_h)
        one.eval_f_dev(o_x, o_f)
        one.eval_grad_f_dev(o_x, o_grad)
        one.eval_pair_dev(o_x, o_g, o_v)
        one.eval_h_dev(o_x, 1.0, o_lam, o_h)
        torch.cuda.synchronize()
        assert bc.same_bits(f[bi:bi + 1], o_f.cpu().numpy()), ("f", bi)
        assert bc.same_bits(grad[bi], o_grad.cpu().numpy()), ("grad f", bi)
        assert bc.same_bits(g[bi, :eng.m], o_g.cpu().numpy()), ("g", bi)
        assert bc.same_bits(v[bi, :eng.nnz_jac], o_v.cpu().numpy()), ("jacobian", bi)
        assert bc.same_bits(h[bi], o_h.cpu().numpy()), ("hessian", bi, np.abs(h[bi] - o_h.cpu().numpy()).max())
        one.close()
    eng.close()


# ------------------------------------------------------------------------------------------- 2. factor and substitute
@pytest.mark.gpu
@pytest.mark.parametrize("nested", [0, 1], ids=["band", "nested"])
@pytest.mark.parametrize("B", [33, 257, 260])
def test_factor_and_substitute_on_given_matrices(built, B, nested):
    """rpm_ipm_debug_solve_dense on test_ipm.py's random quasi-definite matrices in bryson_denham(2, 4)'s envelope.
    Every instance: within 1e-11 max|ref| of numpy.linalg.solve (the bound test_ipm.py and DESIGN.md use for this kernel on these
    matrices), inertia = the sign counts; 33 and 257 are no multiples of the inertia kernel's 4 instances per workgroup, 257 and 260
    lie past 256.
    The picks, three at a time through a B = 3 solver: bit for bit — with the nested layout past 256 instances the last level
    leaves kkt_factor_dense_kernel for kkt_factor_kernel (choose_kernels), so there the small solver runs with upper_dense 0
    (test_register_resident_upper_levels: 0 is kkt_factor_kernel alone), and left at its defaults it agrees to the same 1e-11."""
    from lpopc_amd.engine import BatchedIPM, NLPEngine
    from test_ipm import _random_kkt_dense
    prob = problems.bryson_denham(2, 4)
    eng = NLPEngine(prob, bc.exact(), n_instances=B, device=0)
    eng.set_option("ipm_nested", nested)
    ipm = BatchedIPM(eng)
    dense, sign, filled = _random_kkt_dense(ipm, eng.n, B, 11)
    assert filled > 4 * sign.size
    rhs = np.random.RandomState(5).uniform(-1, 1, size=(B, sign.size))
    sol, npos, nneg = ipm.debug_solve_dense(dense, rhs)
    ipm.close()
    eng.close()
    for bi in range(B):
        ref = np.linalg.solve(dense[bi], rhs[bi])
        assert np.max(np.abs(sol[bi] - ref)) <= 1e-11 * np.max(np.abs(ref)), bi
        assert npos[bi] == (sign > 0).sum() and nneg[bi] == (sign < 0).sum(), bi
    small_eng = NLPEngine(prob, bc.exact(), n_instances=3, device=0)
    small_eng.set_option("ipm_nested", nested)
    small = BatchedIPM(small_eng)
    pk = bc.picks(B)
    pk = pk + [pk[-1]] * (-len(pk) % 3)
    switched = nested == 1 and B > 256
    for upper in ((0, None) if switched else (None,)):       # None: the small solver as it was created
        if switched:
            small.set_option("upper_dense", 1 if upper is None else upper)   # (1: what it was created with)
        for k in range(0, len(pk), 3):
            three = pk[k:k + 3]
            s3, p3, n3 = small.debug_solve_dense(dense[three], rhs[three])
            for j, bi in enumerate(three):
                assert p3[j] == npos[bi] and n3[j] == nneg[bi], (bi, upper)
                if switched and upper is None:
                    assert np.max(np.abs(s3[j] - sol[bi])) <= 1e-11 * np.max(np.abs(sol[bi])), bi
                else:
                    assert bc.same_bits(s3[j], sol[bi]), (bi, upper, np.abs(s3[j] - sol[bi]).max())
    small.close()
    small_eng.close()


@pytest.mark.gpu
def test_factor_variant_switch(built):
    """choose_kernels' other dependence on B: sub-problems of 256 < rows <= 384 per block column are factored by kkt_factor_kernel's
    8-wave variant <3, 8> while B * sub-problems <= 512 and by the 4-wave variant <6> past that.  None of the problems above has
    such sub-problems; quadrotor(2, 12) has (3 sub-problems, asserted), so 171 instances run <6> and one instance <3, 8>.  The two
    take the same products in the same order: picks of a sweep with per-instance targets and starts equal solo bit for bit."""
    B = 171
    prob = problems.quadrotor(2, 12)
    prefs = bc.quadrotor_prefs(B)
    consts = [np.array(problems.quadrotor(2, 12, pref=p).GetOpimalProblemFuns().consts, dtype=np.float64) for p in prefs]
    eng, ipm = bc.batch(prob, bc.exact(), B, nested=1, consts=consts, **SWEEP_OPTS)
    sp = ipm.subproblems()
    rows = int(16 + (sp[:, 3] + sp[:, 2]).max())
    assert 256 < rows <= 384 and len(sp) * (B - 1) <= 512 < len(sp) * B, (rows, len(sp))
    guess = eng.get_starting_point()[:eng.n]
    X0 = np.stack([guess * (1 + 1e-2 * np.random.RandomState(5000 + bi).uniform(-1, 1, guess.size)) for bi in range(B)])
    r = bc.run(ipm, X0)
    assert (r["status"] == 0).all() and len(set(r["iterations"].tolist())) >= 2, (r["status"], r["iterations"])
    solo = bc.Solo(prob, bc.exact(), nested=1, **SWEEP_OPTS)
    for bi in bc.picks(B):
        bc.assert_same(r, bi, solo.solve(X0[bi], consts[bi]), 0, "solo")
    solo.close()
    ipm.close()
    eng.close()


def _perturbed_batch(prob, B, seed, **opts):
    eng, ipm = bc.batch(prob, bc.exact(), B, **opts)
    guess = eng.get_starting_point()[:eng.n]
    X0 = np.stack([guess * (1 + 1e-2 * np.random.RandomState(seed + bi).uniform(-1, 1, guess.size)) for bi in range(B)])
    return eng, ipm, X0


@pytest.mark.gpu
def test_assembly_grid_past_32_instances(built):
    """ipm_launch_assemble runs min(B <= 32 ? 2048 : 64, ceil(entries / 256)) workgroups per instance: quadrotor(8, 8) has 19970
    Jacobian entries (asserted: more than 64 * 256), so 33 instances are assembled by 64 workgroups each and one instance by 79.
    The assembly is reproducible by construction (the duplicates of a slot of K are summed by one thread in COO order, and at most
    two atomic adds land on a slot): picks equal solo."""
    B = 33
    prob = problems.quadrotor(8, 8)
    eng, ipm, X0 = _perturbed_batch(prob, B, 6000, **SWEEP_OPTS)
    assert max(eng.nnz_jac, eng.nnz_h) > 64 * 256 and eng.n + ipm.info()["n_slacks"] < 4096
    r = bc.run(ipm, X0)
    assert (r["status"] == 0).all(), r["status"]
    solo = bc.Solo(prob, bc.exact(), **SWEEP_OPTS)
    for bi in bc.picks(B):
        bc.assert_same(r, bi, solo.solve(X0[bi]), 0, "solo")
    solo.close()
    ipm.close()
    eng.close()


@pytest.mark.gpu
def test_large_instances_on_both_sides_of_32(built):
    """Instances of 4096 unknowns and more: up to 32 of them run the vector kernels with several workgroups of 1024 threads per
    instance (vec_combine adds their partial sums in a fixed order), 33 and more with one workgroup of 256 threads.  The two sum
    in different orders, and no option moves a solver from one side to the other — so across this edge a batch and a one-instance
    solve agree to rounding only: the iterates of quadrotor(32, 8) part in the last bits within two iterations.
    Asserted: 32 instances equal solo bit for bit (test_large_instances_in_a_batch_use_several_workgroups_each has 3); 33
    instances do not depend on their order, bit for bit, and end where solo ends by the bounds test_device_solve_nested_dissection_
    equals_band uses for two summation orders (same status, iterations within 1, obj within 1e-8 max(1, |obj|))."""
    prob = problems.quadrotor(32, 8)
    eng, ipm, X0 = _perturbed_batch(prob, 32, 6000, **SWEEP_OPTS)
    assert eng.n + ipm.info()["n_slacks"] >= 4096
    r32 = bc.run(ipm, X0)
    ipm.close()
    eng.close()
    eng, ipm, X0 = _perturbed_batch(prob, 33, 6000, **SWEEP_OPTS)
    r33 = bc.run(ipm, X0)
    perm = np.random.RandomState(79).permutation(33)
    bc.assert_permuted(r33, bc.run(ipm, X0[perm]), perm, "permutation")
    ipm.close()
    eng.close()
    assert (r32["status"] == 0).all() and (r33["status"] == 0).all()
    solo = bc.Solo(prob, bc.exact(), **SWEEP_OPTS)
    for bi in (0, 1, 30, 31, 32):
        one = solo.solve(X0[bi])
        if bi < 32:
            bc.assert_same(r32, bi, one, 0, "solo, 32 instances")
        assert one["status"][0] == r33["status"][bi]
        assert abs(int(one["iterations"][0]) - int(r33["iterations"][bi])) <= 1, bi
        assert abs(one["obj"][0] - r33["obj"][bi]) <= 1e-8 * max(1.0, abs(r33["obj"][bi])), bi
    solo.close()


# ------------------------------------------------------------------------------------------- 3. a heterogeneous sweep
def _sweep_batch(B, nested, s, **opts):
    eng, ipm = bc.batch(bc.quadrotor_problem(), bc.exact(), B, nested=nested, consts=s["consts"], **dict(SWEEP_OPTS, **opts))
    ipm.set_all_bounds(s["XL"], s["XU"])
    return eng, ipm


def _assert_mixed(r, B):
    fin = bc.finite(B)
    assert r["status"][bc.NAN_X0] == 5 and r["status"][bc.NAN_BOUND] == 5, r["status"]
    assert (r["status"][fin] == 0).all(), r["status"]
    its = r["iterations"][fin]
    assert len(set(its.tolist())) >= 3, its
    assert r["iterations"][bc.EARLY] <= its.max() - 5, (r["iterations"][bc.EARLY], its.max())


@pytest.mark.gpu
@pytest.mark.parametrize("nested", [0, 1], ids=["band", "nested"])
@pytest.mark.parametrize("B", [33, 260])
def test_heterogeneous_sweep(built, B, nested):
    """quadrotor(2, 4), exact Hessian: instances differ in constants, measured initial state and start; one starts at its own
    solution, one has a NaN in x0, one a NaN bound (status 5 from ipm_init_kernel).  The batch is mixed (asserted).  Picks equal
    solo bit for bit (nested at B = 260: solo with upper_dense 0, the last level on kkt_factor_kernel as choose_kernels decides
    past 256 instances; against solo at its defaults: same status, iterations within 1, obj within 1e-8 max(1, |obj|), the
    bounds of test_device_solve_nested_dissection_equals_band for two elimination orders).  The same batch in a random order
    gives every instance the same bits; one start moved by one bit changes that instance and no other; four picks agree with the
    restatement as in test_sweep_with_per_instance_targets.  stats()["iterations"] is the number of passes of ipm_solve_dev's
    loop in which some instance was still running: the largest per-instance count — an instance that ends with status 5 before
    its first pass (its count stays 0) never holds the loop."""
    s = bc.quadrotor_sweep(B)
    eng, ipm = _sweep_batch(B, nested, s)
    first = bc.run(ipm, s["X0"])
    _assert_mixed(first, B)
    assert first["iterations"][bc.NAN_X0] == 0 and first["iterations"][bc.NAN_BOUND] == 0
    assert first["stats"]["iterations"] == int(first["iterations"].max())
    pk = bc.picks(B, bc.SPECIAL)
    # solo
    switched = nested == 1 and B > 256
    solo = bc.Solo(bc.quadrotor_problem(), bc.exact(), nested=nested, upper_dense=0 if switched else None, **SWEEP_OPTS)
    for bi in pk:
        one = solo.solve(s["X0"][bi], s["consts"][bi], s["XL"][bi], s["XU"][bi])
        bc.assert_same(first, bi, one, 0, "solo")
    solo.close()
    if switched:
        solo = bc.Solo(bc.quadrotor_problem(), bc.exact(), nested=nested, **SWEEP_OPTS)
        for bi in pk:
            one = solo.solve(s["X0"][bi], s["consts"][bi], s["XL"][bi], s["XU"][bi])
            assert one["status"][0] == first["status"][bi], bi
            if first["status"][bi] == 0:
                assert abs(int(one["iterations"][0]) - int(first["iterations"][bi])) <= 1, bi
                assert abs(one["obj"][0] - first["obj"][bi]) <= 1e-8 * max(1.0, abs(first["obj"][bi])), bi
        solo.close()
    # the restatement
    for bi in [p for p in pk if p not in bc.SPECIAL][:4]:
        ref = bc.restatement(s, bi, max_iter=200)
        assert ref["status"] == 0 and first["status"][bi] == 0
        assert abs(int(first["iterations"][bi]) - ref["iterations"]) <= 1, bi
        assert abs(first["obj"][bi] - ref["obj"]) <= 1e-8 * max(1.0, abs(ref["obj"])), bi
    # permutation: constants, bounds and starts together
    perm = np.random.RandomState(77).permutation(B)
    assert not np.array_equal(perm, np.arange(B))
    for k, bi in enumerate(perm):
        eng.set_instance_constants(k, s["consts"][bi])
    XLp, XUp, X0p = bc.permuted(perm, s["XL"], s["XU"], s["X0"])
    ipm.set_all_bounds(XLp, XUp)
    second = bc.run(ipm, X0p)
    bc.assert_permuted(first, second, perm, "permutation")
    assert second["stats"]["iterations"] == first["stats"]["iterations"]
    # sensitivity: the last bit of one start
    for bi in range(B):
        eng.set_instance_constants(bi, s["consts"][bi])
    ipm.set_all_bounds(s["XL"], s["XU"])
    moved = B - 3
    assert moved not in bc.SPECIAL
    X0m = s["X0"].copy()
    j = s["free"][np.argmax(np.abs(X0m[moved, s["free"]]))]
    assert s["XL"][moved, j] < X0m[moved, j] < s["XU"][moved, j]
    X0m[moved, j] = np.nextafter(X0m[moved, j], np.inf)
    third = bc.run(ipm, X0m)
    assert not bc.same_bits(third["x"][moved], first["x"][moved])
    assert third["status"][moved] == 0
    for bi in range(B):
        if bi != moved:
            bc.assert_same(first, bi, third, bi, "neighbour of a moved start")
    ipm.close()
    eng.close()


# ------------------------------------------------------------------------------------------- 4. an iteration limit
@pytest.mark.gpu
def test_iteration_limit_splits_the_batch(built):
    """The sweep at B = 40 with max_iter strictly between the smallest and the largest iteration count of a first solve: some
    instances stop with status 2, the others converge, and every pick — the x of the stopped ones included — equals solo with
    the same limit."""
    B = 40
    s = bc.quadrotor_sweep(B)
    eng, ipm = _sweep_batch(B, None, s)
    free_run = ipm.solve(s["X0"])
    its = free_run["iterations"][bc.finite(B)]
    limit = int(its.min() + its.max()) // 2
    assert its.min() < limit < its.max(), its
    ipm.set_option("max_iter", limit)
    r = bc.run(ipm, s["X0"])
    fin = bc.finite(B)
    assert (r["status"][fin] == 2).any() and (r["status"][fin] == 0).any(), r["status"]
    assert set(r["status"].tolist()) == {0, 2, 5}
    assert (r["iterations"][r["status"] == 2] == limit).all()
    pk = bc.picks(B, bc.SPECIAL + (int(np.nonzero(r["status"] == 2)[0][0]), int(np.nonzero(r["status"] == 0)[0][-1])))
    assert (r["status"][pk] == 2).any() and (r["status"][pk] == 0).any()
    solo = bc.Solo(bc.quadrotor_problem(), bc.exact(), **dict(SWEEP_OPTS, max_iter=limit))
    for bi in pk:
        bc.assert_same(r, bi, solo.solve(s["X0"][bi], s["consts"][bi], s["XL"][bi], s["XU"][bi]), 0, "solo at the limit")
    solo.close()
    ipm.close()
    eng.close()


# ------------------------------------------------------------------------------------------- 5. modes
@pytest.mark.gpu
def test_modes_in_a_mixed_batch(built):
    """bryson_denham() on its default mesh, monotone barrier rule, tol 1e-6 (test_instances_of_a_batch_switch_modes_independently)
    at B = 40: the shipped guess (line search gives up -> restoration phase -> least-squares multipliers) at 0, 17, 32 and 39, the
    converged solution at 5 and 33, perturbed guesses elsewhere."""
    B = 40
    GUESS, SOLUTION = (0, 17, 32, 39), (5, 33)
    prob = problems.bryson_denham()
    o = orc.Oracle(prob, bc.exact())
    ref = ipm_oracle.solve(o, o.starting_point(), tol=1e-6, mu_strategy="monotone")
    assert ref["status"] == 0 and ref["restorations"] >= 1
    guess = o.starting_point()
    X0 = np.stack([guess * (1 + 1e-2 * np.random.RandomState(2000 + bi).uniform(-1, 1, o.n)) for bi in range(B)])
    X0[list(GUESS)] = guess
    X0[list(SOLUTION)] = ref["x"]
    opts = dict(tol=1e-6, mu_strategy="monotone", max_iter=400, trace=400)
    eng, ipm = bc.batch(prob, bc.exact(), B, **opts)
    r = bc.run(ipm, X0)
    assert (r["status"][list(GUESS + SOLUTION)] == 0).all(), r["status"]
    assert (r["restorations"][list(GUESS)] >= 1).all() and (r["restorations"][list(SOLUTION)] == 0).all(), r["restorations"]
    assert r["iterations"][SOLUTION[0]] < r["iterations"][GUESS[0]] - 5
    for bi in GUESS[1:]:
        bc.assert_same(r, GUESS[0], r, bi, "the same start twice in a batch")
    solo = bc.Solo(prob, bc.exact(), **opts)
    for bi in bc.picks(B, GUESS + SOLUTION):
        bc.assert_same(r, bi, solo.solve(X0[bi]), 0, "solo")
    solo.close()
    ipm.close()
    eng.close()


# ------------------------------------------------------------------------------------------- 6. limited memory
@pytest.mark.gpu
@pytest.mark.parametrize("B", [70, 260])
def test_limited_memory_hessian(built, B):
    """param_sled(2, 12), default options (limited-memory BFGS): 70 instances cross lb_decide_kernel's 64 per block, 260 cross
    lb_reset_kernel's 256.  Perturbed starts, instance 7 starts at a solution; picks against solo, and the batch in another order.
    The layout is the default one, nested dissection: past 256 instances its last level is factored by kkt_factor_kernel
    (choose_kernels), so solo runs with upper_dense 0 there — left at 1 its iterates part from the batch's at rounding level
    in the second iteration."""
    AT_SOLUTION = 7
    prob = problems.param_sled(2, 12)
    opts = dict(max_iter=300, trace=300)
    solo = bc.Solo(prob, Options(), upper_dense=0 if B > 256 else None, **opts)
    assert len(solo.ipm.subproblems()) > 1                      # nested dissection
    guess = solo.eng.get_starting_point()[:solo.eng.n]
    X0 = np.stack([guess * (1 + 1e-2 * np.random.RandomState(3000 + bi).uniform(-1, 1, guess.size)) for bi in range(B)])
    at = solo.solve(guess)
    assert at["status"][0] == 0
    X0[AT_SOLUTION] = at["x"][0]
    eng, ipm = bc.batch(prob, Options(), B, **opts)
    first = bc.run(ipm, X0)
    assert len(set(first["iterations"].tolist())) >= 3, first["iterations"]
    for bi in bc.picks(B, (AT_SOLUTION,)):
        bc.assert_same(first, bi, solo.solve(X0[bi]), 0, "solo")
    solo.close()
    perm = np.random.RandomState(78).permutation(B)
    second = bc.run(ipm, X0[perm])
    bc.assert_permuted(first, second, perm, "permutation")
    ipm.close()
    eng.close()


# ------------------------------------------------------------------------------------------- 7. gradient-based scaling
@pytest.mark.gpu
@pytest.mark.parametrize("mesh", [(8, 6), (32, 6)], ids=["8x6", "32x6"])
def test_gradient_based_scaling(built, mesh):
    """bryson_denham(8, 6) with nlp_scaling = 1 (the case of test_ipm_warm_start.py) and perturbed starts at B = 40, past the switch
    of the scaling kernels' grid at 32: every instance carries its own factors; lambda (unscaled), obj, the bound multipliers and
    the rest of the result equal solo.  The grid is min(B <= 32 ? 256 : 16, ceil(entries / 256)) workgroups per instance: the 8 x 6
    mesh's 1770 Jacobian entries take 7 on both sides of 32, so the 32 x 6 mesh (asserted: more than 16 * 256 entries) is the
    one on which 40 instances and one instance really run different grids."""
    B = 40
    prob = problems.bryson_denham(*mesh)
    opts = dict(max_iter=400, trace=400, nlp_scaling=1)
    solo = bc.Solo(prob, bc.exact(), **opts)
    assert (solo.eng.nnz_jac > 16 * 256) == (mesh == (32, 6))
    guess = solo.eng.get_starting_point()[:solo.eng.n]
    X0 = np.stack([guess * (1 + 2e-2 * np.random.RandomState(4000 + bi).uniform(-1, 1, guess.size)) for bi in range(B)])
    eng, ipm = bc.batch(prob, bc.exact(), B, **opts)
    r = bc.run(ipm, X0)
    assert (r["status"] == 0).all(), r["status"]
    assert len(set(np.round(r["lambda"][:, 0], 12))) > 1 or len(set(r["iterations"].tolist())) > 1
    for bi in bc.picks(B):
        bc.assert_same(r, bi, solo.solve(X0[bi]), 0, "solo")
    solo.close()
    ipm.close()
    eng.close()


# ------------------------------------------------------------------------------------------- 8. warm start, device pointers
@pytest.mark.gpu
def test_warm_start_and_device_pointer_forms_at_260(built):
    """From the band solve of the heterogeneous sweep at B = 260: the warm solve (options WARM of test_ipm_warm_start.py) from
    (x, lambda, z) against solo warm solves from the same triple; solve_dev on torch tensors against the host form, every
    instance; set_initial_states (host and device-pointer form, the flat index over B * nx) against set_all_bounds with those
    states, every instance."""
    import torch
    from lpopc_amd.engine import BatchedIPM
    from test_ipm_warm_start import WARM
    B = 260
    s = bc.quadrotor_sweep(B)
    eng, cold_s = _sweep_batch(B, 0, s)
    cold = bc.run(cold_s, s["X0"])
    _assert_mixed(cold, B)
    z = (cold["z_L"], cold["z_U"])
    warm_s = BatchedIPM(eng, **dict(SWEEP_OPTS, **WARM))
    warm_s.set_all_bounds(s["XL"], s["XU"])
    warm = bc.run(warm_s, cold["x"], cold["lambda"], z)
    fin = bc.finite(B)
    assert (warm["status"][fin] == 0).all() and warm["status"][bc.NAN_BOUND] == 5, warm["status"]
    solo = bc.Solo(bc.quadrotor_problem(), bc.exact(), nested=0, **dict(SWEEP_OPTS, **WARM))
    for bi in bc.picks(B, bc.SPECIAL):
        one = solo.solve(cold["x"][bi], s["consts"][bi], s["XL"][bi], s["XU"][bi], cold["lambda"][bi], (z[0][bi], z[1][bi]))
        bc.assert_same(warm, bi, one, 0, "solo, warm")
    solo.close()
    # the device-pointer form, cold and warm
    d_x = torch.from_numpy(s["X0"].copy()).cuda()
    d_l = torch.zeros((B, eng.m), dtype=torch.float64, device="cuda")
    dev = cold_s.solve_dev(d_x, d_l)
    torch.cuda.synchronize()
    assert bc.same_bits(d_x.cpu().numpy(), cold["x"]) and bc.same_bits(d_l.cpu().numpy(), cold["lambda"])
    for k in ("obj", "status", "iterations", "kkt_error"):
        assert bc.same_bits(dev[k], cold[k]), k
    d_x, d_l, d_zl, d_zu = (torch.from_numpy(a.copy()).cuda() for a in (cold["x"], cold["lambda"], z[0], z[1]))
    dev = warm_s.solve_dev(d_x, d_l, d_z_L=d_zl, d_z_U=d_zu, warm=True)
    torch.cuda.synchronize()
    for t, k in ((d_x, "x"), (d_l, "lambda"), (d_zl, "z_L"), (d_zu, "z_U")):
        assert bc.same_bits(t.cpu().numpy(), warm[k]), k
    for k in ("obj", "status", "iterations", "kkt_error"):
        assert bc.same_bits(dev[k], warm[k]), k
    warm_s.close()
    cold_s.close()
    # measured initial states of all 260
    plain = bc.quadrotor_sweep(B, special=False)
    states = np.ascontiguousarray(plain["XL"][:, bc.STATE0])
    by_bounds = BatchedIPM(eng, **SWEEP_OPTS)
    by_bounds.set_all_bounds(plain["XL"], plain["XU"])
    want = bc.run(by_bounds, plain["X0"])
    by_bounds.close()
    assert (want["status"] == 0).all()
    for form in ("host", "dev"):
        got_s = BatchedIPM(eng, **SWEEP_OPTS)              # a fresh solver: its bounds are the engine's
        if form == "host":
            got_s.set_initial_states(0, states)
        else:
            got_s.set_initial_states_dev(0, torch.from_numpy(states).cuda())
            torch.cuda.synchronize()
        got = bc.run(got_s, plain["X0"])
        for bi in range(B):
            bc.assert_same(want, bi, got, bi, "set_initial_states, " + form)
        got_s.close()
    eng.close()


# ------------------------------------------------------------------------------------------- 9. shares
@pytest.mark.gpu
@pytest.mark.parametrize("devices", [[0, 0], [0]], ids=["two_shares", "one_share"])
def test_shares_of_a_sweep(built, devices):
    """SweepGroup on the heterogeneous sweep's first 70 instances: the shares cover 0 .. 69 and every instance equals the
    one-engine B = 70 solve."""
    import ctypes as C
    from lpopc_amd.group import SweepGroup
    B = 70
    s = bc.quadrotor_sweep(B)
    eng, ipm = _sweep_batch(B, None, s)
    ref = bc.run(ipm, s["X0"])
    _assert_mixed(ref, B)
    ipm.close()
    eng.close()
    sw = SweepGroup(bc.quadrotor_problem(), devices, B, bc.exact(), max_iter=200)
    shares = sw.shares()
    assert len(shares) == len(devices) and shares[0][0] == 0 and sum(c for _, c in shares) == B
    assert all(shares[r][0] + shares[r][1] == shares[r + 1][0] for r in range(len(shares) - 1))
    for r, (i0, count) in enumerate(shares):
        e = sw._L.rpm_sweep_engine(sw._h, r)
        for bi in range(i0, i0 + count):
            c = np.ascontiguousarray(s["consts"][bi])
            assert sw._L.rpm_set_instance_constants(e, bi - i0, c.ctypes.data_as(C.POINTER(C.c_double)), c.size) == 0
    for bi in range(B):
        sw.set_bounds(bi, s["XL"][bi], s["XU"][bi])
    got = sw.solve(s["X0"])
    zl, zu = sw.bound_multipliers()
    for k in ("x", "lambda", "obj", "status", "iterations", "kkt_error"):
        for bi in range(B):
            assert bc.same_bits(got[k][bi], ref[k][bi]), (k, bi)
    assert bc.same_bits(zl, ref["z_L"]) and bc.same_bits(zu, ref["z_U"])
    assert sw.stats()["iterations"] == int(ref["iterations"].max())
    sw.close()
