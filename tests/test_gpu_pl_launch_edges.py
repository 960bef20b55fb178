"""The pipelined tile kernel's launch edges and tile order: its halves walk tiles w, w + G, ... in an XCD-aware order of the
workgroups, so the first and the last tile of a half, idle halves and the halves of one workgroup with unequal tile
counts all move with the grid.  Bit for bit against the role-looped kernel (`pipeline` 1 against 0) on NaN-filled
outputs: every half one tile (B = 1), halves with one tile more than others, unequal halves inside a workgroup, packed and
padded instances (the `head` path of the line-aligned constant stores), persistent `values` (the skipped constant shares
are never written) and interval shards."""
import numpy as np
import pytest

from lpopc_amd import problems
from lpopc_amd.engine import NLPEngine

pytestmark = pytest.mark.gpu


def _ragged_odd():
    """Delta-III on ragged meshes with 5 tiles of 64 nodes (phase 0 has two): with an odd instance count the halves of
    one workgroup get unequal tile counts.  Intervals of at most 33 nodes keep every tile's constant share within the
    pipelined kernel's limit."""
    p = problems.launch()
    meshes = [([-1, -0.8, -0.5, -0.45, -0.1, 0.3, 1], [5, 16, 2, 16, 16, 16]), ([-1, 0.5, 1], [16, 17]), ([-1, 1], [33]),
              ([-1, -0.9, -0.5, 0.0, 0.25, 1], [3, 4, 7, 12, 16])]
    for i, (mesh, nodes) in enumerate(meshes):
        problems.set_mesh(p.GetPhase(i), mesh, nodes)
    return p


def _iterates(prob, B, seed0):
    one = NLPEngine(prob, device=0)
    xl, xu, _, _ = one.get_bounds_info()
    x0 = one.get_starting_point()
    one.close()
    return np.stack([problems.seeded_iterate(x0, xl, xu, seed0 + i) for i in range(B)])


def _engines(prob, B, align=None, **kw):
    out = []
    for pipeline in (0, 1):
        e = NLPEngine(prob, n_instances=B, device=0, role_loop=1, **kw)
        e.set_option("pipeline", pipeline)
        if align is not None:
            e.set_option("instance_align", align)
        out.append(e)
    return out


def _bits(t):
    import torch
    return t.contiguous().view(-1).view(torch.int64)


def _evaluate(eng, dx, B):
    """fused pair and the Jacobian-only launch into NaN-filled arrays of the engine's instance strides"""
    import torch
    sg, sv = eng.get_option("stride_g"), eng.get_option("stride_values")
    dg = torch.full((B, sg), np.nan, dtype=torch.float64, device="cuda")
    dv = torch.full((B, sv), np.nan, dtype=torch.float64, device="cuda")
    dv2 = torch.full((B, sv), np.nan, dtype=torch.float64, device="cuda")
    eng.eval_pair_dev(dx, dg, dv)
    eng.eval_jac_g_dev(dx, dv2)
    torch.cuda.synchronize()
    return dg, dv, dv2


def _check_same(ref, pl, B, xs, complete=True):
    import torch
    dx = torch.from_numpy(xs).cuda()
    a = _evaluate(ref, dx, B)
    assert ref.get_option("pipeline_active") == 0
    b = _evaluate(pl, dx, B)
    assert pl.get_option("pipeline_active") == 1
    m, nnz = pl.m, pl.nnz_jac
    if complete:   # every entry of g and values written (the padding words stay NaN in both)
        assert not bool(torch.isnan(b[0][:, :m]).any()) and not bool(torch.isnan(b[1][:, :nnz]).any())
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))
    assert torch.equal(_bits(b[1]), _bits(b[2]))


@pytest.mark.parametrize("B", [1, 18, 64])
def test_metric_problem(built, B):
    """B = 1: every half walks one tile (its last); 18: some halves one tile more than others; 64: the bench shape."""
    prob = problems.config("launch")
    ref, pl = _engines(prob, B)
    _check_same(ref, pl, B, _iterates(prob, B, 500))
    ref.close()
    pl.close()


@pytest.mark.parametrize("B", [3, 301])
def test_ragged_mesh_unequal_halves(built, B):
    """5 tiles per instance: W = 15 leaves the last workgroup's second half idle; W = 1505 gives the two halves of one
    workgroup unequal tile counts (and every half two or three tiles)."""
    prob = _ragged_odd()
    ref, pl = _engines(prob, B)
    assert pl.get_option("n_tiles") == 5
    _check_same(ref, pl, B, _iterates(prob, B, 700))
    ref.close()
    pl.close()


@pytest.mark.parametrize("align", [1, 16])
@pytest.mark.parametrize("mesh,B", [("metric", 23), ("ragged", 111)])
def test_instance_align(built, mesh, B, align):
    """instance_align 1 (packed: the constant copies start anywhere inside a 128-byte line, the `head` elements run) and
    16 (every instance on a line)."""
    prob = problems.config("launch") if mesh == "metric" else _ragged_odd()
    ref, pl = _engines(prob, B, align=align)
    _check_same(ref, pl, B, _iterates(prob, B, 900))
    ref.close()
    pl.close()


def test_persistent_values_keeps_the_last_tiles_share(built):
    """persistent_values: the second call skips the constant block, the last tiles' shares included — a marker planted in
    each instance's last constant entry (the last phase's last tile) survives, and everything else equals the role-looped
    kernel's complete evaluation."""
    import torch
    prob, B = _ragged_odd(), 37
    ref, pl = _engines(prob, B)
    pl.set_option("persistent_values", 1)
    xs = [torch.from_numpy(_iterates(prob, B, 1100 + 100 * r)).cuda() for r in range(2)]
    nnz = pl.nnz_jac
    dg = torch.empty((B, pl.m), dtype=torch.float64, device="cuda")
    dv = torch.full((B, nnz), np.nan, dtype=torch.float64, device="cuda")
    rv = torch.empty((B, nnz), dtype=torch.float64, device="cuda")
    pl.eval_pair_dev(xs[0], dg, dv)
    ref.eval_pair_dev(xs[0], dg, rv)
    torch.cuda.synchronize()
    assert pl.get_option("pipeline_active") == 1 and ref.get_option("pipeline_active") == 0
    assert torch.equal(dv, rv)
    marker_at = nnz - 5                     # inside the last Doffdiag copy (the CONST block is the tail)
    assert bool((dv[:, marker_at] == dv[0, marker_at]).all())
    dv[:, marker_at] = 4711.0
    pl.eval_pair_dev(xs[1], dg, dv)
    ref.eval_pair_dev(xs[1], dg, rv)
    torch.cuda.synchronize()
    assert bool((dv[:, marker_at] == 4711.0).all())
    dv[:, marker_at] = rv[:, marker_at]
    assert torch.equal(dv, rv)
    ref.close()
    pl.close()


def test_interval_shards(built):
    """Interval-sharded engines (shard_world 3): each rank walks its own n_my_tiles; entries of the other ranks stay NaN
    in both kernels."""
    prob, B, world = problems.config("launch"), 5, 3
    xs = _iterates(prob, B, 1300)
    for r in range(world):
        ref, pl = _engines(prob, B, shard_mode=1, shard_rank=r, shard_world=world)
        _check_same(ref, pl, B, xs, complete=False)
        ref.close()
        pl.close()
