"""Engine options "tile_order" and "store_policy" of the pipelined kernel (rpm_tile_pl_kernel): which tiles of a round a
half-workgroup takes, and with which cache policy the two bulk streams are stored.  Both are speed only: under every value
the kernel writes the bits the role-looped kernel writes, every entry exactly once.

launch(4, 16) has 64 nodes per phase = one tile per phase, nt = 4 tiles per instance; on a chip of 256 CUs the pipelined
kernel runs G = 512 halves (256 workgroups x 2).  With W = 4 B tiles, a half with slot s walks ceil((W - s) / G) tiles and a
workgroup executes as many barriers as its half 0 (whose slot is the lower of the two, tests/test_tile_order_host.py):
  B = 3    W = 12: 6 workgroups (a grid that is no multiple of 8: every order falls back to order 0), G = 12, every half
           one tile
  B = 129  W = 516 = G + 4: the halves with slots 0..3 walk two tiles, the others one.  Order 0: slots 0..3 are the halves of
           workgroups 0 and 8 (XCD 0).  Order 1 (S = 64 slots per XCD, quarters of Q = 16): XCD 0's slots are
           {0..15, 64..79, 128..143, 192..207}, so slots 0..3 are again workgroups 0 and 8, whose two halves both walk two tiles
  B = 641  W = 2564 = 5 G + 4: six tiles for slots 0..3, five for the rest
quadrotor(8, 8) (18 roles: the one-half shape, nt = 1, G = 256): B = 5 -> 5 workgroups of one tile (fallback to order 0);
B = 300 -> W = G + 44: slots 0..43 walk two tiles.
(Other chips: the same arithmetic with their CU count; the assertions do not depend on it.)
"""
import numpy as np
import pytest

from lpopc_amd import problems
from lpopc_amd.engine import NLPEngine

pytestmark = pytest.mark.gpu

ORDERS = (0, 1)
POLICIES = (0, 1, 2, 3)
_CACHE = {}


def _case(key):
    """Per problem and batch size, once: the iterates, g / values of the role-looped kernel (pipeline = 0) and of a
    one-instance engine for three sampled instances; all kept on the device and never written again."""
    if key in _CACHE:
        return _CACHE[key]
    import torch
    name, B = key
    prob = problems.launch(4, 16) if name == "launch" else problems.quadrotor(8, 8)
    one = NLPEngine(prob, device=0)
    xl, xu, _, _ = one.get_bounds_info()
    x0 = one.get_starting_point()
    xs = np.stack([problems.seeded_iterate(x0, xl, xu, 300 + i) for i in range(B)])
    dx = torch.from_numpy(xs).cuda()
    ref = NLPEngine(prob, n_instances=B, device=0, role_loop=1)
    ref.set_option("pipeline", 0)
    ref.set_option("instance_align", 16)
    sg, sv = ref.get_option("stride_g"), ref.get_option("stride_values")
    g = torch.full((B, sg), np.nan, dtype=torch.float64, device="cuda")
    v = torch.full((B, sv), np.nan, dtype=torch.float64, device="cuda")
    ref.eval_pair_dev(dx, g, v)
    torch.cuda.synchronize()
    assert ref.get_option("pipeline_active") == 0
    m, nnz = ref.m, ref.nnz_jac
    assert not torch.isnan(g[:, :m]).any() and not torch.isnan(v[:, :nnz]).any()
    sampled = {}
    for i in sorted({0, B // 2, B - 1}):
        g1 = torch.full((m,), np.nan, dtype=torch.float64, device="cuda")
        v1 = torch.full((nnz,), np.nan, dtype=torch.float64, device="cuda")
        one.eval_pair_dev(dx[i], g1, v1)
        torch.cuda.synchronize()
        sampled[i] = (g1, v1)
        assert torch.equal(g[i, :m], g1) and torch.equal(v[i, :nnz], v1)
    one.close()
    ref.close()
    _CACHE[key] = dict(prob=prob, B=B, dx=dx, g=g, v=v, m=m, nnz=nnz, sg=sg, sv=sv, sampled=sampled)
    return _CACHE[key]


def _pipelined(c, order, policy, persistent=False):
    eng = NLPEngine(c["prob"], n_instances=c["B"], device=0, role_loop=1)
    eng.set_option("pipeline", 1)
    eng.set_option("instance_align", 16)
    eng.set_option("tile_order", order)
    eng.set_option("store_policy", policy)
    if persistent:
        eng.set_option("persistent_values", 1)
    assert (eng.get_option("tile_order"), eng.get_option("store_policy")) == (order, policy)
    assert (eng.get_option("stride_g"), eng.get_option("stride_values")) == (c["sg"], c["sv"])
    return eng


def _check(c, g, v):
    import torch
    m, nnz = c["m"], c["nnz"]
    assert not torch.isnan(g[:, :m]).any() and not torch.isnan(v[:, :nnz]).any()      # an entry nobody wrote
    assert torch.equal(g[:, :m], c["g"][:, :m]) and torch.equal(v[:, :nnz], c["v"][:, :nnz])
    assert torch.isnan(g[:, m:]).all() and torch.isnan(v[:, nnz:]).all()                # the padding between instances is nobody's
    for i, (g1, v1) in c["sampled"].items():
        assert torch.equal(g[i, :m], g1) and torch.equal(v[i, :nnz], v1)


def _run(c, order, policy):
    import torch
    eng = _pipelined(c, order, policy)
    g = torch.full((c["B"], c["sg"]), np.nan, dtype=torch.float64, device="cuda")
    v = torch.full((c["B"], c["sv"]), np.nan, dtype=torch.float64, device="cuda")
    eng.eval_pair_dev(c["dx"], g, v)
    torch.cuda.synchronize()
    assert eng.get_option("pipeline_active") == 1
    _check(c, g, v)
    eng.close()


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("B", [3, 129, 641])
def test_every_order_and_policy_writes_the_role_looped_kernels_bits(built, B, order, policy):
    _run(_case(("launch", B)), order, policy)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("B", [5, 300])
def test_one_half_shape(built, B, order, policy):
    _run(_case(("quadrotor", B)), order, policy)


def test_persistent_values_under_every_order_and_policy(built):
    """The constant block skipped (the second launch into an array the engine filled before): the Jacobian stream alone,
    with the other iterates' values where the first launch left the constant block."""
    import torch
    c = _case(("launch", 129))
    dx2 = torch.roll(c["dx"], 1, 0)                      # instance i evaluates iterate i - 1
    for order in ORDERS:
        for policy in POLICIES:
            eng = _pipelined(c, order, policy, persistent=True)
            g = torch.full((c["B"], c["sg"]), np.nan, dtype=torch.float64, device="cuda")
            v = torch.full((c["B"], c["sv"]), np.nan, dtype=torch.float64, device="cuda")
            eng.eval_pair_dev(dx2, g, v)
            torch.cuda.synchronize()
            assert torch.equal(v[:, :c["nnz"]], torch.roll(c["v"], 1, 0)[:, :c["nnz"]])
            g.fill_(np.nan)
            marker_at = c["nnz"] - 5                     # inside the constant block (the tail of `values`)
            v[:, marker_at] = 4711.0
            torch.cuda.synchronize()
            eng.eval_pair_dev(c["dx"], g, v)
            torch.cuda.synchronize()
            assert eng.get_option("pipeline_active") == 1
            assert bool((v[:, marker_at] == 4711.0).all())    # skipped, not rewritten
            v[:, marker_at] = c["v"][:, marker_at]
            _check(c, g, v)
            eng.close()


def test_option_values_are_checked(built):
    from lpopc_amd.engine import RpmError
    eng = NLPEngine(problems.launch(4, 16), n_instances=3, device=0, role_loop=1)
    assert (eng.get_option("tile_order"), eng.get_option("store_policy")) in [(o, p) for o in ORDERS for p in POLICIES]
    for key, bad in (("tile_order", -1), ("tile_order", len(ORDERS)), ("store_policy", -1), ("store_policy", len(POLICIES))):
        with pytest.raises(RpmError):
            eng.set_option(key, bad)
    eng.close()
