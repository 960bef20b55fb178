"""The tile orders of the pipelined kernel (engine option "tile_order") as pure index arithmetic, on the host
(rpm_debug_tile_slot = pl_tile_slot of rpm_device_internal.hpp, the function the kernel calls): half `half` of workgroup b
walks tiles slot, slot + G, ... < W, G = nh * nb.  For every order and every grid a launch can have, every tile of [0, W) is
visited exactly once, half 0 of a workgroup walks at least as many tiles as half 1 (its count is the workgroup's barrier
count, and at least one), and a half's next tile is G further (the staged record of the tile after the current one)."""
import pytest

from lpopc_amd.engine import ABI_SYMBOLS, lib

ORDERS = (0, 1)


def _grid(W, nh, slots):
    """launch_tile_pl: the halves of a launch (at most the resident ones) and its workgroups"""
    halves = min(W, slots)
    return (halves + nh - 1) // nh


def _tiles_of(L, order, nh, nb, b, half, W):
    s = L.rpm_debug_tile_slot(order, nh, nb, b, half)
    G = nh * nb
    n_iter = (W - s + G - 1) // G if s < W else 0          # the kernel's n_iter
    return s, [s + j * G for j in range(n_iter)]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("nh,cus", [(2, 256), (1, 256), (2, 304), (2, 60), (1, 8)])
def test_every_tile_is_visited_exactly_once(built, order, nh, cus):
    L = lib()
    assert "rpm_debug_tile_slot" in ABI_SYMBOLS
    slots = nh * cus
    # the batch sizes of tests/test_gpu_tile_order.py (4 tiles and 1 tile per instance), the metric launch, and every small grid
    Ws = sorted({12, 516, 2564, 5, 300, 4096, slots - 1, slots, slots + 1, 2 * slots + 7} | set(range(1, 80)))
    for W in Ws:
        nb = _grid(W, nh, slots)
        G = nh * nb
        seen = []
        for b in range(nb):
            s0, t0 = _tiles_of(L, order, nh, nb, b, 0, W)
            assert 0 <= s0 < G and len(t0) >= 1, (W, b)
            seen += t0
            if nh == 2:
                s1, t1 = _tiles_of(L, order, nh, nb, b, 1, W)
                assert s0 < s1 < G and len(t1) <= len(t0), (W, b)
                seen += t1
        assert sorted(seen) == list(range(W)), (order, nh, cus, W)


def test_the_orders_on_the_full_chip(built):
    """256 workgroups of two halves, G = 512, S = 64 slots per XCD (workgroups b, b + 8, ... share XCD b % 8)."""
    L = lib()
    for xcd in range(8):
        for order, want in ((0, set(range(64 * xcd, 64 * xcd + 64))),
                            (1, {256 * (xcd // 4) + 64 * r + 16 * (xcd % 4) + t for r in range(4) for t in range(16)})):
            got = {L.rpm_debug_tile_slot(order, 2, 256, b, h) for b in range(xcd, 256, 8) for h in (0, 1)}
            assert got == want, (order, xcd)
    # the grids of the three batch sizes of tests/test_gpu_tile_order.py: tiles per half
    for order in ORDERS:
        for W, nb, counts in ((12, 6, {1: 12}), (516, 256, {2: 4, 1: 508}), (2564, 256, {6: 4, 5: 508})):
            n = {}
            for b in range(nb):
                for h in (0, 1):
                    k = len(_tiles_of(L, order, 2, nb, b, h, W)[1])
                    n[k] = n.get(k, 0) + 1
            assert n == counts, (order, W, n)


def test_bad_arguments(built):
    L = lib()
    for args in ((-1, 2, 8, 0, 0), (len(ORDERS), 2, 8, 0, 0), (0, 0, 8, 0, 0), (0, 2, 0, 0, 0), (0, 2, 8, 8, 0), (0, 2, 8, 0, 2)):
        assert L.rpm_debug_tile_slot(*args) == -1
