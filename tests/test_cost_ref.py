"""The restatement of the cost-to-go contract (tests/cost_ref.py) against itself, without a GPU: the closed form of an
open box, the two Dijkstras against each other, and every wrong reading of the header caught on a case that names
it."""
import numpy as np

import cost_ref as ref
import esdf_ref

VS = 0.01
U, FR, OC = ref.UNKNOWN, ref.FREE, ref.OCCUPIED


def _goal_idx(shape, *goals):
    Z, Y, X = shape
    return np.unique([x + X * (y + Y * z) for x, y, z in goals])


def test_closed_form_of_an_open_box():
    shape, goal = (9, 12, 20), (7, 5, 3)
    trav = np.ones(shape, dtype=bool)
    want = ref.closed_form(shape, goal)
    assert want[3, 5, 7] == 0 and want[3, 5, 9] == 20 and want[4, 6, 8] == 17 and want[3, 6, 8] == 14
    for fn in (ref.dijkstra_heap, ref.dijkstra_scipy):
        assert ref.same_bytes(fn(trav, _goal_idx(shape, goal)), want)
    faces = ref.dijkstra_heap(trav, _goal_idx(shape, goal), faces_only=True)
    z, y, x = np.indices(shape)
    assert np.array_equal(faces, 10 * (abs(x - 7) + abs(y - 5) + abs(z - 3)))


def test_the_two_dijkstras_agree():
    trav = ref.random_mask((20, 30, 40), 0.7, seed=3)
    idx = np.flatnonzero(trav.reshape(-1))[[0, 777, 5000]]
    for faces_only in (False, True):
        a = ref.dijkstra_heap(trav, idx, faces_only)
        assert ref.same_bytes(a, ref.dijkstra_scipy(trav, idx, faces_only))
        assert (a == ref.NONE).sum() > (~trav).sum() or not faces_only   # face moves leave some pockets cut off
        assert ref.unconverged_ok(a, a, trav, idx, faces_only)     # an exact field has the three properties too
    assert ref.same_bytes(ref.dijkstra_scipy(trav, np.array([], dtype=np.int64)),
                          np.full(trav.shape, ref.NONE, dtype=np.uint32))


def test_wrong_variants_are_caught():
    # faces only where 26 moves are asked for; weights 10 / 14 / 18: the corner neighbour of the goal
    trav = np.ones((3, 3, 3), dtype=bool)
    idx = _goal_idx(trav.shape, (0, 0, 0))
    right = ref.exact(trav, idx)
    assert right[1, 1, 1] == 17 and right[0, 1, 1] == 14
    assert ref.dijkstra_heap(trav, idx, faces_only=True)[1, 1, 1] == 30
    assert ref.dijkstra_heap(trav, idx, weights=(0, 10, 14, 18))[1, 1, 1] == 18

    # clearance tested with <= instead of <: a voxel exactly two voxels from the obstacle, clearance 2 * vs
    state = np.full((1, 1, 6), FR, dtype=np.uint8)
    state[0, 0, 0] = OC
    clearance = float(np.float32(2) * np.float32(VS))
    field = esdf_ref.esdf(state, VS)
    assert field[0, 0, 2] == np.float32(clearance)
    trav = ref.traversable(state, VS, clearance)
    assert trav.reshape(-1).tolist() == [False, False, True, True, True, True]
    wrong = ~esdf_ref.obstacles(state) & ~(field <= np.float32(clearance))
    assert wrong.reshape(-1).tolist() == [False, False, False, True, True, True]

    # an ESDF that sees an obstacle outside the box: the box is the world's x >= 1, the obstacle sits at x = 0
    world = np.full((1, 1, 6), FR, dtype=np.uint8)
    world[0, 0, 0] = OC
    box = world[:, :, 1:]
    assert ref.traversable(box, VS, 2.5 * VS).all()               # not seen: +inf everywhere
    seen = esdf_ref.esdf(world, VS)[:, :, 1:]
    assert not ref.traversable(box, VS, 2.5 * VS, field=seen)[0, 0, 0]

    # a non-traversable goal accepted: it would be a source inside the wall
    state = np.full((1, 3, 5), FR, dtype=np.uint8)
    state[0, :, 2] = OC
    trav = ref.traversable(state, VS)
    goals = [[2, 1, 0], [0, 1, 0], [0, 1, 0], [-1, 0, 0], [5, 1, 0]]       # wall, free, duplicate, outside, outside
    idx = ref.accept(goals, [0, 0, 0], trav)
    assert idx.tolist() == [5]
    right = ref.exact(trav, idx)
    assert np.all(right[0, :, 3:] == ref.NONE) and ref.summary_of(right, trav)["goals"] == 1
    wrong = ref.dijkstra_heap(np.ones_like(trav), np.array([5, 7]))
    assert wrong[0, 1, 3] == 10

    # the largest code on a tie: between two goals, the edge moves to either cost the same
    trav = np.ones((1, 2, 3), dtype=bool)
    idx = _goal_idx(trav.shape, (0, 0, 0), (2, 0, 0))
    cost = ref.exact(trav, idx)
    assert cost[0, 1, 1] == 14                                    # through (0, 0, 0) or through (2, 0, 0)
    assert ref.next_of(cost, trav)[0, 1, 1] == 0 + 3 * 0 + 9 * 1   # dx = -1, dy = -1, dz = 0: code 9
    assert ref.next_of(cost, trav, largest_code=True)[0, 1, 1] == 2 + 3 * 0 + 9 * 1
    assert ref.next_of(cost, trav)[0, 0, 0] == ref.AT_GOAL

    # a single relaxation round on the serpentine reaches the goal's neighbours only
    trav = ref.serpentine((9, 20, 70))
    idx = ref.accept([[0, 0, 0]], [0, 0, 0], trav)
    right = ref.exact(trav, idx)
    once = ref.relax_once(trav, idx)
    assert (right != ref.NONE).sum() == trav.sum() and (once != ref.NONE).sum() == 2
    assert not ref.same_bytes(once, right)
    assert ref.unconverged_ok(once, right, trav, idx)             # ... but it is a field of the bounded form
    broken = once.copy()
    broken[0, 0, 5] = 50                                          # a finite value no neighbour accounts for
    assert not ref.unconverged_ok(broken, right, trav, idx)
    low = right.copy()
    low[0, 0, 5] -= 1                                             # below the exact cost
    assert not ref.unconverged_ok(low, right, trav, idx)


def test_summary_and_descent_helpers():
    import ratsdf
    trav = ref.random_mask((5, 9, 13), 0.8, seed=1)
    idx = np.flatnonzero(trav.reshape(-1))[[3, 40]]
    cost = ref.exact(trav, idx)
    s = ref.summary_of(cost, trav)
    assert s["goals"] == 2 and s["traversable"] == trav.sum() and s["reached"] == (cost != ref.NONE).sum()
    assert s["max_cost"] == cost[cost != ref.NONE].max() and s.dtype == ratsdf.COST_SUMMARY_DTYPE
    nxt = ref.next_of(cost, trav)
    origin = [-4, 7, 100]
    Z, Y, X = trav.shape
    for i in np.flatnonzero((cost != ref.NONE).reshape(-1)):
        start = [origin[0] + i % X, origin[1] + i // X % Y, origin[2] + i // (X * Y)]
        path = ratsdf.descend(nxt, origin, start)
        assert ref.path_weight(path) == cost.reshape(-1)[i]
        end = path[-1] - origin
        assert cost[end[2], end[1], end[0]] == 0
    assert ratsdf.cost_direction(9) == (-1, -1, 0) and ratsdf.COST_NONE == ref.NONE
