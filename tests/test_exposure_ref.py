"""The numpy restatement of the exposure contract (tests/exposure_ref.py) against hand-written cases, and each
deliberate deviation it can imitate caught on a named case (no GPU needed)."""
import numpy as np
import pytest

import exposure_ref as ref

F = np.float32
VS = 0.01
FR, OC = ref.FREE, ref.OCCUPIED

# the voxels of four walks from (0, 0, 0), written out by hand from the rule: the axis with the smallest
# (2 k + 1) / n among those with steps left, a tie to the lowest axis
WALKS = {
    (3, 1, 0): [(0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 1, 0), (3, 1, 0)],   # 1/3 | 3/3 = 1/1: tie, x | 5/3 > 1: y | x
    (5, 5, 0): [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (2, 2, 0), (3, 2, 0), (3, 3, 0), (4, 3, 0), (4, 4, 0),
                (5, 4, 0), (5, 5, 0)],                                    # every pair of steps starts with a tie
    (4, 4, 4): [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 2), (3, 3, 2),
                (3, 3, 3), (4, 3, 3), (4, 4, 3), (4, 4, 4)],
    (6, 3, 0): [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0), (3, 2, 0), (4, 2, 0), (5, 2, 0), (5, 3, 0),
                (6, 3, 0)],                                               # x at 1 3 5 7 9 11 /6, y at 2 6 10 /6: no tie
}


@pytest.mark.parametrize("end", list(WALKS))
def test_hand_written_walks_and_their_reverses(end):
    cells = WALKS[end]
    assert ref.walk((0, 0, 0), end) == cells
    assert len(cells) == sum(end) + 1
    assert all(sum(abs(a - b) for a, b in zip(u, v)) == 1 for u, v in zip(cells, cells[1:]))      # 6-connected
    # the reverse takes the same axes in the same order from the other end: the mirror image, not the same voxels
    back = ref.walk(end, (0, 0, 0))
    e = np.array(end)
    assert back == [tuple(int(v) for v in e - np.array(c)) for c in cells]
    # any octant and any offset: the same steps with the signs of the direction
    for sign in ((1, -1, 1), (-1, -1, -1), (-1, 1, -1)):
        s = np.array(sign)
        off = np.array([7, -3, 11])
        assert ref.walk(off, off + s * e) == [tuple(int(v) for v in off + s * np.array(c)) for c in cells]


def test_reverse_of_a_tie_walk_visits_other_voxels():
    assert ref.walk((3, 1, 0), (0, 0, 0)) == [(3, 1, 0), (2, 1, 0), (1, 1, 0), (1, 0, 0), (0, 0, 0)]
    assert (2, 0, 0) in WALKS[(3, 1, 0)] and (2, 0, 0) not in ref.walk((3, 1, 0), (0, 0, 0))


def test_vectorised_walks_equal_the_single_walk():
    rng = np.random.default_rng(0)
    blocking = rng.random((9, 10, 11)) < 0.08
    s = np.stack([rng.integers(0, 11, 300), rng.integers(0, 10, 300), rng.integers(0, 9, 300)], 1)
    L = np.stack([rng.integers(0, 11, 300), rng.integers(0, 10, 300), rng.integers(0, 9, 300)], 1)
    want = [not any(blocking[z, y, x] for x, y, z in ref.walk(a, b)) for a, b in zip(s, L)]
    assert ref.clear_walks(blocking, s, L).tolist() == want and 20 < sum(want) < 280


def _floor(shape=(8, 8, 8)):
    state = np.full(shape, FR, dtype=np.uint8)
    state[0] = OC
    return state


def test_lamp_straight_above_a_point():
    """P / 4 pi r^2 with cos(theta) = 1, and P cos / 4 pi r^2 off the axis"""
    state = _floor()
    points = ref.make_points([[0.03, 0.03, 0.004]], [0, 0, 1], prob=0.7)
    lamps = ref.make_lamps([[0.03, 0.03, 0.054], [0.06, 0.03, 0.044]], [2.0, 3.0])
    dose, mask, table, summary = ref.exposure(state, [0, 0, 0], VS, points, lamps)
    r0, r1 = 0.05, 0.05
    want = 2.0 / (4 * np.pi * r0 * r0) + 3.0 * (0.04 / r1) / (4 * np.pi * r1 * r1)
    assert mask[0] == 3 and abs(dose[0] - want) < 1e-5 * want
    assert table.tolist() == [(1, 1, 1, 0), (1, 1, 1, 0)]
    assert (summary["lit_pairs"], summary["points_lit"], summary["points_outside"], summary["lamps_accepted"]) == (2, 1, 0, 2)
    _, _, table, _ = ref.exposure(state, [0, 0, 0], VS, points, lamps, min_irradiance=70.0, p_cutoff=0.8)
    assert table.tolist() == [(1, 0, 0, 0), (1, 1, 0, 0)]            # 63.7 and 76.4 W/m^2; prob 0.7 < 0.8
    # a lamp in the floor is not accepted, one beyond the box neither; the point under the floor is OUTSIDE
    lamps = ref.make_lamps([[0.03, 0.03, 0.0], [0.03, 0.03, 0.09]])
    points = ref.make_points([[0.03, 0.03, 0.004], [0.03, 0.03, 0.004]], [[0, 0, 1], [0, 0, -1]])
    dose, mask, table, summary = ref.exposure(state, [0, 0, 0], VS, points, lamps, dose=np.array([1.5, 2.5], dtype=F))
    assert table["accepted"].tolist() == [0, 0] and mask.tolist() == [0, 0] and dose.tolist() == [1.5, 2.5]
    assert summary["points_outside"] == 1 and summary["lamps_accepted"] == 0


def _differs(state, origin, points, lamps, wrong, **kw):
    good = ref.exposure(state, origin, VS, points, lamps, **kw)
    bad = ref.exposure(state, origin, VS, points, lamps, wrong=wrong, **kw)
    return not (ref.same_bytes(good[0], bad[0]) and ref.same_bytes(good[1], bad[1]))


def test_ties_to_the_highest_axis_are_caught():
    """(5, 5, 0): the contract visits (1, 0, 0), the deviation (0, 1, 0)"""
    for blocker, visible in (((1 + 1, 1 + 0, 1), 0), ((1 + 0, 1 + 1, 1), 1)):
        state = np.full((8, 8, 8), FR, dtype=np.uint8)
        state[blocker[2], blocker[1], blocker[0]] = OC
        points = ref.make_points([[0.0, 0.01, 0.01]], [1, 0, 0])       # start voxel (1, 1, 1)
        lamps = ref.make_lamps([[0.06, 0.06, 0.01]])                   # voxel (6, 6, 1)
        assert ref.exposure(state, [0, 0, 0], VS, points, lamps)[1][0] == visible
        assert ref.exposure(state, [0, 0, 0], VS, points, lamps, wrong="ties_highest")[1][0] == 1 - visible


def test_a_26_connected_line_is_caught():
    """a diagonal wall whose voxels touch by edges: the walk is stopped, Bresenham's line slips through"""
    state = np.full((1, 8, 8), FR, dtype=np.uint8)
    for k in range(8):
        state[0, k, 7 - k] = OC
    points = ref.make_points([[0.0, 0.01, 0.0]], [1, 0, 0])           # start voxel (1, 1, 0)
    lamps = ref.make_lamps([[0.06, 0.06, 0.0]])                       # voxel (6, 6, 0): the line jumps (3, 3) -> (4, 4)
    assert ref.exposure(state, [0, 0, 0], VS, points, lamps)[1][0] == 0
    assert ref.exposure(state, [0, 0, 0], VS, points, lamps, wrong="bresenham")[1][0] == 1


def test_a_descending_sum_is_caught():
    """a near lamp and two far ones: (big + small) + small != (small + small) + big in fp32"""
    state = _floor((16, 8, 8))
    points = ref.make_points([[0.03, 0.03, 0.004]], [0, 0, 1])
    lamps = ref.make_lamps([[0.03, 0.03, 0.014], [0.05, 0.03, 0.14], [0.02, 0.05, 0.15]], [5.0, 0.37, 0.41])
    assert ref.exposure(state, [0, 0, 0], VS, points, lamps)[1][0] == 7
    found = False
    for power in np.linspace(0.3, 0.5, 40):
        lamps["power"][2] = power
        found = found or _differs(state, [0, 0, 0], points, lamps, "descending")
    assert found


def test_a_contracted_dot_product_is_caught():
    state = _floor()
    rng = np.random.default_rng(4)
    points = ref.make_points(rng.uniform(0.0, 0.07, (200, 3)) * [1, 1, 0] + [0, 0, 0.004], [0, 0, 1])
    n = rng.normal(size=(200, 3)) + [0, 0, 2]
    points["normal"] = (n / np.linalg.norm(n, axis=1, keepdims=True) * 0.9).astype(F)
    lamps = ref.make_lamps(rng.uniform(0.0, 0.07, (8, 3)) * [1, 1, 0.6] + [0, 0, 0.02])
    assert _differs(state, [0, 0, 0], points, lamps, "contracted")


def test_facing_with_equality_is_caught():
    """a lamp exactly in the point's tangent plane: c == 0.0f, not facing"""
    state = _floor()
    points = ref.make_points([[0.03, 0.03, 0.03]], [0, 0, 1])
    lamps = ref.make_lamps([[0.05, 0.04, 0.03]])
    assert ref.exposure(state, [0, 0, 0], VS, points, lamps)[1][0] == 0
    assert ref.exposure(state, [0, 0, 0], VS, points, lamps, wrong="facing_ge")[1][0] == 1


def test_truncation_at_negative_indices_is_caught():
    """q = -2.6: floorf(q + 0.5f) is voxel -3, (int)q is voxel -2"""
    origin = [-8, -8, -8]
    state = np.full((8, 8, 8), FR, dtype=np.uint8)
    state[4, 4, 5] = OC                                                 # voxel (-3, -4, -4)
    points = ref.make_points([[-0.036, -0.04, -0.04]], [1, 0, 0])       # q = (-2.6, -4, -4): start voxel (-3, -4, -4)
    lamps = ref.make_lamps([[-0.01, -0.04, -0.04]])
    assert ref.exposure(state, origin, VS, points, lamps)[1][0] == 0    # it starts inside the blocker
    assert ref.exposure(state, origin, VS, points, lamps, wrong="truncate")[1][0] == 1
    # at positive indices the two agree on this point's mirror image only by luck of the fraction
    lamps = ref.make_lamps([[-0.036, -0.04, -0.04]])                    # the lamp's voxel: floorf(-3.6 + 0.5) = -4
    table = ref.exposure(state, origin, VS, points, lamps)[2]
    assert table["accepted"][0] == 1


def test_states_and_flags():
    state = np.full((4, 4, 12), FR, dtype=np.uint8)
    state[:, :, 4:8] = ref.UNKNOWN
    points = ref.make_points([[0.10, 0.01, 0.01]], [-1, 0, 0])
    lamps = ref.make_lamps([[0.01, 0.01, 0.01], [0.05, 0.01, 0.01]])
    assert ref.exposure(state, [0, 0, 0], VS, points, lamps)[1][0] == 3
    _, mask, table, _ = ref.exposure(state, [0, 0, 0], VS, points, lamps, unknown_occupied=True)
    assert mask[0] == 0 and table["accepted"].tolist() == [1, 0]
    assert ref.exposure(state, [0, 0, 0], VS, points, lamps, max_range=0.06)[1][0] == 2
