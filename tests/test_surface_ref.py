"""The numpy restatement of the surface-point contract (tests/surface_ref.py) on its own: shapes whose surface is known
in closed form, and the tiling property of the edge ownership rule."""
import numpy as np

import surface_ref as ref

VS = np.float32(0.02)


def _sorted_rows(rec):
    rows = np.ascontiguousarray(rec).view(np.uint8).reshape(len(rec), -1)
    return rows[np.lexsort(rows.T)]


def test_plane_points_lie_on_the_plane_and_face_along_the_axis():
    for axis in range(3):
        # tsdf linear in one axis, zero at 11.25 voxels: positive (free) above
        blocks = ref.blocks_of(*ref.solid((0, 0, 0), (2, 2, 2), lambda *g: (g[axis] - 11.25) / 8.0))
        rec = ref.surface_points(blocks, [0, 0, 0], [24, 24, 24], VS)
        assert len(rec) == 24 * 24
        want = np.float32(np.float32(11) + np.float32(0.25)) * VS
        assert np.all(rec["pos"][:, axis] == want)
        n = np.zeros(3, dtype=np.float32)
        n[axis] = 1
        assert np.all(rec["normal"] == n)
        others = [b for b in range(3) if b != axis]
        got = set(map(tuple, np.rint(rec["pos"][:, others] / VS).astype(int)))
        assert got == {(i, j) for i in range(24) for j in range(24)}
        assert np.all(rec["prob"] == np.float32(0.5)) and np.all(rec["rgbw"]["weight"] == 3)
        # f = 0.25: the lower endpoint (index 11 along the axis) is the chosen one
        assert np.all(rec["rgbw"]["rgb"[axis]] == 11)
        # the flipped field faces the other way
        flipped = ref.blocks_of(*ref.solid((0, 0, 0), (2, 2, 2), lambda *g: (11.25 - g[axis]) / 8.0))
        back = ref.surface_points(flipped, [0, 0, 0], [24, 24, 24], VS)
        assert np.all(back["normal"] == -n) and np.all(back["pos"] == rec["pos"])


def test_sphere_points_lie_within_a_voxel_of_the_sphere_and_face_outwards():
    c, r = np.array([11.3, 12.1, 10.7]), 6.4
    dist = lambda x, y, z: np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    blocks = ref.blocks_of(*ref.solid((0, 0, 0), (2, 2, 2), lambda x, y, z: np.clip((dist(x, y, z) - r) / 4.0, -1, 1)))
    rec = ref.surface_points(blocks, [0, 0, 0], [24, 24, 24], VS)
    assert len(rec) > 300
    p = rec["pos"].astype(np.float64) / float(VS)
    radial = p - c
    d = np.linalg.norm(radial, axis=1)
    # both endpoints of a crossing edge lie within one voxel of the surface, and so does every point between them
    assert np.all(np.abs(d - r) <= 1.0)
    assert np.all(np.abs(np.linalg.norm(rec["normal"].astype(np.float64), axis=1) - 1) < 1e-6)
    assert np.all((rec["normal"] * radial).sum(1) > 0)


def test_adjacent_boxes_tile_without_duplicates_or_gaps():
    rng = np.random.default_rng(5)
    pos, tsdf, rgbw, prob = ref.solid((-1, -1, -1), (1, 1, 0), lambda x, y, z: rng.uniform(-1, 1, x.shape))
    rgbw["weight"] = rng.integers(0, 4, tsdf.shape)
    blocks = ref.blocks_of(pos, tsdf, rgbw, prob)
    whole = ref.surface_points(blocks, [-7, -6, -5], [20, 17, 11], VS)
    assert len(whole) > 1000
    for axis, cut in ((0, 4), (1, 2), (2, 0), (0, 0)):
        o1, d1 = [-7, -6, -5], [20, 17, 11]
        o2, d2 = list(o1), list(d1)
        d1[axis] = cut - o1[axis]
        o2[axis], d2[axis] = cut, d2[axis] - d1[axis]
        a, b = ref.surface_points(blocks, o1, d1, VS), ref.surface_points(blocks, o2, d2, VS)
        both = _sorted_rows(np.concatenate([a, b]))
        assert len(np.unique(both, axis=0)) == len(both)             # no duplicates
        assert np.array_equal(both, _sorted_rows(whole))             # no gaps


def test_order_and_filters():
    pos, tsdf, rgbw, prob = ref.solid((0, 0, 0), (1, 1, 1), lambda x, y, z: np.where((x + y + z) % 2 == 0, 0.5, -0.5))
    blocks = ref.blocks_of(pos, tsdf, rgbw, prob)
    rec = ref.surface_points(blocks, [0, 0, 0], [16, 16, 16], VS)
    assert len(rec) == 3 * 16 * 16 * 15                              # every edge between two voxels crosses
    v = np.floor(rec["pos"] / VS + np.float32(1e-3)).astype(int)
    key = [tuple(r) for r in np.stack([v[:, 2] >> 3, v[:, 1] >> 3, v[:, 0] >> 3,
                                       (v[:, 0] & 7) + 8 * (v[:, 1] & 7) + 64 * (v[:, 2] & 7)], 1)]
    assert key == sorted(key)
    assert len(ref.surface_points(blocks, [0, 0, 0], [16, 16, 16], VS, min_weight=4)) == 0
    assert len(ref.surface_points(blocks, [0, 0, 0], [16, 16, 16], VS, min_weight=3, min_prob=0.5)) == len(rec)
    assert len(ref.surface_points(blocks, [0, 0, 0], [16, 16, 16], VS, min_prob=0.5000001)) == 0
