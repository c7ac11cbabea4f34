"""The numpy restatement of the surface-mesh contract (tests/surface_mesh_ref.py) against properties that need no
engine: its vertices are surface points, a sphere comes out closed and oriented, boxes tile, and an unobserved voxel
takes out exactly the cells that touch it."""
import numpy as np
import pytest

import surface_mesh_ref as mref
import surface_ref as ref

VS = 0.02
CENTRE, RADIUS = (3.21, -5.43, 14.69), 9.1       # off the lattice: no voxel lies on the sphere
LO, HI = (-2, -3, 0), (2, 1, 3)                  # blocks: voxels -16 .. 23, -24 .. 15, 0 .. 31
ORIGIN, DIMS = [-9, -18, 2], [25, 26, 25]        # contains the sphere with a margin, not block aligned
SPLIT = [3, -6, 13]                              # not block aligned either


@pytest.fixture(scope="module")
def sphere():
    m = mref.sphere_blocks(CENTRE, RADIUS, LO, HI)
    return m, ref.blocks_of(*m)


@pytest.fixture(scope="module")
def whole(sphere):
    return mref.surface_mesh(sphere[1], ORIGIN, DIMS, VS)


def test_sphere_lies_inside_the_box_and_off_the_lattice(sphere):
    m, _ = sphere
    c, o, d = np.array(CENTRE), np.array(ORIGIN), np.array(DIMS)
    assert (c - RADIUS - 1 > o).all() and (c + RADIUS + 1 < o + d - 1).all()
    assert (m.rgbw["weight"] > 0).all() and (m.tsdf != 0).all()


def test_vertices_are_a_subsequence_of_the_surface_points(sphere, whole):
    v, tri = whole
    points = ref.surface_points(sphere[1], ORIGIN, np.array(DIMS) + 1, VS, min_prob=0)
    assert 0 < len(v) <= len(points) and v.dtype == ref.POINT
    mref.assert_subsequence(v, points)
    # a box that cuts the sphere: crossings between two cells outside it are surface points and no vertices
    cut = mref.surface_mesh(sphere[1], ORIGIN, [8, 26, 25], VS)[0]
    points = ref.surface_points(sphere[1], ORIGIN, [9, 27, 26], VS, min_prob=0)
    assert 0 < len(cut) < len(points)
    mref.assert_subsequence(cut, points)


def test_closed_sphere(whole):
    v, tri = whole
    assert len(tri) > 1000 and tri.dtype == np.int32 and tri.shape[1] == 3
    mref.assert_closed(tri, len(v))


def test_orientation(whole):
    mref.assert_oriented(*whole, CENTRE, VS)


def test_tiling(sphere, whole):
    rows = []
    o, d, s = np.array(ORIGIN), np.array(DIMS), np.array(SPLIT)
    for k in range(8):
        up = np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1], dtype=bool)
        lo = np.where(up, s, o)
        n = np.where(up, o + d - s, s - o)
        v, tri = mref.surface_mesh(sphere[1], lo, n, VS)
        assert len(tri) > 0 and len(np.unique(tri)) == len(v)
        rows.append(mref.triangle_rows(v, tri))
    rows = np.concatenate(rows)
    rows = rows[np.lexsort(rows.T[::-1])]
    want = mref.triangle_rows(*whole)
    assert rows.shape == want.shape and np.array_equal(rows, want)


def test_unobserved_hole(sphere, whole):
    m, _ = sphere
    # a voxel next to the surface, inside the shell of crossings
    c = np.array(CENTRE)
    hole = np.round(c + np.array([0.0, 0.0, RADIUS])).astype(np.int64)
    pos, t, rgbw, p = (a.copy() for a in m)
    i = int(np.flatnonzero((pos.astype(np.int64) == hole >> 3).all(axis=1))[0])
    rgbw["weight"][i, int((hole[0] & 7) + 8 * (hole[1] & 7) + 64 * (hole[2] & 7))] = 0
    v, tri = mref.surface_mesh(ref.blocks_of(pos, t, rgbw, p), ORIGIN, DIMS, VS)
    assert len(np.unique(tri)) == len(v)                      # no vertex is left unreferenced
    # the triangles that vanish are exactly those of the eight cells touching the voxel
    full, holed = mref.triangle_rows(*whole), mref.triangle_rows(v, tri)
    gone = np.array(sorted(set(map(bytes, full)) - set(map(bytes, holed))))
    assert len(set(map(bytes, holed)) - set(map(bytes, full))) == 0
    assert len(full) - len(holed) == len(gone) > 0
    vw, tw = whole
    cell = np.floor(vw["pos"][tw].astype(np.float64).mean(axis=1) / VS).astype(np.int64)   # the cell of each triangle
    touching = ((cell >= hole - 1) & (cell <= hole)).all(axis=1)
    assert touching.sum() == len(gone)
    assert len({tuple(r) for r in cell[touching]}) >= 2
    kept = mref.triangle_rows(vw, tw[~touching])
    assert np.array_equal(kept, holed)
