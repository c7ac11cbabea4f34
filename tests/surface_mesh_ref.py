"""numpy restatement of the surface-mesh contract of include/ratsdf_surface_mesh.h (test infrastructure).

`surface_mesh(blocks, origin, dims, vs, min_weight)` takes the map as surface_ref's dict (blocks_of) and returns
(vertices as surface_ref.POINT records, triangles int32 [n, 3]) in the header's orders.  Written in another shape than
the kernel: ONE dense array over the box and the layer of voxels above it, no blocks and no staging; the cells' cases
and the edges they use are whole-array operations; a vertex's index is looked up in a dictionary from (owner, axis).
The vertex records are surface_ref's: every crossing whose owner lies in [origin, origin + dims] is a record of
surface_ref.surface_points over that range, and the vertices are picked from them.

`sphere_blocks(centre, radius, lo, hi)` is the sphere of mesh_cases.sphere_mesh_map's construction (raycast_cases'
distance field, colour and probability) over EVERY block of lo .. hi, every voxel observed."""
import numpy as np

import raycast_cases as rc
import surface_ref as sr
from mesh_cases import case_table
from test_mesh import CORNER, EDGE

POINT = sr.POINT
_CORNER = np.array(CORNER, dtype=np.int64)
_EDGE = np.array(EDGE, dtype=np.int64)
EDGE_DIM = np.abs(_CORNER[_EDGE[:, 0]] - _CORNER[_EDGE[:, 1]]).argmax(axis=1)
# the end of the edge that lies at 0 along the edge's axis
EDGE_LOWER = np.where(_CORNER[_EDGE[:, 0], EDGE_DIM] == 0, _EDGE[:, 0], _EDGE[:, 1])
_UNIT = np.eye(3, dtype=np.int64)


def _order(v, *minor):
    """the permutation that sorts voxels v [n, 3] by block z, y, x, then x + 8y + 64z in the block, then `minor`"""
    local = (v[:, 0] & 7) + 8 * (v[:, 1] & 7) + 64 * (v[:, 2] & 7)
    return np.lexsort(tuple(minor) + (local, v[:, 0] >> 3, v[:, 1] >> 3, v[:, 2] >> 3))


def surface_mesh(blocks, origin, dims, vs, min_weight=1):
    origin = np.array([int(v) for v in origin], dtype=np.int64)
    dims = np.array([int(v) for v in dims], dtype=np.int64)
    X, Y, Z = (int(v) for v in dims)
    table = case_table()
    # voxels origin .. origin + dims + 1: the corners of the box's cells and the upper ends of the edges they own
    t, obs, _, _ = sr._dense(blocks, origin, origin + dims + 1, int(min_weight))
    neg = t < 0

    def sh(a, off, n=(X, Y, Z)):                    # the array at v + off for v in [0, n) (off, n: x, y, z)
        return a[off[2]:off[2] + n[2], off[1]:off[1] + n[1], off[0]:off[0] + n[0]]

    complete = np.ones((Z, Y, X), dtype=bool)
    pattern = np.zeros((Z, Y, X), dtype=np.int64)
    for i, c in enumerate(_CORNER):
        complete &= sh(obs, c)
        pattern |= sh(neg, c).astype(np.int64) << i
    # the lattice edges that belong to a complete cell of the box
    used = np.zeros((3,) + t.shape, dtype=bool)
    for e in range(12):
        sh(used[EDGE_DIM[e]], _CORNER[EDGE_LOWER[e]])[...] |= complete
    # every crossing whose owner lies in [origin, origin + dims], in the header's order: surface_ref's records
    # (voxel 32768 does not exist: it owns nothing)
    n1 = np.minimum(dims + 1, 32768 - origin)
    # (the mesh has no min_prob: -inf drops nothing, where 0.0 would drop a vertex of negative probability)
    points = sr.surface_points(blocks, origin, n1, vs, min_weight, -np.inf)
    zero = np.zeros(3, dtype=np.int64)
    own, axis, vert = [], [], []
    for a in range(3):
        cross = sh(obs, zero, n1) & sh(obs, _UNIT[a], n1) & (sh(neg, zero, n1) != sh(neg, _UNIT[a], n1))
        z, y, x = np.nonzero(cross)
        own.append(np.stack([x, y, z], axis=1) + origin)
        axis.append(np.full(len(x), a))
        vert.append(sh(used[a], zero, n1)[cross])
    own, axis, vert = np.concatenate(own), np.concatenate(axis), np.concatenate(vert)
    order = _order(own, axis)
    own, axis, vert = own[order], axis[order], vert[order]
    assert len(points) == len(own)
    vertices = points[vert]
    index = {(int(w[0]), int(w[1]), int(w[2]), int(a)): i for i, (w, a) in enumerate(zip(own[vert], axis[vert]))}
    # triangles: the cells in the header's order, each its table row, in the table's own order
    z, y, x = np.nonzero(complete & (table[pattern, 0] >= 0))
    cells = np.stack([x, y, z], axis=1) + origin
    cells = cells[_order(cells)]
    tri = []
    for v in cells:
        row = table[pattern[v[2] - origin[2], v[1] - origin[1], v[0] - origin[0]]]
        for k in range(0, 15, 3):
            if row[k] < 0:
                break
            ids = []
            for e in row[k:k + 3]:
                w = v + _CORNER[EDGE_LOWER[e]]
                ids.append(index[(int(w[0]), int(w[1]), int(w[2]), int(EDGE_DIM[e]))])
            tri.append(ids)
    return vertices, np.array(tri, dtype=np.int32).reshape(-1, 3)


def sphere_blocks(centre, radius, lo, hi, weight=rc.WEIGHT):
    """import_blocks' arrays (a raycast_cases.BlockSet) of every block in lo .. hi (block coordinates, inclusive): the
    distance to a sphere, positive outside, truncated at six voxels as raycast_cases does; every voxel observed"""
    pos = rc._cube(lo, np.asarray(hi) + 1)
    m = rc._from_distance(pos, np.linalg.norm(rc.block_voxels(pos) - np.asarray(centre, dtype=np.float64), axis=2)
                          - radius)
    m.rgbw["weight"] = weight
    return m


# ---- properties of a mesh, asserted on the restatement without a GPU and on the engine's output with one ----------
def triangle_rows(vertices, tri):
    """the triangles as sorted rows of nine floats (position triples, rotated so that the smallest vertex leads: the
    winding is kept)"""
    p = vertices["pos"][np.asarray(tri)]                              # [n, 3, 3]
    if len(p) == 0:
        return np.zeros((0, 9), np.float32)
    _, rank = np.unique(p.reshape(-1, 3), axis=0, return_inverse=True)
    first = rank.reshape(-1, 3).argmin(axis=1)
    rot = (first[:, None] + np.arange(3)[None]) % 3
    rows = p[np.arange(len(p))[:, None], rot].reshape(len(p), 9)
    return rows[np.lexsort(rows.T[::-1])]


def assert_closed(tri, n_vertices, euler=2):
    """index topology: every directed edge once, its opposite present, every vertex referenced, V - E + F = euler"""
    tri = np.asarray(tri, dtype=np.int64)
    assert tri.min() >= 0 and tri.max() < n_vertices
    half = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    key = half[:, 0] * n_vertices + half[:, 1]
    assert len(np.unique(key)) == len(key), "an edge is walked twice in the same direction"
    assert np.array_equal(np.unique(key), np.unique(half[:, 1] * n_vertices + half[:, 0])), "an edge lacks its opposite"
    assert len(np.unique(tri)) == n_vertices, "a vertex is not referenced"
    v, e, f = n_vertices, len(half) // 2, len(tri)
    print(f"surface mesh: V {v} - E {e} + F {f} = {v - e + f}")
    assert v - e + f == euler


def assert_oriented(vertices, tri, centre, vs):
    """every triangle of non-zero area faces free space: along its vertices' normals and away from the centre"""
    p = vertices["pos"][np.asarray(tri)].astype(np.float64)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    area = np.linalg.norm(n, axis=1) > 0
    normals = vertices["normal"][np.asarray(tri)].astype(np.float64).sum(axis=1)
    out = p.mean(axis=1) - np.asarray(centre, dtype=np.float64) * vs
    print(f"surface mesh: {int(area.sum())} of {len(tri)} triangles have an area")
    assert area.sum() > 0
    assert ((n * normals).sum(axis=1)[area] > 0).all(), "a triangle faces against its vertex normals"
    assert ((n * out).sum(axis=1)[area] > 0).all(), "a triangle faces the centre"


def assert_subsequence(part, whole):
    """the records of `part` appear in `whole`, byte for byte and in order"""
    a = [r.tobytes() for r in np.ascontiguousarray(part)]
    b = [r.tobytes() for r in np.ascontiguousarray(whole)]
    j = 0
    for i, r in enumerate(a):
        while j < len(b) and b[j] != r:
            j += 1
        assert j < len(b), f"record {i} of {len(a)} is not in the rest of the surface points"
        j += 1
