"""The numpy restatement of the clustered-mesh contract (tests/cluster_mesh_ref.py, include/ratsdf_cluster_mesh.h)
against answers worked out by hand, against properties that need no engine, and against the mistakes a kernel could
make: each wrong variant differs from the restatement on a named case."""
import functools

import numpy as np
import pytest

import cluster_mesh_ref as cref
import surface_cases as sc
import surface_mesh_ref as mref
import surface_ref as ref

F = np.float32
VS = 0.02
FACTORS = cref.FACTORS
# the sphere of the GPU test: centre near the corner of block 0 / -1 on x and y, negative coordinates included
CENTRE, RADIUS = (-0.4, -0.3, 3.6), 9.6
LO, HI = (-2, -2, -1), (1, 1, 1)                  # blocks: voxels -16 .. 15, -16 .. 15, -8 .. 15
ORIGIN, DIMS = [-13, -12, -8], [26, 26, 24]       # contains the sphere with a margin


@functools.lru_cache(maxsize=None)
def sphere():
    return ref.blocks_of(*mref.sphere_blocks(CENTRE, RADIUS, LO, HI))


@functools.lru_cache(maxsize=None)
def sphere_welded():
    return cref.welded(sphere(), ORIGIN, DIMS, VS)


@functools.lru_cache(maxsize=None)
def sphere_mesh(k, variant=cref.CONTRACT):
    return cref.cluster_mesh(sphere(), ORIGIN, DIMS, VS, k, variant=variant, mesh=sphere_welded())


# ---- 1. hand-computed answers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", FACTORS)
@pytest.mark.parametrize("f", [0.25, 0.75])
def test_plane_between_two_layers(k, f):
    """tsdf 1 - f... below and above: t0 = f, t1 = f - 1 across the layers z0, z0 + 1 gives f = t0 / (t0 - t1) exactly
    (0.25 and 0.75 are exact, and so is every sum of the tree: powers of two times one value).  The members are the z
    edges of the box's columns, k^2 per cluster; with f >= 0.5 they belong to the cluster layer of z0 + 1."""
    cx, cy, z0 = 3, 2, 11                                        # z0 + 1 = 12 starts a cluster layer for every k
    arrays = ref.solid((-1, 0, 0), (1, 1, 2), lambda x, y, z: np.where(z <= z0, F(f), F(f - 1)))
    blocks = ref.blocks_of(*arrays)
    origin, dims = [-8, 0, 6], [cx * k - 1, cy * k - 1, 10]       # the owners: whole clusters in x and y
    v, tri = cref.cluster_mesh(blocks, origin, dims, VS, k)
    assert len(v) == cx * cy and len(tri) == 2 * (cx - 1) * (cy - 1)
    layer = ((z0 + 1) if f >= 0.5 else z0) >> {2: 1, 4: 2, 8: 3}[k]
    want = []
    for y in range(cy):
        for x in range(cx):
            base = np.array([origin[0] + x * k, origin[1] + y * k, layer * k])
            want.append([float(c) for c in ((F(base[0]) + F((k - 1) / 2)) * F(VS),
                                            (F(base[1]) + F((k - 1) / 2)) * F(VS), F(z0 + f) * F(VS))])
    assert sorted(v["pos"].tolist()) == sorted(want), (k, f)      # (the order is the invariants' business)
    assert (v["normal"] == np.array([0, 0, -1], dtype=F)).all()   # the tsdf falls with z: free space is below
    assert (v["prob"] == F(0.5)).all() and (v["rgbw"]["weight"] == 3).all()
    p = v["pos"][tri].astype(np.float64)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (n[:, 2] < 0).all() and (n[:, :2] == 0).all()          # the winding faces free space


def test_rounded_mean_of_the_colour():
    """colour from the voxel index (ref.solid): the members of a cluster are the voxels of one layer, so r is the
    rounded mean of base .. base + k - 1, k times each: (2 * sum + n) / (2 * n) rounds the half up"""
    arrays = ref.solid((0, 0, 0), (1, 1, 1), lambda x, y, z: np.where(z <= 3, F(0.25), F(-0.75)))
    v, _ = cref.cluster_mesh(ref.blocks_of(*arrays), [0, 0, 0], [15, 15, 8], VS, 4)
    assert len(v) == 16
    r = v["rgbw"]["r"].tolist()                                   # means 1.5, 5.5, ...: rounded up
    assert sorted(set(r)) == [2, 6, 10, 14] and all(r.count(c) == 4 for c in (2, 6, 10, 14))
    assert v["rgbw"]["b"].tolist() == [3] * 16


# ---- 2. invariants on a sphere -------------------------------------------------------------------------------------
def test_sphere_lies_inside_the_box():
    c, o, d = np.array(CENTRE), np.array(ORIGIN), np.array(DIMS)
    assert (c - RADIUS - 1 > o).all() and (c + RADIUS + 1 < o + d - 1).all()
    assert (o < 0).all()


def check_invariants(v, tri, welded, k, centre=None):
    """the header's statements about the output, on any (vertices, triangles) of the box of `welded`"""
    s = {2: 1, 4: 2, 8: 3}[k]
    m = 8 >> s
    tri = np.asarray(tri, dtype=np.int64)
    assert tri.min() >= 0 and tri.max() < len(v)                                      # indices valid
    assert ((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])).all()
    assert (tri[:, 0] < tri[:, 1]).all() and (tri[:, 0] < tri[:, 2]).all()            # the first index is the smallest
    assert len({tuple(r) for r in tri}) == len(tri)                                   # no duplicate triple
    # the clusters with members, in the header's order
    up = welded.f >= F(0.5)
    q = (welded.owner + np.where(up[:, None], np.eye(3, dtype=np.int64)[welded.axis], 0)) >> s
    keys = sorted({tuple(int(c) for c in r) for r in q},
                  key=lambda c: (c[2] >> (3 - s), c[1] >> (3 - s), c[0] >> (3 - s),
                                 (c[0] & (m - 1)) + m * (c[1] & (m - 1)) + m * m * (c[2] & (m - 1))))
    assert len(v) == len(keys)
    base = np.array(keys, dtype=np.int64) << s
    lo, hi = (base - 0.5) * VS, (base + k - 0.5) * VS
    pos = v["pos"].astype(np.float64)
    assert ((pos >= lo) & (pos <= hi)).all()                                          # inside the cluster's extent
    # the order: first index, then the codes of the second and the third cluster relative to the first
    qa = np.array(keys, dtype=np.int64)
    d2, d3 = qa[tri[:, 1]] - qa[tri[:, 0]], qa[tri[:, 2]] - qa[tri[:, 0]]
    assert np.abs(d2).max() <= 1 and np.abs(d3).max() <= 1
    code = lambda d: (d[:, 0] + 1) + 3 * (d[:, 1] + 1) + 9 * (d[:, 2] + 1)
    key = (tri[:, 0] * 27 + code(d2)) * 27 + code(d3)
    assert (np.diff(key) > 0).all()
    if centre is not None:                                                            # faces away from the centre
        p = pos[tri]
        n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        area = np.linalg.norm(n, axis=1) > 0
        out = p.mean(axis=1) - np.asarray(centre, dtype=np.float64) * VS
        assert area.sum() > 0 and ((n * out).sum(axis=1)[area] > 0).all()


@pytest.mark.parametrize("k", FACTORS)
def test_sphere_invariants(k):
    v, tri = sphere_mesh(k)
    w = sphere_welded()
    print(f"k {k}: {len(w.vertices)} -> {len(v)} vertices, {len(w.triangles)} -> {len(tri)} triangles")
    assert 0 < len(v) < len(w.vertices) and 0 < len(tri) < len(w.triangles)
    check_invariants(v, tri, w, k, CENTRE)


# ---- 3. the wrong variants -------------------------------------------------------------------------------------------
def _case(name, k, variant=cref.CONTRACT):
    c = sc.case(name)
    return cref.cluster_mesh(sc.blocks_of(c), c.origin, c.dims, sc.VS, k, variant=variant, mesh=_case_welded(name))


@functools.lru_cache(maxsize=None)
def _case_welded(name):
    c = sc.case(name)
    return cref.welded(sc.blocks_of(c), c.origin, c.dims, sc.VS)


def _vertices_differ(a, b):
    return len(a) != len(b) or not ref.same_bytes(a, b)


@pytest.mark.parametrize("name", ["ladder_small", "ladder_large"])
def test_a_sequential_sum_is_caught(name):
    want = _case(name, 4)[0]
    got = _case(name, 4, cref.Variant(sequential=True))[0]
    assert len(got) == len(want) and cref.differing(got, want) > 0


def test_the_tie_rule_is_caught():
    want, got = _case("quotients", 2), _case("quotients", 2, cref.Variant(tie_gt=True))
    assert _vertices_differ(got[0], want[0]) or not np.array_equal(got[1], want[1])


def test_sorting_a_triple_is_caught():
    want, got = sphere_mesh(4)[1], sphere_mesh(4, cref.Variant(sort_triple=True))[1]
    assert want.shape != got.shape or not np.array_equal(want, got)
    flipped = {tuple(r) for r in got} - {tuple(r) for r in want}
    assert len(flipped) > 0                                      # triangles whose winding was lost


NOISE_LO, NOISE_HI, NOISE_BOX = (-1, -1, 0), (0, 0, 1), ([-8, -8, 0], [16, 16, 16])


def noise_arrays():
    """uniform noise over 2 x 2 x 2 blocks: a smooth sphere never maps two triangles to one triple, noise does"""
    rng = np.random.default_rng(11)
    return ref.solid(NOISE_LO, NOISE_HI, lambda x, y, z: rng.uniform(-1, 1, x.shape))


@pytest.mark.parametrize("k", FACTORS)
def test_missing_duplicate_removal_is_caught(k):
    blocks = ref.blocks_of(*noise_arrays())
    removed = cref.duplicates_removed(blocks, *NOISE_BOX, VS, k)
    print(f"duplicates removed on the noise map at k = {k}: {removed}")
    assert removed > 0
    w = cref.welded(blocks, *NOISE_BOX, VS)
    v, tri = cref.cluster_mesh(blocks, *NOISE_BOX, VS, k, mesh=w)
    check_invariants(v, tri, w, k)


def test_summing_world_positions_is_caught():
    want, got = sphere_mesh(4)[0], sphere_mesh(4, cref.Variant(world_pos=True))[0]
    assert len(got) == len(want) and cref.differing(got, want) > 0
    assert np.abs(got["pos"].astype(np.float64) - want["pos"]).max() < 1e-6     # the same points, rounded elsewhere


def test_a_truncating_shift_is_caught():
    want, got = sphere_mesh(4), sphere_mesh(4, cref.Variant(truncating_shift=True))
    assert len(got[0]) != len(want[0]) or _vertices_differ(got[0], want[0])


# ---- 4. the awkward values: what the GPU test relies on --------------------------------------------------------------
@pytest.mark.parametrize("name", sc.CASES)
@pytest.mark.parametrize("k", [2, 4])
def test_nan_counts_of_the_awkward_sets(name, k):
    """the GPU test compares a NaN of the restatement as "is NaN" only: no set but the two that plant NaN words
    (nonfinite: tsdf; probabilities: prob) has one, so the exemption cannot hide a failure elsewhere"""
    v, tri = _case(name, k)
    assert len(v) > 0 and (len(tri) > 0 or name == "quotients")  # (quotients: lone pairs, no cell spans 3 clusters)
    nans = cref.nan_count(v)
    print(f"{name} k {k}: {len(v)} vertices, {len(tri)} triangles, {nans} NaN words")
    assert (nans > 0) == (name in ("nonfinite", "probabilities"))
