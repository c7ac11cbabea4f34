"""Crafted maps for the marching-cubes export (k_marching_cubes and the scans of ra-slam_amd/csrc/kernels_mesh.h, the host
sequence of query.inc), and a plain numpy reference of it, written once and run against the CPU oracle
(tests/test_mesh_cases.py, no GPU) and the HIP engine (tests/test_gpu_mesh.py).  Same role as raycast_cases.py: no GPU
and no torch at import (test_mesh.py, whose table loader, corner and edge lists and triangle rows are used here, imports
neither torch nor the engine library).

The maps are written voxel by voxel (import_blocks): both implementations hold the same floats, and every vertex
operation is one correctly rounded float32 operation, so the bar is EQUALITY of the triangle rows and of the exported
vertices -- engine, oracle and mesh_ref alike.

mesh_ref restates the rules of gather_valid_mesh (oracle/ratsdf_oracle.cpp) in another shape than the kernel and the
oracle have: no staged 16^3 tile, every value is fetched from the whole map by its global voxel coordinates, all cubes
of the map are walked at once, edge by edge.
"""
import functools
from pathlib import Path

import numpy as np

import raycast_cases as rc
from raycast_cases import BlockSet, F, Lookup, block_keys, block_voxels, concat, plane_patch, sphere_shell
from ratsdf._abi import RGBW_DTYPE
from test_mesh import CORNER, EDGE, _tri_rows, load_cases

ROOT = Path(__file__).resolve().parent.parent
VS, TRUNC = rc.VS, rc.TRUNC
MIN_WEIGHT = 10          # a voxel is observed when its weight is ABOVE this (the ray cast: at or above)
UNOBSERVED = F(-10)
VERTS_PER_BLOCK, TRIS_PER_BLOCK, SCAN_TILE, SCAN_PASS = 729 * 3, 512 * 5, 4096, 1024

tri_rows = _tri_rows


def vertex_rows(v, p):
    """the exported vertices as a sorted multiset of (x, y, z, probability) rows"""
    a = np.concatenate([np.asarray(v, F).reshape(-1, 3), np.asarray(p, F).reshape(-1, 1)], axis=1)
    return a[np.lexsort(a.T[::-1])]


def unreferenced(v, tri):
    """number of exported vertices that no triangle names"""
    return len(v) - len(np.unique(np.asarray(tri).reshape(-1)))


# ---------------------------------------------------------------------------------------------------------------------
# the reference
_CORNER = np.array(CORNER, dtype=np.int64)
_EDGE = np.array(EDGE, dtype=np.int64)
_EDGE_DIM = np.abs(_CORNER[_EDGE[:, 0]] - _CORNER[_EDGE[:, 1]]).argmax(axis=1)
# the end of the edge that lies at 0 along the edge's axis
_EDGE_LOWER = np.where(_CORNER[_EDGE[:, 0], _EDGE_DIM] == 0, _EDGE[:, 0], _EDGE[:, 1])
_UNIT = np.eye(3, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def case_table():
    """[256, 16] edge numbers per sign pattern, -1 after the last triangle (oracle/mc_cases.inc)"""
    cases = load_cases(ROOT / "oracle" / "mc_cases.inc")
    assert len(cases) == 256
    t = np.full((256, 16), -1, dtype=np.int64)
    for c, s in enumerate(cases):
        t[c, :len(s)] = [int(ch, 16) for ch in s]
    return t


def _wrap16(a):
    return ((np.asarray(a, dtype=np.int64) + 32768) & 0xFFFF) - 32768


class Field:
    """tsdf and probability of the whole map by global voxel coordinates (8 * block + local, not wrapped: the block of a
    voxel is its coordinates >> 3, as the neighbour lookup forms it); -10 and 0 where the block is absent or the voxel's
    weight is not above MIN_WEIGHT"""

    def __init__(self, m):
        self.look = Lookup(m)
        self.seen = m.rgbw["weight"].astype(np.int64) > MIN_WEIGHT
        self.t = np.where(self.seen, m.tsdf, UNOBSERVED).astype(F)
        self.p = np.where(self.seen, m.prob, F(0)).astype(F)

    def at(self, vox):
        """(tsdf, probability, observed) at voxels [..., 3]"""
        vox = np.asarray(vox, dtype=np.int64)
        r = self.look.rows(vox)
        i = (vox[..., 0] & 7) + (vox[..., 1] & 7) * 8 + (vox[..., 2] & 7) * 64
        ok = r >= 0
        rr = np.where(ok, r, 0)
        return (np.where(ok, self.t[rr, i], UNOBSERVED).astype(F), np.where(ok, self.p[rr, i], F(0)).astype(F),
                ok & self.seen[rr, i])


def _new_info():
    return dict(blocks=0, interior=np.zeros(256, np.int64), seam=np.zeros(256, np.int64), straddle=np.zeros(8, np.int64),
                dropped_at=np.zeros(3, np.int64), cull_small=0, cull_large_observed=0)


def mesh_ref(m, vs=VS, chunk=256):
    """Marching cubes over the block set `m`: (vertices [n, 3] float32, triangles [k, 3] int64, probabilities [n] float32,
    info).  Vertices are in the order of m's blocks, unreferenced ones included; compare through tri_rows / vertex_rows.
    info counts what the walk met: sign patterns among cubes whose eight corners are all observed (`interior`; `seam`:
    those of them that straddle a block face; `straddle[x + 2y + 4z]`: by the faces they straddle), triangles dropped
    at their first / second / third edge, and edges culled by either rule."""
    info = _new_info()
    info["blocks"] = len(m)
    if len(m) == 0:
        return np.zeros((0, 3), F), np.zeros((0, 3), np.int64), np.zeros(0, F), info
    field, table = Field(m), case_table()
    pos = np.asarray(m.pos, dtype=np.int64)
    vmask = np.zeros(len(m) * VERTS_PER_BLOCK, dtype=bool)
    kept = []
    local = block_voxels(np.zeros((1, 3), np.int64))[0]                       # [512, 3]
    for b0 in range(0, len(m), chunk):
        rows = np.arange(b0, min(b0 + chunk, len(m)))
        origin = pos[rows][:, None, :] * 8 + local[None]                       # [n, 512, 3] the cubes' corner 0
        lt, _, seen = field.at(origin[:, :, None, :] + _CORNER[None, None])   # [n, 512, 8]
        pattern = ((lt < 0).astype(np.int64) << np.arange(8)).sum(axis=-1)
        whole = seen.all(axis=-1)
        face = (local == 7).astype(np.int64) @ np.array([1, 2, 4])            # [512]
        face = np.broadcast_to(face, pattern.shape)
        info["interior"] += np.bincount(pattern[whole], minlength=256)
        info["seam"] += np.bincount(pattern[whole & (face > 0)], minlength=256)
        info["straddle"] += np.bincount(face[whole], minlength=8)
        cut = (pattern != 0) & (pattern != 255)                                # the cubes that hold triangles at all
        lt, pattern = lt[cut], pattern[cut]                                    # [k, 8], [k]
        corner0 = np.broadcast_to(local[None], cut.shape + (3,))[cut]          # [k, 3] in the block
        row = np.broadcast_to(rows[:, None], cut.shape)[cut]
        for i in range(5):
            alive = table[pattern, 3 * i] >= 0
            ids = np.zeros(pattern.shape + (3,), dtype=np.int64)
            for j in range(3):
                e = np.where(alive, table[pattern, 3 * i + j], 0)
                a, b = lt[np.arange(len(e)), _EDGE[e, 0]], lt[np.arange(len(e)), _EDGE[e, 1]]
                diff = np.abs((b - a).astype(F))
                small, large = diff.astype(np.float64) < 1e-3, diff >= F(2)
                drop = alive & (small | large)
                info["dropped_at"][j] += int(drop.sum())
                info["cull_small"] += int((alive & small).sum())
                info["cull_large_observed"] += int((alive & large & (a > UNOBSERVED) & (b > UNOBSERVED)).sum())
                alive = alive & ~drop
                at = corner0 + _CORNER[_EDGE_LOWER[e]]                          # [k, 3] in the block's 9^3 lattice
                ids[:, j] = (row * 729 + at[:, 2] * 81 + at[:, 1] * 9 + at[:, 0]) * 3 + _EDGE_DIM[e]
                vmask[ids[:, j][alive]] = True                                 # (set before the later edges are judged)
            kept.append(ids[alive])
    vid = np.flatnonzero(vmask)
    brow, lattice, dim = vid // VERTS_PER_BLOCK, vid // 3 % 729, vid % 3
    at = np.stack([lattice % 9, lattice // 9 % 9, lattice // 81], axis=1)
    t1, p1, _ = field.at(pos[brow] * 8 + at)
    t2, p2, _ = field.at(pos[brow] * 8 + at + _UNIT[dim])
    v1 = _wrap16(_wrap16(pos[brow] << 3) + at).astype(F)
    with np.errstate(all="ignore"):
        sfac = ((-t1) / (t2 - t1).astype(F)).astype(F)
        v = ((v1 + (sfac[:, None] * _UNIT[dim].astype(F)).astype(F)).astype(F) * F(vs)).astype(F)
        p = ((p1 + p2).astype(F) / F(2)).astype(F)
    tri = np.searchsorted(vid, np.concatenate(kept).reshape(-1, 3))
    return v, tri, p, info


# ---------------------------------------------------------------------------------------------------------------------
# builders
def replaced(m, **fields):
    """m with some arrays replaced (BlockSet's own __len__ stands in the way of NamedTuple._replace)"""
    return BlockSet(**{**dict(zip(BlockSet._fields, tuple(m))), **fields})


def _probability(v):
    """a function of the voxel's coordinates, exact in float32, whose pairwise means are exact too"""
    return ((((7 * v[..., 0] + 13 * v[..., 1] + 29 * v[..., 2]) & 63) + 0.5) / 64).astype(F)


def _colour(v, weight):
    rgbw = np.zeros(v.shape[:-1], dtype=RGBW_DTYPE)
    rgbw["r"], rgbw["g"], rgbw["b"] = (37 * v[..., 0]) & 255, (59 * v[..., 1]) & 255, (83 * v[..., 2]) & 255
    rgbw["weight"] = weight
    return rgbw


NOISE_OFFSET = (-7, -12, -5)           # block offset of the cube: negative, non-zero
NOISE_EXTENT = (4, 3, 3)               # 3x3x3 gives every pattern across a face too, some only once: a fourth layer on x
NOISE_SEED = 20250117
NOISE_WEIGHTS = ((0, 9, 10, 11, 40), (0.01, 0.01, 0.02, 0.26, 0.70))
NOISE_ABSENT = (3, 1, 1)               # the centre block of the +x face is left out
NOISE_UNDERWEIGHT = (1, 1, 2)          # the centre block of the +z face: present, every voxel at weight 10
_BELOW_1E3 = np.nextafter(F(1e-3), F(0))        # float32(1e-3) is above 1e-3 as a double, its predecessor below
_ONE = F(1)
NOISE_PAIRS = (
    # (first voxel relative to the cube's first voxel, axis, tsdf of the first, tsdf of the second): opposite signs
    ((8 + 2, 8 + 2, 8 + 2), 0, F(-2.0 ** -11), F(F(1e-3) - F(2.0 ** -11))),       # diff = float32(1e-3): kept
    ((8 + 2, 8 + 4, 8 + 2), 0, F(-2.0 ** -11), F(_BELOW_1E3 - F(2.0 ** -11))),    # diff just under 1e-3: culled
    ((8 + 2, 8 + 7, 8 + 5), 1, F(-2.0 ** -11), F(_BELOW_1E3 - F(2.0 ** -11))),    # the same across a block face
    ((8 + 4, 8 + 2, 8 + 2), 1, _ONE, -_ONE),                                      # diff = 2: culled
    ((8 + 4, 8 + 5, 8 + 2), 1, _ONE, np.nextafter(-_ONE, F(0))),                  # 2 - 2^-24 rounds to 2: culled
    ((8 + 6, 8 + 2, 8 + 2), 2, _ONE, np.nextafter(np.nextafter(-_ONE, F(0)), F(0))),   # 2 - 2^-23: kept
    ((8 + 6, 8 + 7, 8 + 4), 1, _ONE, -_ONE),                                      # diff = 2 across a block face
    ((8 + 2, 8 + 6, 8 + 6), 0, F(0.0), F(-0.5)),                                  # zero: `lt < 0` is false, sfac = 0
    ((8 + 4, 8 + 6, 8 + 6), 0, F(-0.0), F(-0.5)),                                 # negative zero: the same
    ((8 + 6, 8 + 4, 8 + 6), 2, F(-0.25), F(0.0)),                                 # zero at the far end: sfac = 1
    ((8 + 7, 8 + 7, 8 + 7), 1, F(-0.0), F(-0.75)),                                # negative zero in a block's last voxel
)


@functools.lru_cache(maxsize=None)
def noise_blocks():
    """4x3x3 blocks of noise (one left out, one under-weight) that reach every sign pattern, both thresholds of either
    rule and the zeros; asserts by mesh_ref alone that they do, and prints the counts"""
    off = np.array(NOISE_OFFSET, dtype=np.int64)
    idx = rc._cube((0, 0, 0), NOISE_EXTENT)
    idx = idx[~(idx == NOISE_ABSENT).all(axis=1)]
    pos = idx + off
    v = block_voxels(pos)
    rng = np.random.default_rng(NOISE_SEED)
    tsdf = rng.uniform(-1, 1, size=v.shape[:-1]).astype(F)
    weight = rng.choice(NOISE_WEIGHTS[0], p=NOISE_WEIGHTS[1], size=v.shape[:-1])
    weight[(idx == NOISE_UNDERWEIGHT).all(axis=1)] = MIN_WEIGHT
    look = Lookup(BlockSet(pos.astype(np.int16), tsdf, tsdf, tsdf))

    def put(vox, value):
        vox = np.asarray(vox, dtype=np.int64)
        r = int(look.rows(vox))
        assert r >= 0 and not (idx[r] == NOISE_UNDERWEIGHT).all()
        i = int((vox[0] & 7) + (vox[1] & 7) * 8 + (vox[2] & 7) * 64)
        tsdf[r, i], weight[r, i] = value, rc.WEIGHT

    for first, axis, t1, t2 in NOISE_PAIRS:
        first = off * 8 + np.array(first)
        put(first, t1)
        put(first + _UNIT[axis], t2)
    m = BlockSet(pos.astype(np.int16), tsdf, _colour(v, weight), _probability(v))
    _, tri, _, info = mesh_ref(m)
    print(f"mesh noise_blocks: {len(m)} blocks, {len(tri)} triangles; per sign pattern among whole cubes: "
          f"{info['interior'].min()} .. {info['interior'].max()} ({int((info['interior'] > 0).sum())} of 256), across a "
          f"block face {info['seam'].min()} .. {info['seam'].max()} ({int((info['seam'] > 0).sum())} of 256); by faces "
          f"straddled (x + 2y + 4z) {info['straddle'].tolist()}; triangles dropped at edge 1 / 2 / 3: "
          f"{info['dropped_at'].tolist()}; edges culled under 1e-3: {info['cull_small']}, at 2 or more between observed "
          f"voxels: {info['cull_large_observed']}")
    assert (info["interior"] > 0).all() and (info["seam"] >= 2).all()
    assert (info["straddle"][1:] >= 3).all()
    assert info["dropped_at"][1] > 0 and info["dropped_at"][2] > 0
    assert info["cull_small"] >= 2 and info["cull_large_observed"] >= 3
    w = m.rgbw["weight"]
    assert all((w == k).any() for k in NOISE_WEIGHTS[0]) and (w > MIN_WEIGHT).mean() > 0.85
    return m


# the centre is no lattice point and no half point on any axis.  With this pair no lattice edge that crosses the sphere
# is so nearly tangent that its ends differ by less than 1e-3 (such an edge is culled and opens a hole: (3.3, -5.4, 110.7)
# with 40.25 has six), no voxel lies on the sphere, mesh_ref's surface is closed and has no triangle of zero area
# (test_mesh_cases.py asserts all of it)
SPHERE_CENTRE, SPHERE_RADIUS = (3.21, -5.43, 110.69), 40.1
SPHERE_ZERO_AREA_CAP = 0


@functools.lru_cache(maxsize=None)
def sphere_mesh_map():
    m = sphere_shell(SPHERE_CENTRE, SPHERE_RADIUS)
    return replaced(m, prob=_probability(block_voxels(m.pos)))


def scan_tiles(nb):
    """(tiles of the vertex scan, tiles of the triangle scan) of a map of nb blocks"""
    return -(-nb * VERTS_PER_BLOCK // SCAN_TILE), -(-nb * TRIS_PER_BLOCK // SCAN_TILE)


# k_scan_tile_sums takes 1024 tiles of 4096 items per pass; a block has 2187 candidate vertices and 2560 candidate
# triangles.  A third pass needs more than 2048 tiles: more than 3835 blocks (vertices), 3276 (triangles).
#   3875 blocks: 3875 * 2187 = 2069 * 4096 + 1: 2070 vertex tiles, the last holds ONE item (2187^-1 = 3875 mod 4096: the
#                only such count below 7971); triangles 2422 tiles, the last holds 3584
#   3912 blocks: 3912 * 2560 = 2445 * 4096: 2445 triangle tiles, the last one full; vertices 2089 tiles, the last 3096
#   4101 blocks: generic: vertices 2190 tiles (the last holds 2743), triangles 2564 tiles (the last holds 512)
# (big_map() asserts these remainders and that every scan takes three passes)
BIG_COUNTS = (3875, 3912, 4101)
BIG_CENTRE, BIG_RADIUS = (2.6, 1.3, -3.8), 82.0


@functools.lru_cache(maxsize=None)
def big_map():
    """a sphere shell of a little over BIG_COUNTS[-1] blocks, x slowest: a prefix of it is a connected part of the shell"""
    m = sphere_shell(BIG_CENTRE, BIG_RADIUS)
    m = replaced(m, prob=_probability(block_voxels(m.pos)))
    assert len(m) >= BIG_COUNTS[-1], len(m)
    a, b, c = BIG_COUNTS
    assert a * VERTS_PER_BLOCK % SCAN_TILE == 1 and b * TRIS_PER_BLOCK % SCAN_TILE == 0
    assert c * TRIS_PER_BLOCK % SCAN_TILE > 1 and c * VERTS_PER_BLOCK % SCAN_TILE > 1
    assert all(min(scan_tiles(n)) > 2 * SCAN_PASS for n in BIG_COUNTS) and max(scan_tiles(c)) <= 3 * SCAN_PASS
    return m.take(np.arange(BIG_COUNTS[-1]))


def big_maps():
    """the three prefixes of big_map()"""
    m = big_map()
    return [m.take(np.arange(n)) for n in BIG_COUNTS]


EDGE_WRAP = (4096, 0, 0)               # the first block whose voxel coordinates no longer fit int16


@functools.lru_cache(maxsize=None)
def _edge_maps():
    out = {}
    for name, at in (("edge_hi", rc.EDGE_HI), ("edge_lo", rc.EDGE_LO)):
        m = rc.patch(at)
        out[name] = replaced(m, prob=_probability(block_voxels(m.pos)))
    assert out["edge_hi"].pos[:, 0].max() == 4095 and out["edge_lo"].pos[:, 0].min() == -4096
    # the same plane over blocks 4094 .. 4097 on x (plane_patch itself stops at 4095)
    n, c = rc._unit(rc.PLANE_NORMAL), rc.block_centre(EDGE_WRAP)
    pos = rc._cube((4094, -3, -3), (4098, 3, 3))
    pos = pos[np.abs((rc.block_centre(pos) - c) @ n) <= rc.KEEP_VOXELS]
    m = rc._from_distance(pos, (block_voxels(pos) - c) @ n)
    out["edge_wrap"] = replaced(m, prob=_probability(block_voxels(m.pos)))
    assert sorted(set(m.pos[:, 0].tolist())) == [4094, 4095, 4096, 4097]
    return out


def edge_maps():
    """{name: plane patch}: edge_hi and edge_lo reach the last blocks whose voxels have int16 coordinates, 4095 and
    -4096 on x (import_blocks takes any int16 block coordinate).  In them no exported vertex shows the int16 wrap of
    the vertex base: the lattice points at x = 32768 belong to cubes that reach into the absent block 4096, and all
    their triangles are dropped.  edge_wrap has blocks 4095 and 4096 side by side: there the vertices at x >= 32768
    are exported, wrapped to -32768 and up."""
    return dict(_edge_maps())


@functools.lru_cache(maxsize=None)
def single_block():
    """one block of the noise alone: all seven neighbours absent"""
    m = noise_blocks()
    return m.take(np.flatnonzero((m.pos == np.array(NOISE_OFFSET) + 1).all(axis=1)))


def empty():
    return BlockSet(np.zeros((0, 3), np.int16), np.zeros((0, 512), F), np.zeros((0, 512), RGBW_DTYPE),
                    np.zeros((0, 512), F))


EDIT_EXTRA = 50


def edited_maps():
    """(the sphere without its last EDIT_EXTRA blocks, those blocks): the `edited` sequence imports the first, deletes
    every third block, imports them back in reverse order and then the rest"""
    m = sphere_mesh_map()
    n = len(m) - EDIT_EXTRA
    return m.take(np.arange(n)), m.take(np.arange(n, len(m)))


CASES = ("noise", "sphere", "single_block", "empty", "edge_hi", "edge_lo", "edge_wrap")


def cases():
    """{name: BlockSet} of every crafted map but the three big ones"""
    out = dict(noise=noise_blocks(), sphere=sphere_mesh_map(), single_block=single_block(), empty=empty())
    out.update(edge_maps())
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """mesh_ref of a named case, or of the first n blocks of the big map (("big", n)), computed once"""
    if isinstance(name, tuple):
        return mesh_ref(big_map().take(np.arange(name[1])))
    return mesh_ref(cases()[name])


def present(m, directory_blocks):
    """the blocks of m that a directory (dump_directory()[1]) holds"""
    held = np.stack([directory_blocks["x"], directory_blocks["y"], directory_blocks["z"]], axis=1)
    return m.take(np.flatnonzero(np.isin(block_keys(m.pos), block_keys(held))))


# ---------------------------------------------------------------------------------------------------------------------
# what the tests assert (on the oracle's mesh without a GPU, on the engine's with one)
def assert_same_mesh(got, want, what):
    """equal triangle rows and equal exported vertices; got / want = (v, tri, p).  Prints the counts."""
    (gv, gt, gp), (wv, wt, wp) = got[:3], want[:3]
    print(f"mesh {what}: {len(gv)} vertices ({unreferenced(gv, gt)} unreferenced), {len(gt)} triangles; expected "
          f"{len(wv)} ({unreferenced(wv, wt)}), {len(wt)}")
    assert len(gp) == len(gv) and len(wp) == len(wv)
    if len(gt):
        assert gt.min() >= 0 and gt.max() < len(gv), what
    a, b = tri_rows(gv, gt, gp), tri_rows(wv, wt, wp)
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: triangles differ"
    a, b = vertex_rows(gv, gp), vertex_rows(wv, wp)
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: exported vertices differ"


def weld(v, tri):
    """(number of distinct vertex positions, triangles over them): block faces export the same position twice"""
    pts, inv = np.unique(np.asarray(v), axis=0, return_inverse=True)
    return len(pts), inv.reshape(-1)[np.asarray(tri)]


def assert_closed_sphere(v, tri, centre, radius, vs=VS, zero_area_cap=SPHERE_ZERO_AREA_CAP):
    """every edge in exactly two triangles, once in each direction; V - E + F = 2; every normal outward (tsdf > 0
    outside, the table's winding).  Triangles of zero area are left out, at most zero_area_cap of them."""
    x = np.asarray(v, dtype=np.float64) / vs
    a, b, c = (x[tri[:, k]] for k in range(3))
    normal = np.cross(b - a, c - a)
    flat = np.linalg.norm(normal, axis=1) == 0
    assert flat.sum() <= zero_area_cap, f"{int(flat.sum())} triangles of zero area"
    tri, normal, mid = tri[~flat], normal[~flat], ((a + b + c) / 3)[~flat]
    out = (normal * (mid - np.asarray(centre))).sum(axis=1)
    assert (out > 0).all() or (out < 0).all(), f"{int((out > 0).sum())} of {len(out)} normals point outward"
    _, w = weld(v, tri)
    assert (w[:, 0] != w[:, 1]).all() and (w[:, 1] != w[:, 2]).all() and (w[:, 0] != w[:, 2]).all()
    half = np.concatenate([w[:, [0, 1]], w[:, [1, 2]], w[:, [2, 0]]])
    assert len(np.unique(half, axis=0)) == len(half), "an edge is walked twice in the same direction"
    back = np.unique(half[:, ::-1], axis=0)
    assert np.array_equal(np.unique(half, axis=0), back), "an edge lacks its opposite"
    n_v, n_e, n_f = len(np.unique(w)), len(half) // 2, len(w)
    print(f"mesh sphere: V {n_v} - E {n_e} + F {n_f} = {n_v - n_e + n_f}; {int(flat.sum())} triangles of zero area")
    assert n_v - n_e + n_f == 2
    return n_v, n_e, n_f


def assert_on_sphere(v, centre, radius, vs=VS):
    """Linear interpolation of a 1-Lipschitz field whose curvature is at most 1 / (R - 1) errs over a unit edge by at
    most 1 / (8 (R - 1)); 1e-4 for the float32 rounding of the stored field.  Voxels."""
    d = np.abs(np.linalg.norm(np.asarray(v, dtype=np.float64) / vs - np.asarray(centre), axis=1) - radius)
    bound = 1 / (8 * (radius - 1)) + 1e-4
    print(f"mesh sphere: largest distance of a vertex from the sphere {d.max():.6f} voxels (bound {bound:.6f})")
    assert d.max() <= bound


def assert_vertex_probabilities(m, v, p, vs=VS):
    """every exported probability is the float32 mean of the probabilities of the two voxels its vertex lies between,
    found again from the vertex's coordinates.  A vertex ON a voxel (sfac 0 or 1) does not tell which edge it came
    from: for those this is a plausibility check only, the mean with ANY of the six neighbours passes; their exact
    values are held by the comparison with mesh_ref (assert_same_mesh)."""
    field = Field(m)
    x = np.asarray(v, dtype=np.float64) / vs
    near = np.round(x)
    off = np.abs(x - near) > 0.01
    assert (off.sum(axis=1) <= 1).all(), "a vertex lies off the lattice on more than one axis"
    on = ~off.any(axis=1)
    dim = off.argmax(axis=1)
    lo = near.astype(np.int64)
    rows = np.flatnonzero(~on)
    lo[rows, dim[rows]] = np.floor(x[rows, dim[rows]]).astype(np.int64)
    _, p1, s1 = field.at(lo[rows])
    _, p2, s2 = field.at(lo[rows] + _UNIT[dim[rows]])
    assert s1.all() and s2.all(), "a vertex lies next to an unobserved voxel"
    want = ((p1 + p2).astype(F) / F(2)).astype(F)
    assert np.array_equal(np.asarray(p)[rows], want), f"{int((np.asarray(p)[rows] != want).sum())} probabilities differ"
    for r in np.flatnonzero(on):
        _, p1, _ = field.at(lo[r])
        others = [field.at(lo[r] + s * _UNIT[d]) for d in range(3) for s in (1, -1)]
        assert any(seen and F(F(p1 + q) / F(2)) == p[r] for _, q, seen in others), f"vertex {r} at {lo[r]}"
    return len(rows), int(on.sum())


def owners(v, tri, vs=VS):
    """block position [k, 3] of the cube each triangle of non-zero area lies in (by its centroid)"""
    x = np.asarray(v, dtype=np.float64) / vs
    a, b, c = (x[tri[:, k]] for k in range(3))
    keep = np.linalg.norm(np.cross(b - a, c - a), axis=1) > 0
    return np.floor(((a + b + c) / 3)[keep]).astype(np.int64) >> 3
