"""Crafted maps and labelled triangle meshes for the label score against a mesh (include/ratsdf_score_mesh.h), and the
wrong variants each must catch.  Same role as score_cases.py: no GPU and no torch at import; what is expected comes
from the BlockSet a map was written from and tests/score_mesh_ref.py, never from an engine (an engine's directory dump
only says in which order the blocks are gathered).  tests/test_score_mesh_cases.py evaluates the variants without a
GPU, tests/test_gpu_score_mesh.py runs every case on the engine.

Maps are a handful of blocks.  Where exact ties and exact distances are wanted the voxel size is 1 / 64, so that every
voxel coordinate and every difference to the crafted vertices is exact in float32; the other cases use query_cases'
0.02.
"""
import functools
from typing import NamedTuple

import numpy as np

import query_cases as qc
import score_cases as sc
import score_mesh_ref as mr
from raycast_cases import BlockSet
from score_cases import SMALL, VS, VS64, around, craft, nxt, sparse_tsdf
from score_mesh_ref import HIGH, IGNORE, LOW

F = np.float32
D = np.float64
MAX_REFS = 1 << 25          # RATSDF_LABELMESH_MAX_REFS of the header
MAX_CELLS = 1 << 24
CHUNK = 256                 # kMeshChunk of kernels_score_mesh.h: triangle records per LDS chunk


class Case(NamedTuple):
    name: str
    blocks: BlockSet
    engine: dict             # table sizes of the engine the map is loaded into
    vs: float
    vertices: np.ndarray     # [v, 3] float32
    labels: np.ndarray       # [v] uint8
    triangles: np.ndarray    # [t, 3] int32
    cell: float              # what label_mesh() is given (0: 8 voxel sizes)
    params: dict             # tsdf_below, max_dist, p_cutoff, min_weight
    wrong: tuple = ()        # names of WRONG variants (variant()) this case must tell from the contract
    grid_cell: float = 0.0   # the cell of score_mesh_ref.grid_nearest (0: 8 voxel sizes)


PARAMS = dict(tsdf_below=0.1, max_dist=0.3, p_cutoff=0.5, min_weight=0)


def _p(**kw):
    return {**PARAMS, **kw}


def small_tris(points, labels, size=0.01, rng=None):
    """one small triangle per point: (p, p + (size, 0, 0), p + (0, size, 0)), or with rng two random offsets of that
    length; the three vertices carry the point's label"""
    p = np.asarray(points, dtype=D).reshape(-1, 3)
    n = len(p)
    if rng is None:
        o1, o2 = np.tile([size, 0, 0], (n, 1)), np.tile([0, size, 0], (n, 1))
    else:
        o1, o2 = rng.uniform(-size, size, size=(n, 3)), rng.uniform(-size, size, size=(n, 3))
    v = np.stack([p, p + o1, p + o2], axis=1).reshape(-1, 3).astype(F)
    return v, np.repeat(np.asarray(labels, dtype=np.uint8), 3), np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def join(*meshes):
    """meshes (vertices, labels, triangles) put behind one another"""
    vs_, ls, ts, base = [], [], [], 0
    for v, l, t in meshes:
        v = np.asarray(v, dtype=F).reshape(-1, 3)
        vs_.append(v), ls.append(np.asarray(l, dtype=np.uint8).reshape(-1))
        ts.append(np.asarray(t, dtype=np.int64).reshape(-1, 3) + base)
        base += len(v)
    return np.concatenate(vs_), np.concatenate(ls), np.concatenate(ts).astype(np.int32)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261021)
    out = []

    def add(name, blocks, engine, vs, mesh, cell=0.0, params=None, wrong=(), grid_cell=0.0):
        v, l, t = mesh
        v = np.ascontiguousarray(v, dtype=F).reshape(-1, 3)
        l = np.ascontiguousarray(l, dtype=np.uint8).reshape(-1)
        t = np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)
        assert len(v) == len(l) and (len(t) == 0 or (t.min() >= 0 and t.max() < len(v)))
        out.append(Case(name, blocks, engine, vs, v, l, t, cell, params or _p(), tuple(wrong), grid_cell))

    # ---- the distance -----------------------------------------------------------------------------------------------
    # one large triangle in the plane z = 0, legs of one block edge; the nine blocks around it hold voxels in each of
    # the seven regions (the face, three edges, three vertices) and on the borders between them, up to 7 voxels above
    nine = [(x, y, 0) for x in (-1, 0, 1) for y in (-1, 0, 1)]
    tri = ([(0, 0, 0), (0.125, 0, 0), (0, 0.125, 0)], [HIGH, HIGH, HIGH], [(0, 1, 2)])
    add("voronoi", craft(nine, tsdf=F(0.03125), weight=1), SMALL, VS64, tri, params=_p(max_dist=0.25),
        wrong=("nearest_vertex", "plane_distance", "box_distance"))
    # two triangles sharing the edge on the x axis, voxels of the plane y = 0 equidistant from both; exact duplicates of
    # both over vertices of their own with other labels; a far triangle holds index 0
    quad = craft([(0, 0, 0), (-1, -1, -1), (-1, 0, 0), (0, -1, 0)], tsdf=F(0.03125), weight=1)
    v = [(0.5, 0.5, 0.5), (0.625, 0.5, 0.5), (0.5, 0.625, 0.5),            # far
         (0, 0, 0), (0.125, 0, 0), (0, 0.125, 0), (0, -0.125, 0),          # the pair: (3, 4, 5) and (3, 4, 6)
         (0, 0, 0), (0.125, 0, 0), (0, 0.125, 0), (0, -0.125, 0)]          # their duplicates
    add("ties", quad, SMALL, VS64, (v, [IGNORE] * 3 + [LOW] * 4 + [HIGH] * 4,
                                    [(0, 1, 2), (3, 4, 5), (3, 4, 6), (7, 8, 9), (7, 8, 10)]),
        params=_p(max_dist=0.25), wrong=("ties_highest",))
    # a triangle whose three vertices carry the three labels, voxels nearest to each; a second, uniform one elsewhere
    v = [(0, 0, 0), (0.125, 0, 0), (0, 0.125, 0), (0.5, 0.5, 0.5), (0.625, 0.5, 0.5), (0.5, 0.625, 0.5)]
    add("mixed_labels", craft(nine, tsdf=F(0.03125), weight=1), SMALL, VS64,
        (v, [HIGH, LOW, IGNORE, LOW, LOW, LOW], [(0, 1, 2), (3, 4, 5)]), params=_p(max_dist=0.25),
        wrong=("label_of_nearest_vertex", "label_of_last_vertex"))
    # a wall of two large low-touch triangles in the plane z = 0 and a small high-touch handle 5 cm in front of its
    # middle: the voxels on the wall are nearer to a vertex of the handle than to any vertex of the wall
    wall = ([(-0.32, -0.32, 0), (0.48, -0.32, 0), (0.48, 0.48, 0), (-0.32, 0.48, 0)], [LOW] * 4, [(0, 1, 2), (0, 2, 3)])
    handle = ([(0.06, 0.06, 0.05), (0.10, 0.06, 0.05), (0.06, 0.10, 0.05), (0.10, 0.10, 0.05)], [HIGH] * 4,
              [(0, 1, 2), (1, 3, 2)])
    add("mesh_against_points", craft([(0, 0, 0), (1, 0, 0)], tsdf=F(0.05), weight=1), SMALL, VS, join(wall, handle),
        params=_p(max_dist=0.3))
    # dist2 == max_dist^2 exactly (voxel (0, 0, 0) and the vertex at -0.25: matched), and one float32 step beyond (voxel
    # (7, 0, 0) and its vertex: not matched).  Nothing else is within reach of anything.
    x = float(F(7 / 64) + nxt(0.25))
    v = [(-0.25, 0, 0), (-0.5, 0.25, 0), (-0.5, -0.25, 0), (x, 0, 0), (x + 0.25, 0.25, 0), (x + 0.25, -0.25, 0)]
    add("max_dist_edge", craft([(0, 0, 0)], tsdf=F(0.03125), weight=1), SMALL, VS64,
        (v, [HIGH] * 3 + [LOW] * 3, [(0, 1, 2), (3, 4, 5)]), params=_p(max_dist=0.25))

    # ---- the grid ---------------------------------------------------------------------------------------------------
    cell = float(F(8) * F(VS))
    # the box of the large triangle covers the block's cell, its surface lies 0.28 m and more away; the small triangle
    # two rings out is nearer to the voxels at the block's far side
    big = ([(1.5, -0.3, -0.3), (-0.3, 1.5, -0.3), (-0.3, -0.3, 1.5)], [LOW] * 3, [(0, 1, 2)])
    near = ([(0.40, 0.05, 0.05), (0.42, 0.07, 0.05), (0.40, 0.07, 0.07)], [HIGH] * 3, [(0, 1, 2)])
    add("covering_box", craft([(0, 0, 0)], tsdf=sparse_tsdf([(0, 0, 0)], 2), weight=1), SMALL, VS, join(big, near),
        params=_p(max_dist=0.6), wrong=("first_hit",), grid_cell=cell)
    # a long triangle passes the block, its first vertex lies four cells away; a decoy is nearer in cells, not in metres
    long_ = ([(-0.7, 0.05, 0.05), (0.5, 0.02, 0.3), (0.5, 0.3, 0.02)], [HIGH] * 3, [(0, 1, 2)])
    decoy = ([(0.25, 0.30, 0.30), (0.27, 0.30, 0.30), (0.25, 0.32, 0.30)], [LOW] * 3, [(0, 1, 2)])
    add("spanning", craft([(0, 0, 0)], tsdf=sparse_tsdf([(0, 0, 0)], 2), weight=1), SMALL, VS, join(long_, decoy),
        params=_p(max_dist=0.3), wrong=("single_cell",), grid_cell=cell)
    # queries on a cell border, the winner in the neighbouring and in the diagonal cell (score_cases' points as
    # triangles); negative coordinates, where truncation files the voxel one cell too high
    two = [(0, 0, 0), (-1, -1, -1)]
    b = sc.case("cell_border")
    add("cell_border", craft(two, tsdf=sparse_tsdf(two), weight=1), SMALL, VS,
        small_tris(b.points, b.labels, 0.004), params=_p(max_dist=0.3), wrong=(), grid_cell=cell)
    neg = [(-1, -1, -1), (-2, -1, -1)]
    b = sc.case("negative")
    add("negative", craft(neg, tsdf=sparse_tsdf(neg, 3), weight=1), SMALL, VS, small_tris(b.points, b.labels, -0.004),
        params=_p(max_dist=0.3), wrong=("truncate",), grid_cell=cell)
    # triangles far outside the map, and blocks far outside the triangles' bounding box: the ring loop ends
    three = [(0, 0, 0), (4000, 0, 0), (0, -3000, 17)]
    pts, lab = around(rng, craft([(0, 0, 0)]), VS, 40)
    near_mesh = small_tris(pts, lab, 0.02, rng)
    add("far", craft(three, tsdf=sparse_tsdf(three)), SMALL, VS,
        join(near_mesh, small_tris([(-5000.0, 0.1, 0.1), (0.1, 0.1, 900.0)], [HIGH, LOW], 0.5)),
        params=_p(max_dist=0.5))
    # score_cases' ring of more than 256 rows of cells, its three points as triangles a quarter of a cell wide
    b = sc.case("wide_ring")
    add("wide_ring", b.blocks, SMALL, VS64, small_tris(b.points, b.labels, VS64 / 4), cell=VS64, params=b.params)

    # ---- dropped --------------------------------------------------------------------------------------------------
    blk3 = [(0, 0, 0), (1, 0, 0), (0, 1, 1)]
    blk = craft(blk3, tsdf=sparse_tsdf(blk3, 2))

    def cloud(k, lo=-0.1, hi=0.4, size=0.03):
        return small_tris(rng.uniform(lo, hi, size=(k, 3)), rng.integers(0, 3, size=k), size, rng)

    v, l, t = cloud(60)
    v[::7, 0], v[3::11, 1], v[5::13, 2], v[0] = np.nan, np.inf, -np.inf, (np.nan, np.nan, np.nan)
    add("non_finite", blk, SMALL, VS, (v, l, t))
    # coincident vertices: an index used twice, two vertices with equal coordinates, -0.0 against 0.0; the fourth
    # triangle (collinear, distinct) and the rest are kept
    v0, l0, t0 = cloud(20)
    v = [(0.05, 0.05, 0.05), (0.09, 0.05, 0.05), (0.05, 0.05, 0.05), (0.0, 0.06, -0.0), (-0.0, 0.06, 0.0),
         (0.07, 0.09, 0.05), (0.13, 0.05, 0.05)]
    add("coincident", blk, SMALL, VS,
        join((v, [HIGH, LOW, IGNORE, HIGH, LOW, HIGH, LOW], [(0, 1, 1), (0, 1, 2), (3, 4, 5), (0, 1, 6), (5, 3, 4)]),
             (v0, l0, t0)))
    # vertices no triangle uses, among them a NaN and one far away: they take no part in the bounding box
    v0, l0, t0 = cloud(20)
    add("unused_vertices", blk, SMALL, VS,
        join(([(np.nan, 0, 0), (700.0, -700.0, 30.0), (0.1, 0.1, 0.1)], [LOW, HIGH, IGNORE], np.zeros((0, 3))),
             (v0, l0, t0)))
    v = [(0.05, 0.05, 0.05), (np.nan, 0.05, 0.05), (0.09, 0.09, 0.09)]
    add("all_dropped", blk, SMALL, VS, (v, [LOW, HIGH, LOW], [(0, 1, 2), (0, 0, 2), (2, 0, 2)]))
    add("no_vertices", blk, SMALL, VS, (np.zeros((0, 3)), [], np.zeros((0, 3))))

    # ---- shapes ---------------------------------------------------------------------------------------------------
    # collinear triangles with distinct vertices: the exact segment distance, no NaN
    p0 = rng.uniform(0.0, 0.3, size=(30, 3))
    d = rng.uniform(-0.04, 0.04, size=(30, 3))
    col = np.stack([p0, p0 + d, p0 + d * rng.uniform(-1.5, 2.5, size=(30, 1))], axis=1).reshape(-1, 3)
    col[:9] = np.stack([p0[:3], p0[:3] + [0.03, 0, 0], p0[:3] + [0.0475, 0, 0]], axis=1).reshape(-1, 3)  # (exactly)
    add("collinear", blk, SMALL, VS, (col, rng.integers(0, 3, size=90), np.arange(90).reshape(-1, 3)))
    # slivers 1e-6 thin, 2 to 5 cm long
    a = rng.uniform(-0.05, 0.35, size=(120, 3))
    u = rng.normal(size=(120, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(u, rng.normal(size=(120, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    ln = rng.uniform(0.02, 0.05, size=(120, 1))
    sl = np.stack([a, a + u * ln, a + u * ln * rng.uniform(0.1, 0.9, size=(120, 1)) + w * 1e-6], axis=1).reshape(-1, 3)
    add("slivers", blk, SMALL, VS, (sl, rng.integers(0, 3, size=360), np.arange(360).reshape(-1, 3)),
        wrong=("fma",))
    # triangles of 1e-20 extent at the origin (their products underflow) among ordinary ones
    tiny = ([(0, 0, 0), (1e-20, 0, 0), (0, 1e-20, 0), (1e-20, 1e-20, 3e-20), (-2e-20, 1e-20, 0), (0, 0, 1e-20)],
            [HIGH, HIGH, HIGH, LOW, LOW, LOW], [(0, 1, 2), (3, 4, 5)])
    add("tiny", blk, SMALL, VS, join(tiny, cloud(10, 0.1, 0.4)), params=_p(max_dist=0.2))
    # coordinates of 1e30: products overflow, dist2 is inf or NaN and never within reach; the grid's cell grows
    huge = ([(-1e30, 0, 0), (0, 2e30, 0), (3e38, -3e38, 3e38), (1e30, 1e30, 1e30), (0.1, 0.1, 0.1), (0.1, 1e30, 0.1)],
            [HIGH, LOW, LOW, HIGH, LOW, HIGH], [(0, 1, 2), (3, 4, 5)])
    add("huge", craft([(0, 0, 0)], tsdf=sparse_tsdf([(0, 0, 0)])), SMALL, VS, join(near_mesh, huge),
        params=_p(max_dist=0.5))

    # ---- sizes ----------------------------------------------------------------------------------------------------
    for k in (0, 1, 255, 256, 257):
        add(f"tris_{k}", blk, SMALL, VS, join(([(0.2, 0.2, 0.2)], [HIGH], np.zeros((0, 3))), cloud(k)))
    for k in (CHUNK + 44, 2 * CHUNK + 88):                 # one cell, more than one and more than two LDS chunks
        add(f"crowded_{k}", craft([(0, 0, 0)], tsdf=sparse_tsdf([(0, 0, 0)], 2)), SMALL, VS,
            cloud(k, 0.03, 0.12, 0.015))
    # twenty triangles that each span the whole 100 m box, over a grid of 0.16 m cells: the cell limit doubles the edge
    # twice, the reference cap once more
    corner = np.array([(-50, -50, -50), (50, 50, -50), (-50, 50, 50)], dtype=D)
    span = np.concatenate([corner + rng.uniform(0, 0.5, size=(3, 3)) * [(1, 1, 1), (-1, -1, 1), (1, -1, -1)]
                           for _ in range(20)])
    add("ref_cap", blk, SMALL, VS, join((span, rng.integers(0, 3, size=60), np.arange(60).reshape(-1, 3)), cloud(40)),
        params=_p(max_dist=1.0))

    # ---- selection and score: score_cases' blocks of edge values against a lattice of small triangles -------------
    lat = (np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) * 2 + 0.5) * VS
    lattice = small_tris(lat, np.arange(64) % 3, 0.007)
    add("selection", sc.case("selection").blocks, SMALL, VS, lattice, params=_p(min_weight=2), wrong=("select_le",))
    add("score", sc.case("score").blocks, SMALL, VS, lattice, wrong=("cutoff_ge", "bin_round"))

    # ---- layout: chain walks, the table's last entry, both ends of the int16 grid ------------------------------------
    for m, per_block, md in ((qc.tiny_table(), 3, 0.3), (qc.known_order(), 30, 0.3), (qc.edges(), 30, 1.0)):
        p, lab = around(rng, m.blocks, VS, per_block)
        add(f"layout_{m.name}", m.blocks, m.engine, VS, small_tris(p, lab, 0.02, rng), params=_p(max_dist=md))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


NAMES = ("voronoi", "ties", "mixed_labels", "mesh_against_points", "max_dist_edge", "covering_box", "spanning",
         "cell_border", "negative", "far", "wide_ring", "non_finite", "coincident", "unused_vertices", "all_dropped", "no_vertices",
         "collinear", "slivers", "tiny", "huge", "tris_0", "tris_1", "tris_255", "tris_256", "tris_257", "crowded_300",
         "crowded_600", "ref_cap", "selection", "score", "layout_tiny_table", "layout_known_order", "layout_edges")

VARIANTS = ("nearest_vertex", "plane_distance", "box_distance", "ties_highest", "label_of_nearest_vertex",
            "label_of_last_vertex", "first_hit", "single_cell", "truncate", "select_le", "cutoff_ge", "bin_round", "fma")


# ---------------------------------------------------------------------------------------------------------------------
def expected_info(c):
    """ratsdf_labelmesh_info of a case's set, from the header's rules"""
    v, t = mr.as_mesh(c.vertices, c.triangles)
    keep = mr.kept_triangles(v, t)
    e = F(8) * F(c.vs) if c.cell == 0 else F(c.cell)
    while e < F(1e-6):
        e = F(e * F(2))
    info = dict(vertices=len(v), triangles=len(t), kept=len(keep), mixed=mr.mixed_triangles(v, c.labels, t), refs=0,
                origin=(0.0, 0.0, 0.0), cells=(1, 1, 1))
    if len(keep):
        corners = v[t[keep]]                                         # [k, 3, 3]
        tlo, thi = corners.min(axis=1).astype(D), corners.max(axis=1).astype(D)
        lo, hi = tlo.min(axis=0), thi.max(axis=0)
        while True:
            cells = np.floor((hi - lo) / float(e)) + 1
            if cells.prod() <= MAX_CELLS:
                spans = np.floor((thi - lo) / float(e)) - np.floor((tlo - lo) / float(e)) + 1
                refs = int(spans.prod(axis=1).sum())
                if refs <= MAX_REFS:
                    break
            e = F(e * F(2))
        info.update(origin=tuple(float(F(x)) + 0.0 for x in lo), cells=tuple(int(x) for x in cells), refs=refs)
    info["cell"] = float(e)
    return info


def rows_in_order(c, directory_blocks):
    """the rows of the case's BlockSet in the order of a directory dump"""
    return qc.rows_of(c.blocks, qc.directory_positions(directory_blocks))


_CACHE = {}


def _score(c, rows, **kw):
    b = c.blocks
    return mr.score(b.pos[rows], b.tsdf[rows], b.rgbw["weight"][rows], b.prob[rows], c.vs, c.vertices, c.labels,
                    c.triangles, **c.params, **kw)


def expected(c, rows, **variant):
    """(score record, per-voxel records) of case `c` with its blocks gathered in the order `rows`; computed once per
    order and variant, shared, never changed"""
    key = (c.name, np.asarray(rows).tobytes(), tuple(sorted(variant.items())))
    if key not in _CACHE:
        rec, pv = _score(c, rows, **variant)
        rec.setflags(write=False)
        pv.setflags(write=False)
        _CACHE[key] = (rec, pv)
    return _CACHE[key]


def grid_cell_of(c):
    return c.grid_cell or float(F(8) * F(c.vs))


def through_grid(c, **kw):
    """the case's result with score_mesh_ref.grid_nearest as the search (blocks in list order)"""
    fn = lambda q, md: mr.grid_nearest(q, c.vertices, c.triangles, md, grid_cell_of(c), **kw)
    return _score(c, np.arange(len(c.blocks)), nearest_fn=fn)


def variant(c, name):
    """the result of the WRONG variant `name` on case `c` (blocks in list order), and of the contract computed the
    same way: (wrong, right), each (score record, per-voxel records)"""
    rows = np.arange(len(c.blocks))
    if name in ("truncate", "first_hit", "single_cell"):
        return through_grid(c, **{name: True}), through_grid(c)
    if name in mr.DIST_VARIANTS:
        return expected(c, rows, variant=name), expected(c, rows)
    if name.startswith("label_of_"):
        return expected(c, rows, label_of=name.split("_")[2]), expected(c, rows)
    return expected(c, rows, **{name: True}), expected(c, rows)


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
