"""Crafted maps and labelled point sets for the label score (include/ratsdf_score.h), and the wrong variants each must
catch.  Same role as readout_cases.py: no GPU and no torch at import; what is expected comes from the BlockSet a map was
written from and tests/score_ref.py, never from an engine (an engine's directory dump only says in which order the
blocks are gathered).  tests/test_score_cases.py evaluates the variants without a GPU, tests/test_gpu_score.py runs
every case on the engine.

Maps are a handful of blocks.  Where exact ties and exact distances are wanted the voxel size is 1 / 64, so that every
voxel coordinate and every difference to the crafted points is exact in float32; the other cases use query_cases' 0.02.
"""
import functools
from typing import NamedTuple

import numpy as np

import query_cases as qc
import score_ref
from ratsdf._abi import RGBW_DTYPE
from raycast_cases import BlockSet
from score_ref import HIGH, IGNORE, LOW

F = np.float32
VS = qc.VS
VS64 = 1.0 / 64
SMALL = dict(block_bits=8, bucket_bits=12)


class Case(NamedTuple):
    name: str
    blocks: BlockSet
    engine: dict             # table sizes of the engine the map is loaded into
    vs: float
    points: np.ndarray       # [k, 3] float32
    labels: np.ndarray       # [k] uint8
    cell: float              # what label_set() is given (0: 8 voxel sizes)
    params: dict             # tsdf_below, max_dist, p_cutoff, min_weight
    wrong: tuple = ()        # names of WRONG variants (variant()) this case must tell from the contract
    grid_cell: float = 0.0   # the cell of score_ref.grid_nearest for the variants that need a grid


def nxt(x, up=True):
    return np.nextafter(F(x), F(np.inf if up else -np.inf))


def craft(pos, tsdf=None, weight=None, prob=None):
    """a BlockSet at `pos`: tsdf / weight / prob are [n, 512] arrays, a scalar, or None for query_cases' functions of
    the voxel coordinate (tsdf scattered over [-1, 1), weights 0 .. 3, prob in [0, 1))"""
    pos = np.asarray(pos, dtype=np.int64).reshape(-1, 3)
    v = qc.voxel_coordinates(pos)
    shape = v.shape[:2]
    rgbw = np.zeros(shape, dtype=RGBW_DTYPE)
    rgbw["r"], rgbw["g"], rgbw["b"] = (37 * v[..., 0]) & 255, (59 * v[..., 1]) & 255, (83 * v[..., 2]) & 255
    rgbw["weight"] = ((v[..., 0] + 3 * v[..., 1] + 5 * v[..., 2]) & 3) if weight is None else weight
    t = qc.tsdf_of(v) if tsdf is None else np.broadcast_to(np.asarray(tsdf, dtype=F), shape).copy()
    p = qc.prob_of(v) if prob is None else np.broadcast_to(np.asarray(prob, dtype=F), shape).copy()
    return BlockSet(pos.astype(np.int16), t, rgbw, p)


def sparse_tsdf(pos, every=4):
    """0.05 (selected at the reference's 0.1) on every `every`-th voxel by coordinate sum, 0.5 elsewhere"""
    v = qc.voxel_coordinates(np.asarray(pos, dtype=np.int64).reshape(-1, 3))
    return np.where((v.sum(axis=-1) % every) == 0, F(0.05), F(0.5)).astype(F)


def around(rng, blocks, vs, per_block, spread=1.5):
    """per_block random float32 points within `spread` block edges of each block's centre, labels 0 .. 2"""
    c = (qc.wrap16(np.asarray(blocks.pos).astype(np.int64) << 3) + 4).astype(np.float64) * vs   # (wrapped: block 4096)
    pts = (c[:, None, :] + rng.uniform(-spread * 8 * vs, spread * 8 * vs, size=(len(c), per_block, 3))).reshape(-1, 3)
    return pts.astype(F), rng.integers(0, 3, size=len(pts)).astype(np.uint8)


PARAMS = dict(tsdf_below=0.1, max_dist=0.3, p_cutoff=0.5, min_weight=0)
WIDE_RING_POINTS = np.array([(-8, -8, -8), (16, 16, 16), (3.5, 3.5, 12.5)])   # of "wide_ring", in voxel sizes


def _p(**kw):
    return {**PARAMS, **kw}


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261020)
    out = []

    def add(name, blocks, engine, vs, points, labels, cell=0.0, params=None, wrong=(), grid_cell=0.0):
        points = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
        labels = np.ascontiguousarray(labels, dtype=np.uint8).reshape(-1)
        assert len(points) == len(labels)
        out.append(Case(name, blocks, engine, vs, points, labels, cell, params or _p(), tuple(wrong), grid_cell))

    # ---- nearest ----------------------------------------------------------------------------------------------------
    # exact ties at the voxels of the plane x = 0 (two points, and their duplicates) and at the origin (three); the
    # far point holds index 0, so "the first in memory" is not the answer either.  The duplicates carry other labels.
    a = 1.0 / 128
    quad = craft([(0, 0, 0), (-1, -1, -1), (-1, 0, 0), (0, -1, 0)], tsdf=F(0.03125), weight=1)
    add("ties", quad, SMALL, VS64, [(0.5, 0.5, 0.5), (a, 0, 0), (-a, 0, 0), (0, a, 0), (-a, 0, 0), (a, 0, 0)],
        [IGNORE, LOW, HIGH, HIGH, LOW, HIGH], params=_p(max_dist=0.25), wrong=("ties_highest",))
    # d2 == max_dist^2 exactly (voxel (0, 0, 0) and the point at -0.25: matched), and one float32 step beyond (voxel
    # (7, 0, 0) and its point: not matched).  Nothing else is within reach of anything.
    one = craft([(0, 0, 0)], tsdf=F(0.03125), weight=1)
    add("max_dist_edge", one, SMALL, VS64, [(-0.25, 0, 0), (F(7 / 64) + nxt(0.25), 0, 0)], [HIGH, LOW],
        params=_p(max_dist=0.25))
    # queries on a cell border (the grid's origin is the anchor at -0.32 = -2 cells, so the voxel at 0 lies on the
    # lattice): the winner in the neighbouring cell, in the diagonal one, and a farther point in the voxel's own cell,
    # which a search that stops at the first ring with a hit returns
    two = [(0, 0, 0), (-1, -1, -1)]
    pts = [(-0.32, -0.32, -0.32), (0.64, 0.64, 0.64), (0.15, 0.15, 0.15), (-0.01, 0.004, 0.004),
           (-0.013, -0.013, -0.013), (0.155, 0.01, 0.01), (0.01, -0.005, 0.15), (-0.15, -0.15, -0.01)]
    add("cell_border", craft(two, tsdf=sparse_tsdf(two), weight=1), SMALL, VS, pts,
        [IGNORE, LOW, LOW, HIGH, HIGH, LOW, HIGH, LOW], params=_p(max_dist=0.3), wrong=("first_hit",),
        grid_cell=float(F(8) * F(VS)))
    # negative coordinates: voxel (-7, -7, -7) lies 0.875 cells below zero.  Truncation puts it in cell 0, the ring
    # around which misses the point in cell -2 at 0.03 and is content with the one at 0.12
    neg = [(-1, -1, -1), (-2, -1, -1)]
    pts = [(-0.02, -0.14, -0.14), (-0.17, -0.14, -0.14), (-0.30, -0.02, -0.02), (-0.01, -0.01, -0.01)]
    add("negative", craft(neg, tsdf=sparse_tsdf(neg, 3), weight=1), SMALL, VS, pts, [LOW, HIGH, HIGH, IGNORE],
        params=_p(max_dist=0.3), wrong=("truncate",), grid_cell=float(F(8) * F(VS)))
    # points far outside the map, and a block far outside the points' bounding box: the ring loop ends, all unmatched
    far = craft([(0, 0, 0), (4000, 0, 0), (0, -3000, 17)], tsdf=sparse_tsdf([(0, 0, 0), (4000, 0, 0), (0, -3000, 17)]))
    near_pts, near_lab = around(rng, craft([(0, 0, 0)]), VS, 40)
    add("far", far, SMALL, VS, np.concatenate([near_pts, [(-5000.0, 0.1, 0.1), (0.1, 0.1, 900.0)]]),
        np.concatenate([near_lab, [HIGH, LOW]]), params=_p(max_dist=0.5))
    add("huge", craft([(0, 0, 0)], tsdf=sparse_tsdf([(0, 0, 0)])), SMALL, VS,
        np.concatenate([near_pts, [(-1e30, 0, 0), (0, 2e30, 0), (3e38, -3e38, 3e38)]]),
        np.concatenate([near_lab, [HIGH, LOW, LOW]]), params=_p(max_dist=0.5))
    # a ring of more than 256 rows of cells, which the walk takes in two passes: cells of one voxel size, two far
    # points that stretch the grid 8 and 9 cells beyond the block, and the one point within reach (6 cells) 5.5 cells
    # above the block's top plane.  The top voxels under it first meet it in ring 5 (18 x 18 rows), in the last slab.
    add("wide_ring", craft([(0, 0, 0)], tsdf=F(0.03125), weight=1), SMALL, VS64, WIDE_RING_POINTS * VS64,
        [LOW, IGNORE, HIGH], cell=VS64, params=_p(max_dist=6 * VS64))

    # ---- set shape --------------------------------------------------------------------------------------------------
    blk = craft([(0, 0, 0), (1, 0, 0), (0, 1, 1)], tsdf=sparse_tsdf([(0, 0, 0), (1, 0, 0), (0, 1, 1)], 2))
    add("one_cell", blk, SMALL, VS, rng.uniform(0.05, 0.12, size=(5, 3)), [LOW, HIGH, IGNORE, HIGH, LOW])
    spread = rng.uniform(-50, 50, size=(300, 3))           # (100 m / 0.16 m)^3 cells: the edge doubles twice
    spread[:40] = rng.uniform(-0.1, 0.4, size=(40, 3))
    add("doubled_cell", blk, SMALL, VS, spread, rng.integers(0, 3, size=300), params=_p(max_dist=1.0))
    for k in (2049, 4097):                                  # one cell, more than one and more than two LDS chunks
        add(f"crowded_{k}", craft([(0, 0, 0)], tsdf=sparse_tsdf([(0, 0, 0)], 2)), SMALL, VS,
            rng.uniform(0.01, 0.15, size=(k, 3)), rng.integers(0, 3, size=k))
    for k in (0, 1, 255, 256, 257):
        add(f"points_{k}", blk, SMALL, VS, rng.uniform(-0.1, 0.4, size=(k, 3)), rng.integers(0, 3, size=k))
    bad = rng.uniform(-0.1, 0.4, size=(60, 3)).astype(F)
    bad[::7, 0], bad[3::11, 1], bad[5::13, 2], bad[0] = np.nan, np.inf, -np.inf, (np.nan, np.nan, np.nan)
    add("non_finite", blk, SMALL, VS, bad, rng.integers(0, 3, size=60))
    add("none_finite", blk, SMALL, VS, np.full((4, 3), np.nan), [LOW, HIGH, LOW, IGNORE])

    # ---- selection and score: one block whose first slots hold the edge values -------------------------------------
    T = F(0.1)
    t = np.full((1, 512), F(0.05), dtype=F)
    edge_t = [T, -T, nxt(T, False), -nxt(T, False), nxt(T), -nxt(T), F(np.nan), F(np.inf), F(-np.inf), F(0), F(-0.0),
              np.uint32(0xFFC00001).view(F), np.uint32(1).view(F)]
    t[0, :len(edge_t)] = edge_t
    w = ((np.arange(512) + 2) % 5).reshape(1, 512)          # weights 0 .. 4 around min_weight = 2; slots 0, 1: 2, 3
    pr = (((np.arange(512) * 37) % 512) / 512.0).astype(F).reshape(1, 512)      # every multiple of 1 / 512 in [0, 1)
    edge_p = [F(k / 256) for k in (1, 2, 127, 128, 129, 255)] + [nxt(F(k / 256), False) for k in (1, 2, 128, 255)] + \
             [F(0), F(-0.0), F(1), nxt(1, False), nxt(1), F(7.5), F(-0.25), F(np.nan), F(np.inf), F(-np.inf),
              nxt(0.5), np.uint32(1).view(F)]
    pr[0, 64:64 + len(edge_p)] = edge_p                     # (slots 64 ..: all selected at tsdf 0.05)
    # labelled points on a 4 x 4 x 4 lattice over the block, the three labels by turns
    lat = (np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) * 2 + 0.5) * VS
    lat_lab = (np.arange(64) % 3).astype(np.uint8)
    add("selection", craft([(0, 0, 0)], tsdf=t, weight=w, prob=pr), SMALL, VS, lat, lat_lab,
        params=_p(min_weight=2), wrong=("select_le",))
    add("score", craft([(0, 0, 0)], tsdf=t, weight=1, prob=pr), SMALL, VS, lat, lat_lab,
        wrong=("cutoff_ge", "bin_round"))

    # ---- layout: chain walks, the table's last entry, both ends of the int16 grid ------------------------------------
    for m, per_block, md in ((qc.tiny_table(), 3, 0.3), (qc.known_order(), 30, 0.3), (qc.edges(), 30, 1.0)):
        p, lab = around(rng, m.blocks, VS, per_block)
        add(f"layout_{m.name}", m.blocks, m.engine, VS, p, lab, params=_p(max_dist=md),
            wrong=("fma",) if m.name == "tiny_table" else ())
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


NAMES = ("ties", "max_dist_edge", "cell_border", "negative", "far", "huge", "wide_ring", "one_cell", "doubled_cell", "crowded_2049",
         "crowded_4097", "points_0", "points_1", "points_255", "points_256", "points_257", "non_finite", "none_finite",
         "selection", "score", "layout_tiny_table", "layout_known_order", "layout_edges")


# ---------------------------------------------------------------------------------------------------------------------
def expected_info(points, cell, vs):
    """ratsdf_labelset_info of a set, from the header's rules"""
    points = np.asarray(points, dtype=F).reshape(-1, 3)
    keep = score_ref.kept_points(points)
    c = F(8) * F(vs) if cell == 0 else F(cell)
    while c < F(1e-6):
        c = F(c * F(2))
    info = dict(points=len(points), kept=len(keep), origin=(0.0, 0.0, 0.0), cells=(1, 1, 1))
    if len(keep):
        lo, hi = points[keep].min(axis=0), points[keep].max(axis=0)
        ext = hi.astype(np.float64) - lo.astype(np.float64)
        while True:
            cells = np.floor(ext / float(c)) + 1
            if cells.prod() <= 2 ** 24:
                break
            c = F(c * F(2))
        info.update(origin=tuple(float(v) + 0.0 for v in lo), cells=tuple(int(v) for v in cells))
    info["cell"] = float(c)
    return info


def ring_row(info, pos, vs, lo, hi=None):
    """where the device's walk (score_walk, kernels_score.h) first meets a record of the set described by `info`
    (expected_info) whose box is lo .. hi (a point: lo alone), from the block at `pos`: (the ring r, the smallest index
    among the rows of cells of ring r's cube that hold a cell of the record).  A workgroup takes 256 rows at a time."""
    o = np.array([float(F(x)) for x in info["origin"]])
    cell, n = float(F(info["cell"])), np.array(info["cells"])
    g0 = qc.wrap16(np.asarray(pos, dtype=np.int64) << 3)
    blo = np.floor(((g0.astype(F) * F(vs)).astype(np.float64) - o) / cell).astype(np.int64)
    bhi = np.floor((((g0 + 7).astype(F) * F(vs)).astype(np.float64) - o) / cell).astype(np.int64)
    lo = np.asarray(lo, dtype=F)
    hi = lo if hi is None else np.asarray(hi, dtype=F)
    clo = np.clip(np.floor((lo.astype(np.float64) - o) / cell).astype(np.int64), 0, n - 1)
    chi = np.clip(np.floor((hi.astype(np.float64) - o) / cell).astype(np.int64), 0, n - 1)
    met = []
    for x in range(clo[0], chi[0] + 1):
        for y in range(clo[1], chi[1] + 1):
            for z in range(clo[2], chi[2] + 1):
                c = np.array([x, y, z])
                r = int(max(0, (blo - c).max(), (c - bhi).max()))
                y0, y1, z0 = max(blo[1] - r, 0), min(bhi[1] + r, n[1] - 1), max(blo[2] - r, 0)
                met.append((r, int((z - z0) * (y1 - y0 + 1) + (y - y0))))
    return min(met)


def rows_in_order(c, directory_blocks):
    """the rows of the case's BlockSet in the order of a directory dump"""
    return qc.rows_of(c.blocks, qc.directory_positions(directory_blocks))


_CACHE = {}


def expected(c, rows, **variant):
    """(score record, per-voxel records) of case `c` with its blocks gathered in the order `rows`; computed once per
    order and variant, shared, never changed"""
    key = (c.name, np.asarray(rows).tobytes(), tuple(sorted(variant.items())))
    if key not in _CACHE:
        b = c.blocks
        rec, pv = score_ref.score(b.pos[rows], b.tsdf[rows], b.rgbw["weight"][rows], b.prob[rows], c.vs, c.points,
                                  c.labels, **c.params, **variant)
        rec.setflags(write=False)
        pv.setflags(write=False)
        _CACHE[key] = (rec, pv)
    return _CACHE[key]


def variant(c, name):
    """the result of the WRONG variant `name` on case `c` (blocks in list order), and of the contract computed the
    same way: (wrong, right), each (score record, per-voxel records)"""
    rows = np.arange(len(c.blocks))
    if name in ("truncate", "first_hit"):
        kw = dict(truncate=True) if name == "truncate" else dict(first_hit=True)
        wrong_fn = lambda q, p, md: score_ref.grid_nearest(q, p, md, c.grid_cell, **kw)
        right_fn = lambda q, p, md: score_ref.grid_nearest(q, p, md, c.grid_cell)
        b = c.blocks
        args = (b.pos[rows], b.tsdf[rows], b.rgbw["weight"][rows], b.prob[rows], c.vs, c.points, c.labels)
        return (score_ref.score(*args, **c.params, nearest_fn=wrong_fn),
                score_ref.score(*args, **c.params, nearest_fn=right_fn))
    return expected(c, rows, **{name: True}), expected(c, rows)


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
