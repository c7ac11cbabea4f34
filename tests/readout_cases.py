"""Crafted maps, point sets, boxes and engine-free restatements for the two planner read-outs: point sampling
(ratsdf_sample_points[_device], include/ratsdf_sample.h) and the ESDF (ratsdf_esdf[_device], include/ratsdf_esdf.h),
with two surface-point boxes on the chained directories.  Written once and run against the CPU oracle's map
(tests/test_readout_cases.py, no GPU) and the HIP engine (tests/test_gpu_readout.py).  Same role as query_cases.py and
raycast_cases.py: no GPU and no torch at import.

What is expected never comes from an engine:
  * corner values come from the BlockSet the map was written from (`blockset_lookup`, on raycast_cases.Lookup), and go
    through sample_ref.sample, the header's fp32 formulas;
  * voxel states come from the BlockSet too (`box_state`, the three rules of ratsdf_esdf.h per voxel), and go through
    esdf_ref.esdf: scipy's exact EDT plus the header's fp32 formula.  The line, slab and plane boxes also carry their
    field in closed form (`Box.by_hand`).
The wrong variants at the end of the file (a permuted corner map, another rounding, no range guard, ...) are what the
CPU test evaluates to show that the named sets tell them apart.

Maps.  signs / known_order / edges / tiny_table are query_cases' (values a function of the unwrapped voxel coordinate,
one special block per map with NaN, -0.0, +-inf and denormals, weights 0 .. 3), loaded into their own small
directories so the chain walk and the wrap at the table's end are taken.  New here: corner_subsets (every subset of a
2 x 2 x 2 block neighbourhood once), signs_weighted (signs with the special slots observed), and the ESDF maps
esdf_lines, esdf_slabs, esdf_random, whose voxel states are chosen per voxel.
"""
import functools
from typing import Callable, NamedTuple

import numpy as np

import esdf_ref
import query_cases as qc
import sample_ref
from esdf_ref import FREE, OCCUPIED, UNKNOWN
from query_cases import F, TRUNC, VS, Map, edges, known_order, load, make_map, signs, tiny_table  # noqa: F401
from ratsdf._abi import RGBW_DTYPE, SAMPLE_ALLOCATED
from raycast_cases import BlockSet, Lookup, block_keys

INF = float("inf")
DENORMAL = float(np.uint32(1).view(F))            # the smallest positive float32 denormal
# the row of the special block in each of query_cases' maps (make_map's special_row)
SPECIAL_ROWS = {"signs": 0, "signs_weighted": 0, "known_order": 1, "edges": 6, "tiny_table": 199}


# ---------------------------------------------------------------------------------------------------------------------
# voxel values out of a BlockSet
def slot_of(v):
    """voxel x + 8y + 64z inside its block, for integer voxel coordinates [..., 3]"""
    v = np.asarray(v).astype(np.int64)
    return (v[..., 0] & 7) + (v[..., 1] & 7) * 8 + (v[..., 2] & 7) * 64


def fetch(look, blk, slot):
    """(allocated, tsdf, rgbw, prob) of voxel `slot` of the blocks at block coordinates `blk` ([n, 3])"""
    r = look.rows(np.asarray(blk).astype(np.int64) * 8)
    ok = r >= 0
    rr = np.where(ok, r, 0)
    m = look.m
    rgbw = m.rgbw[rr, slot].copy()
    rgbw[~ok] = np.zeros(1, dtype=RGBW_DTYPE)
    return ok, np.where(ok, m.tsdf[rr, slot], F(-10)), rgbw, np.where(ok, m.prob[rr, slot], F(0))


def blockset_lookup(blocks, look=None, perm=None):
    """the `lookup` of sample_ref.sample from a BlockSet alone.  perm (WRONG unless None): the corner-to-block map with
    its axes permuted -- the corner that lies (dx, dy, dz) blocks from the floor's block is read from the block at
    (d[perm[0]], d[perm[1]], d[perm[2]]); the voxel inside the block is the right one."""
    look = Lookup(blocks) if look is None else look

    def lookup(v):
        v = np.asarray(v).astype(np.int64)
        blk = v >> 3
        if perm is not None:
            c = blk.reshape(8, -1, 3)                      # sample_ref.sample asks corner-major; corner 0 is the floor
            blk = (c[0][None] + (c - c[0][None])[..., list(perm)]).reshape(-1, 3)
        return fetch(look, blk, slot_of(v))
    return lookup


def box_state(blocks, origin, dims, occupied_below=0.0, occupied=None, look=None):
    """the states of a box, (dims[2], dims[1], dims[0]) uint8, by the rules of ratsdf_esdf.h voxel by voxel: UNKNOWN
    when the voxel's block is not in the map or its weight is 0, OCCUPIED when tsdf <= occupied_below (fp32), FREE
    otherwise.  occupied(t, threshold) replaces the comparison (the wrong variants below)."""
    look = Lookup(blocks) if look is None else look
    (ox, oy, oz), (X, Y, Z) = (int(v) for v in origin), (int(v) for v in dims)
    assert min(ox, oy, oz) >= -32768 and max(ox + X, oy + Y, oz + Z) <= 32768 and min(X, Y, Z) >= 1
    z, y, x = np.meshgrid(np.arange(oz, oz + Z), np.arange(oy, oy + Y), np.arange(ox, ox + X), indexing="ij")
    v = np.stack([x, y, z], axis=-1)
    ok, t, c, _ = fetch(look, v >> 3, slot_of(v))
    with np.errstate(invalid="ignore"):
        occ = (t <= F(occupied_below)) if occupied is None else occupied(t, F(occupied_below))
    return np.where(~ok | (c["weight"] == 0), UNKNOWN, np.where(occ, OCCUPIED, FREE)).astype(np.uint8)


def special_voxels(m):
    """[k, 3] the voxels of the map's special block that hold a special tsdf or probability"""
    slots = np.array(sorted(set(qc.SPECIAL_TSDF) | set(qc.SPECIAL_PROB)))
    return qc.voxel_coordinates(m.blocks.pos[SPECIAL_ROWS[m.name]])[0][slots]


def cell_of(points):
    """floorf(p / vs) of float32 points as int64 (finite points in the int32 range only)"""
    return np.floor(np.asarray(points, dtype=F) / F(VS)).astype(np.int64)


def touches_special(m, points):
    """[n] bool: one of the 8 corners of the point's cell is a special voxel of the map"""
    d = cell_of(points)[:, None, :] - special_voxels(m)[None, :, :]
    return np.any(np.all((d >= -1) & (d <= 0), axis=2), axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# point coordinates
def preimage(t):
    """a float32 p whose quotient p / vs is the float32 `t` bit for bit, or None: the quotient skips some values"""
    t, vs = F(t), F(VS)
    p0 = F(t * vs)
    for step in (0, 1, -1, 2, -2, 3, -3):
        p = p0
        for _ in range(abs(step)):
            p = np.nextafter(p, F(INF if step > 0 else -INF))
        if (p / vs).view(np.uint32) == t.view(np.uint32):
            return p
    return None


def coord(t):
    """the coordinate for grid value t: exact where the quotient can be, else the rounded product"""
    p = preimage(t)
    return F(F(t) * F(VS)) if p is None else p


def _grid(values):
    """the float32 points of the product values^3, x slowest"""
    c = np.array(values, dtype=F)
    return np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)


def _cells(floors, fractions):
    """points at every floor ([n, 3] ints) + fraction triple ([k, 3]), as metres: [n * k, 3] float32"""
    g = np.asarray(floors, dtype=np.float64)[:, None, :] + np.asarray(fractions, dtype=np.float64)[None, :, :]
    return (g.reshape(-1, 3) * VS).astype(F)


QUARTERS = qc._cube((0, 0, 0), (2, 2, 2)) * 0.5 + 0.25          # the nearest voxel at each of the 8 corners
FRACTIONS4 = qc._cube((0, 0, 0), (4, 4, 4)) * 0.25              # 0, 1/4, 1/2, 3/4 per axis


# ---------------------------------------------------------------------------------------------------------------------
# corner_subsets
CLUSTER_GRID, CLUSTER_STEP, CLUSTER_BASE = (8, 8, 4), 4, (-16, -16, -8)
CORNER_BLOCKS = qc._cube((0, 0, 0), (2, 2, 2))                  # bit k of a subset: block (k >> 2, (k >> 1) & 1, k & 1)


def cluster_base(s):
    """the block at corner (0, 0, 0) of cluster s: a 8 x 8 x 4 grid of clusters four blocks apart (two blocks of
    cluster, two of gap: a point's corners never reach the next cluster), half of it at negative coordinates"""
    s = np.asarray(s)
    i = np.stack([s >> 5, (s >> 2) & 7, s & 3], axis=-1)
    return np.asarray(CLUSTER_BASE) + CLUSTER_STEP * i


@functools.lru_cache(maxsize=None)
def corner_subsets():
    """cluster s (0 .. 255) holds exactly the blocks of its 2 x 2 x 2 neighbourhood whose bit is set in s: 1024 blocks.
    No special block: every record of this map compares as bytes."""
    pos = [cluster_base(s) + CORNER_BLOCKS[k] for s in range(256) for k in range(8) if (s >> k) & 1]
    return Map("corner_subsets", make_map(np.array(pos), special_row=None), dict(block_bits=11, bucket_bits=12))


def corner_subsets_points():
    """per cluster the cells that straddle its blocks: floor local 7 on all three axes, on two and on one (the other
    axes at local 3 of the lower or of the upper block), each at the 8 quarter fractions"""
    locals_ = [(a, b, c) for a in (3, 7, 11) for b in (3, 7, 11) for c in (3, 7, 11) if 7 in (a, b, c)]
    floors = (cluster_base(np.arange(256)) * 8)[:, None, :] + np.array(locals_)[None, :, :]
    return _cells(floors.reshape(-1, 3), QUARTERS)


# ---------------------------------------------------------------------------------------------------------------------
# point sets
class PointSet(NamedTuple):
    name: str
    map: Map
    points: np.ndarray       # [n, 3] float32 metres
    nan_allowed: bool = False


def _signs_values():
    """grid values of `signs` (voxels -16 .. 15) and a layer around: integers, exact halves, and odd ones"""
    ints = [coord(i) for i in range(-17, 17)]
    halves = [p for p in (preimage(l + 0.5) for l in range(-18, 17)) if p is not None]
    ulps = [p for i in (-16, -9, -8, -1, 1, 7, 8, 15) for s in (-INF, INF)
            for p in [preimage(np.nextafter(F(i), F(s)))] if p is not None]
    odd = [F(-0.0), F(0.0), F(DENORMAL), F(-DENORMAL), np.uint32(0x00400000).view(F)] + ulps
    return ints, halves, odd


@functools.lru_cache(maxsize=None)
def point_sets():
    rng = np.random.default_rng(20240607)
    s, sets = signs(), []

    def add(name, m, pts, special=None):
        pts = np.ascontiguousarray(pts, dtype=F).reshape(-1, 3)
        if m.name in SPECIAL_ROWS and special is not None:
            pts = pts[touches_special(m, pts) == special]
        assert len(pts) > 0, name
        sets.append(PointSet(name, m, pts, bool(special)))

    sets.append(PointSet("corner_subsets", corner_subsets(), corner_subsets_points()))
    ints, halves, odd = _signs_values()
    add("signs_integer", s, _grid(ints), special=False)
    every = np.array(ints + halves + odd, dtype=F)
    half = np.array(halves, dtype=F)
    add("signs_halves", s, half[rng.integers(0, len(half), size=(8000, 3))], special=False)
    add("signs_odd", s, every[rng.integers(0, len(every), size=(20000, 3))], special=False)
    floors = (special_voxels(s)[:, None, :] - qc._cube((0, 0, 0), (2, 2, 2))[None, :, :]).reshape(-1, 3)
    add("specials", s, _cells(np.unique(floors, axis=0), FRACTIONS4), special=True)
    # the ends of the int16 range: per axis the last cell inside (floor 32766 / -32768) and the first outside, the
    # other two floors inside block 0 (0 .. 6: no corner leaves it)
    inside, outside = [], []
    others = qc._cube((0, 0, 0), (7, 7, 1))[::3, :2]
    for a in range(3):
        for end, out in ((32766, 32767), (-32768, -32769)):
            for dst, f in ((inside, end), (outside, out)):
                fl = np.insert(others, a, f, axis=1)
                dst.append(_cells(fl, QUARTERS))
    add("edges_inside", edges(), np.concatenate(inside))
    add("edges_outside", edges(), np.concatenate(outside))
    for m in (tiny_table(), known_order()):
        v = qc.voxel_coordinates(m.blocks.pos).reshape(-1, 3)
        values = np.unique(v)                                    # every integer voxel point of every block
        add(f"{m.name}_integer", m, np.array([coord(c) for c in values], dtype=F)[np.searchsorted(values, v)],
            special=False)
        pick = v[rng.integers(0, len(v), size=min(20000, 2 * len(v)))]
        add(f"{m.name}_jitter", m, ((pick + rng.uniform(-1.5, 1.5, size=pick.shape)) * VS).astype(F), special=False)
    assert len({p.name for p in sets}) == len(sets)
    return sets


def point_set(name):
    return next(p for p in point_sets() if p.name == name)


BATCH_LENGTHS = (1, 255, 256, 257)          # one lane, a workgroup less one, a workgroup, a workgroup and one lane


@functools.lru_cache(maxsize=None)
def expected_samples(name):
    """the records of the point set `name`: computed once, shared, never changed"""
    ps = point_set(name)
    with np.errstate(invalid="ignore", over="ignore"):          # the special block's NaNs and infinities
        out = sample_ref.sample(ps.points, VS, blockset_lookup(ps.map.blocks))
    out.setflags(write=False)
    return out


def _components(rec):
    """[n, 4] the tsdf and the three gradient components"""
    return np.concatenate([rec["tsdf"][:, None], rec["grad"]], axis=1)


def nan_components(want):
    """[n, 4] bool: components the restatement has as NaN while ALLOCATED is set -- x86 and the GPU keep different
    payloads and signs when a NaN goes through arithmetic, so only their being NaN is compared"""
    return np.isnan(_components(want)) & ((want["flags"] & SAMPLE_ALLOCATED) != 0)[:, None]


def assert_samples(got, want, what, nan_allowed=False):
    """byte equality of two record arrays; where nan_allowed, the NaN components of nan_components() need only be NaN"""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = nan_components(want)
    assert nan_allowed or not nan.any(), f"{what}: the restatement has NaN components outside the specials set"
    g = got.copy()
    if nan.any():
        gc = _components(g)
        assert np.isnan(gc[nan]).all(), f"{what}: {int((~np.isnan(gc[nan])).sum())} components must be NaN and are not"
        bits = np.where(nan, _components(want).view(np.uint32), gc.view(np.uint32))
        g["tsdf"].view(np.uint32)[...] = bits[:, 0]
        g["grad"].view(np.uint32)[...] = bits[:, 1:]
    a = g.view(np.uint8).reshape(len(g), -1)
    b = np.ascontiguousarray(want).view(np.uint8).reshape(len(want), -1)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(g)} records differ, the first is {int(bad[0])}: " \
                          f"{got[bad[0]]} != {want[bad[0]]}"


# ---------------------------------------------------------------------------------------------------------------------
# ESDF maps: states chosen per voxel
def state_blocks(pos, state):
    """the BlockSet of the blocks at `pos` whose voxels have the states `state` ([n, 512]): OCCUPIED is a tsdf in
    [-7/16, -0.0] (0 counts as occupied: "at or behind the surface"), FREE one in [1/16, 1/2], both with weight 1 or 2;
    UNKNOWN is weight 0 over a tsdf of -1/2, which would be occupied if the weight were not looked at"""
    pos = np.asarray(pos, dtype=np.int64).reshape(-1, 3)
    v = qc.voxel_coordinates(pos)
    h = v[..., 0] + 3 * v[..., 1] + 5 * v[..., 2]
    mag = ((h & 7).astype(np.float64) / 16).astype(F)
    tsdf = np.where(state == OCCUPIED, -mag, np.where(state == FREE, mag + F(1 / 16), F(-0.5))).astype(F)
    rgbw = np.zeros(tsdf.shape, dtype=RGBW_DTYPE)
    rgbw["r"], rgbw["g"], rgbw["b"] = (37 * v[..., 0]) & 255, (59 * v[..., 1]) & 255, (83 * v[..., 2]) & 255
    rgbw["weight"] = np.where(state == UNKNOWN, 0, 1 + ((h >> 3) & 1))
    return BlockSet(pos.astype(np.int16), tsdf, rgbw, qc.prob_of(v))


class Box(NamedTuple):
    name: str
    map: str                       # one of ESDF_MAPS
    origin: tuple
    dims: tuple
    occupied_below: float = 0.0
    unknown_occupied: bool = False
    by_hand: Callable = None       # () -> the field in closed form, where there is one

    @property
    def voxels(self):
        return int(np.prod(self.dims))


def field_of_points(dims, obstacles):
    """the field of a box whose only obstacles are the isolated voxels `obstacles` (box coordinates): the distance to
    the nearest one; an obstacle itself lies one voxel from free space, or nowhere near any if the box is all obstacle"""
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    d2 = np.min([(x - a) ** 2 + (y - b) ** 2 + (z - c) ** 2 for a, b, c in obstacles], axis=0)
    out = np.sqrt(d2.astype(F)) * F(VS)
    inside = d2 == 0
    if inside.all():
        out[...] = -INF
    else:
        for a, b, c in obstacles:       # the closed form holds when a free voxel of the box touches every obstacle
            near = [(a + d, b, c) for d in (-1, 1)] + [(a, b + d, c) for d in (-1, 1)] + [(a, b, c + d) for d in (-1, 1)]
            assert any(0 <= p < X and 0 <= q < Y and 0 <= r < Z and not inside[r, q, p] for p, q, r in near)
        out[inside] = -(np.sqrt(F(1)) * F(VS))
    return out


def field_of_solid(dims, free):
    """the field of a box that is all obstacle but the voxel `free` (None: no free voxel at all)"""
    X, Y, Z = dims
    if free is None:
        return np.full((Z, Y, X), -INF, dtype=F)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    d2 = (x - free[0]) ** 2 + (y - free[1]) ** 2 + (z - free[2]) ** 2
    out = -(np.sqrt(d2.astype(F)) * F(VS))
    out[d2 == 0] = np.sqrt(F(1)) * F(VS)
    return out


LINE_X = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024)      # both sides of one, two and sixteen waves, and the cap
LINE_YZ = (1, 2, 64, 65, 1024)
PLANE_OBSTACLES = [(0, 0, 0), (512, 512, 0)]


def _line_scenes():
    """(name, origin, dims, obstacles) of the sparse scenes, each in a region of its own (24 voxels or more apart)"""
    scenes = []
    ends = lambda n: (("first", [0]), ("last", [n - 1]), ("both", sorted({0, n - 1})))
    for i, (n, (tag, at)) in enumerate((n, e) for n in LINE_X for e in ends(n)):
        scenes.append((f"x{n}_{tag}", (-517, -20003 + 24 * i, -11), (n, 1, 1), [(a, 0, 0) for a in at]))
    for i, (n, (tag, at)) in enumerate((n, e) for n in LINE_YZ for e in ends(n)):
        scenes.append((f"y{n}_{tag}", (1003 + 24 * i, -517, 5), (8, n, 8), [(3, a, 5) for a in at]))
        scenes.append((f"z{n}_{tag}", (-2005 - 24 * i, 13, -517), (8, 8, n), [(6, 2, a) for a in at]))
    scenes.append(("plane_1024", (-517, 3003, -21), (1024, 1024, 1), PLANE_OBSTACLES))
    return scenes


@functools.lru_cache(maxsize=None)
def esdf_lines():
    """only the blocks that hold an obstacle exist; their other voxels are FREE, every fifth UNKNOWN.  The rest of
    each box lies in no block: UNKNOWN, which is no obstacle unless the flag says so."""
    obst = np.array([np.add(o, p) for _, o, _, ps in _line_scenes() for p in ps], dtype=np.int64)
    pos = np.unique(obst >> 3, axis=0)
    v = qc.voxel_coordinates(pos)
    state = np.where((v[..., 0] + v[..., 1] + v[..., 2]) % 5 == 0, UNKNOWN, FREE)
    state[np.isin(block_keys(v), block_keys(obst))] = OCCUPIED
    return Map("esdf_lines", state_blocks(pos, state), dict(block_bits=8, bucket_bits=12))


SLABS = (("slab_y", (-13, -517, 5), (8, 1024, 8), (2, 700, 6)), ("slab_z", (2003, -5, -517), (8, 8, 1024), (5, 1, 333)))


@functools.lru_cache(maxsize=None)
def esdf_slabs():
    """two slabs, all OCCUPIED inside their box but one FREE voxel each; the voxels of their blocks outside the box
    are FREE, so a transform that looked beyond the box would find them"""
    sets = []
    for _, origin, dims, free in SLABS:
        o, d = np.array(origin), np.array(dims)
        pos = qc._cube(o >> 3, ((o + d - 1) >> 3) + 1)
        v = qc.voxel_coordinates(pos)
        inside = np.all((v >= o) & (v < o + d), axis=-1) & ~np.all(v == o + np.array(free), axis=-1)
        sets.append(state_blocks(pos, np.where(inside, OCCUPIED, FREE)))
    return Map("esdf_slabs", BlockSet(*(np.concatenate([s[i] for s in sets]) for i in range(4))),
               dict(block_bits=11, bucket_bits=12))


RANDOM_BOX = ((-67, -31, -19), (130, 67, 41))      # 67 x 41 and 130 x 41 columns: no multiples of 64
RANDOM_FREE_PLANES_Z, RANDOM_FREE_PLANE_Y, RANDOM_FREE_ROWS_YZ = (7, 8, 30), 40, ((11, 3), (12, 3), (50, 20))
RANDOM_HANDFUL = 12
RANDOM_CROP = ((20, 5, 2), (12, 10, 9))            # box coordinates: z 2 .. 10 and y 5 .. 14, 1080 voxels


@functools.lru_cache(maxsize=None)
def esdf_random():
    """The blocks the box meets, 60 of them absent.  Every voxel's tsdf is its rank in a seeded permutation,
    (rank - 2^18) / 2^19 (exact, below 0.4): occupied_below = random_threshold(k) makes exactly the k lowest ranks
    obstacles -- isolated voxels scattered over the box.  Three z planes, one y plane and three x rows of the box hold
    3/4 instead and so no obstacle at any such threshold (lines with nothing on them beside lines with something); a
    handful of voxels hold 1, the only ones not OCCUPIED at occupied_below = 0.8.  3% of the rest have weight 0."""
    rng = np.random.default_rng(977)
    o, d = np.array(RANDOM_BOX[0]), np.array(RANDOM_BOX[1])
    pos = qc._cube(o >> 3, ((o + d - 1) >> 3) + 1)
    pos = pos[np.sort(rng.permutation(len(pos))[60:])]
    v = qc.voxel_coordinates(pos)
    n = v.shape[0] * 512
    assert n < 1 << 19
    tsdf = ((rng.permutation(n).astype(np.float64) - 2 ** 18) / 2 ** 19).astype(F).reshape(-1, 512)
    b = v - o                                          # box coordinates
    plain = np.isin(b[..., 2], RANDOM_FREE_PLANES_Z) | (b[..., 1] == RANDOM_FREE_PLANE_Y)
    for y, z in RANDOM_FREE_ROWS_YZ:
        plain |= (b[..., 1] == y) & (b[..., 2] == z)
    tsdf[plain] = F(0.75)
    inbox = np.flatnonzero((np.all((b >= 0) & (b < d), axis=-1) & ~plain).reshape(-1))
    tsdf.reshape(-1)[rng.choice(inbox, RANDOM_HANDFUL, replace=False)] = F(1)
    s = state_blocks(pos, np.full(tsdf.shape, FREE))
    s.rgbw["weight"] = np.where((rng.random(tsdf.shape) < 0.03) & ~plain & (tsdf < 1), 0, 1 + (tsdf > 0))
    return Map("esdf_random", BlockSet(s.pos, tsdf, s.rgbw, s.prob), dict(block_bits=10, bucket_bits=12))


def random_threshold(k):
    """occupied_below that takes the ranks 0 .. k - 1 of esdf_random"""
    return float(F((k - 0.5 - 2 ** 18) / 2 ** 19))


@functools.lru_cache(maxsize=None)
def signs_weighted():
    """`signs` with every special slot of its special block observed (weight 1 where it was 0): the NaNs, -0.0, the
    infinities and the denormals all reach the comparison with occupied_below"""
    b = signs().blocks
    rgbw = b.rgbw.copy()
    slots = sorted(qc.SPECIAL_TSDF)
    rgbw["weight"][SPECIAL_ROWS["signs"], slots] = np.maximum(rgbw["weight"][SPECIAL_ROWS["signs"], slots], 1)
    return Map("signs_weighted", BlockSet(b.pos, b.tsdf, rgbw, b.prob), signs().engine)


SPECIAL_THRESHOLDS = (("0", 0.0), ("-0", -0.0), ("denormal", DENORMAL), ("-denormal", -DENORMAL), ("inf", INF),
                      ("-inf", -INF))


# the maps by name, built when first asked for: tests parametrise over the names, so collecting them builds nothing
_BUILDERS = dict(corner_subsets=corner_subsets, signs=signs, edges=edges, tiny_table=tiny_table, known_order=known_order,
                 esdf_lines=esdf_lines, esdf_slabs=esdf_slabs, esdf_random=esdf_random, signs_weighted=signs_weighted)
SAMPLE_MAPS = ("corner_subsets", "signs", "edges", "tiny_table", "known_order")      # the maps of point_sets()
ESDF_MAPS = ("esdf_lines", "esdf_slabs", "esdf_random", "signs_weighted", "edges", "tiny_table", "known_order")


def get_map(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def boxes():
    out = []
    for name, origin, dims, obstacles in _line_scenes():
        out.append(Box(name, "esdf_lines", origin, dims,
                       by_hand=functools.partial(field_of_points, dims, tuple(obstacles))))
    for name, origin, dims, free in SLABS:
        out.append(Box(f"{name}_one_free", "esdf_slabs", origin, dims, by_hand=functools.partial(field_of_solid, dims, free)))
        # the same slab with nothing FREE: every tsdf is <= +inf
        out.append(Box(f"{name}_all_occupied", "esdf_slabs", origin, dims, INF,
                       by_hand=functools.partial(field_of_solid, dims, None)))
    n = len(esdf_random().blocks) * 512
    for tag, ob in [(f"rank_{k}", random_threshold(k)) for k in (RANDOM_HANDFUL, n // 200, n // 10, n // 2)] + \
                   [("all_but_a_handful", 0.8)]:
        for unk in (False, True):
            out.append(Box(f"random_{tag}_{'unk' if unk else 'obs'}", "esdf_random", *RANDOM_BOX, ob, unk))
    # a corner of the random box small enough for the O(n^2) definition, across two of the obstacle-free planes and
    # two of the obstacle-free rows: lines with nothing on them beside lines with something
    for unk in (False, True):
        out.append(Box(f"random_crop_{'unk' if unk else 'obs'}", "esdf_random",
                       tuple(o + c for o, c in zip(RANDOM_BOX[0], RANDOM_CROP[0])), RANDOM_CROP[1],
                       random_threshold(n // 10), unk))
    for tag, ob in SPECIAL_THRESHOLDS:
        for unk in (False, True):
            out.append(Box(f"specials_{tag}_{'unk' if unk else 'obs'}", "signs_weighted", (-19, -18, -17), (30, 29, 28),
                           ob, unk))
    for b in qc.EDGE_BLOCKS[:6]:                       # an 8^3 box on each range-end block
        out.append(Box("edge_block_%d_%d_%d" % b, "edges", tuple(8 * c for c in b), (8, 8, 8)))
    out.append(Box("edge_x_low_16", "edges", (-32768, 0, 0), (16, 8, 8)))         # block -4096, never block 4096
    out.append(Box("edge_x_low_16_unk", "edges", (-32768, 0, 0), (16, 8, 8), 0.0, True))
    out.append(Box("edge_ends_at_32767", "edges", (32756, -3, 2), (12, 13, 9)))
    out.append(Box("edge_z_ends_at_32767", "edges", (-2, 1, 32750), (11, 5, 18), 0.25, True))
    for unk in (False, True):
        tag = "unk" if unk else "obs"
        out.append(Box(f"tiny_table_{tag}", "tiny_table", (-25, -25, -25), (50, 50, 50), 0.0, unk))
        # known_order's blocks lie further apart than a box may be long: one box around the origin's five, one on
        # each of the three blocks that share a bucket, one on the far block
        out.append(Box(f"known_order_origin_{tag}", "known_order", (-10, -26, -10), (28, 44, 28), 0.0, unk))
        for b in qc.COLLISION[:3] + qc.APART[4:]:
            out.append(Box("known_order_%d_%d_%d_%s" % (b + (tag,)), "known_order",
                           tuple(max(8 * c - 1, -32768) for c in b),
                           tuple(min(8 * c + 9, 32768) - max(8 * c - 1, -32768) for c in b), 0.0, unk))
    assert len({b.name for b in out}) == len(out)
    return out


def box(name):
    return next(b for b in boxes() if b.name == name)


@functools.lru_cache(maxsize=None)
def _look(map_name):
    return Lookup(get_map(map_name).blocks)


@functools.lru_cache(maxsize=None)
def expected_state(name):
    b = box(name)
    s = box_state(get_map(b.map).blocks, b.origin, b.dims, b.occupied_below, look=_look(b.map))
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def expected_field(name):
    b = box(name)
    f = esdf_ref.esdf(expected_state(name), VS, b.unknown_occupied)
    f.setflags(write=False)
    return f


# ---------------------------------------------------------------------------------------------------------------------
# surface points on the chained directories (tests/surface_ref.py, fed from the BlockSet): (name, map, origin, dims,
# the least number of points the restatement must give).  The boxes keep clear of the special blocks: a NaN that went
# through arithmetic has no agreed bits.  known_order's blocks lie further apart than a box may be long, so it gets a
# box per cluster as for the ESDF: block (63, 171, 45) is the one found by the walk that leaves the table's end and
# wraps to entry 2, (33, 180, 42) heads that bucket; the bucket's third block, (61, 16, 170), is the special one.
SURFACE_BOXES = (("tiny_table", "tiny_table", (-25, -25, -25), (50, 50, 39), 10000),   # reads z <= 15: block (2, 2, 2) is out
                 ("known_order_origin", "known_order", (-10, -26, -10), (28, 44, 28), 300),
                 ("known_order_63_171_45", "known_order", (503, 1367, 359), (10, 10, 10), 100),
                 ("known_order_33_180_42", "known_order", (263, 1439, 335), (10, 10, 10), 100))


# ---------------------------------------------------------------------------------------------------------------------
# the WRONG variants (tests/test_readout_cases.py shows that the named sets tell each from the contract)
PERMUTATIONS = ((0, 2, 1), (1, 0, 2), (2, 1, 0), (1, 2, 0), (2, 0, 1))


class WrappedLookup(Lookup):
    """WRONG: blocks told apart by their wrapped voxel coordinates only (13 bits of the block coordinate): block 4096
    answers for voxel -32768, the later block of the list winning"""

    def __init__(self, m):
        self.m = m
        k = block_keys(m.pos.astype(np.int64) & 0x1FFF)
        self.order = np.argsort(k, kind="stable")
        self.keys = k[self.order]

    def rows(self, vox):
        k = block_keys((np.asarray(vox).astype(np.int64) >> 3) & 0x1FFF)
        at = np.maximum(np.searchsorted(self.keys, k, side="right") - 1, 0)
        return np.where(self.keys[at] == k, self.order[at], -1)


def mirrored_samples(ps):
    """WRONG: the records of a point set with the tsdf of the mirrored pairing (sample_ref.mirrored_tsdf)"""
    want = expected_samples(ps.name).copy()
    g = ps.points / F(VS)
    lookup = blockset_lookup(ps.map.blocks)
    fl = np.floor(g).astype(np.int64)
    with np.errstate(invalid="ignore"):
        t = sample_ref.mirrored_tsdf(g, lambda i, j, k: lookup(fl + np.array([i, j, k]))[1])
    ok = (want["flags"] & SAMPLE_ALLOCATED) != 0
    want["tsdf"][ok] = t[ok]
    return want


def _flush(x):
    x = np.asarray(x, dtype=F)
    return np.where(np.abs(x) < np.finfo(F).tiny, np.copysign(F(0), x), x)


WRONG_STATES = {
    "less_than": lambda t, ob: t < ob,
    "denormals_flushed": lambda t, ob: _flush(t) <= _flush(ob),
    "nan_occupied": lambda t, ob: ~(t > ob),
}


def differing(a, b):
    """how many records (rows) of two arrays differ as bytes"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    return int((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1).sum())
