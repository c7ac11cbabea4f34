"""Crafted block sets for plain map fusion (include/ratsdf_fuse.h: ratsdf_fuse_map, ratsdf_fuse_blocks,
ratsdf_fuse_blocks_device, ratsdf_fuse_map_file).  Written once, checked without a GPU in tests/test_fuse_cases.py (the
cases are not vacuous, and planted mistakes fail them) and run against the HIP engine in tests/test_gpu_fuse_cases.py.
Same role as raycast_cases.py, mesh_cases.py, query_cases.py and readout_cases.py: no GPU and no torch at import.

What is expected never comes from an engine: it is tests/fuse_ref.py (the numpy restatement of the header) applied to
the crafted inputs.  Both maps of a case go into their engines with import_blocks, so every voxel word is known.

Voxel cases (`VOXEL_CASES`): a pair of voxel rows (a = destination, b = source) laid into blocks at the same
positions on both sides; every voxel of the destination meets the voxel of the same index of the source.
  colours        every (numerator, weight sum) of the colour quotient that two maps built from frames can produce
                 (weights 1 .. 40), and the rounding ties with their neighbours at the weights only an imported map
                 holds (sums 82 .. 510)
  tsdf           signed zeros, subnormals, values outside [-1, 1], overflow of the weighted sum, infinities and NaN
                 crossed with weights 1 .. 255, and a block of random bit patterns
  edges          contributes() on both sides: weight 0, weight 1 at -1.0 and its two neighbouring bit patterns, -1.0 at
                 weights 2 and 255, and the hand-worked rows of test_fuse_ref.CASES
  patterns       whole blocks copied / averaged / untouched, one lane's eight voxels, one voxel per lane
  prob_grid      probabilities from FLT_MIN to the predecessor of 1 crossed with weights 1 .. 255
  prob_special   0, 1, -0.0, NaN, +-inf, 2.0 and -0.5 on either side, in all pairings
  prob_subnormal subnormal probabilities (kept apart: the hardware's log2 reads a subnormal input as zero)

Block-list cases (functions below): long_list, short_lists, passes_run_out, chained, positions_and_shards.

The mistakes of `MISTAKES` are single wrong lines planted in a copy of the restatement; `failing_cases` says which
cases tell each of them from the right one.
"""
import functools
from typing import NamedTuple

import numpy as np

import fuse_ref
from fuse_ref import F
from ratsdf._abi import RGBW_DTYPE

U32 = np.uint32
FLT_MIN = float(U32(0x00800000).view(F))
FLT_MAX = float(np.finfo(F).max)
DENORM_MIN = float(U32(1).view(F))           # the smallest positive subnormal
DENORM_MAX = float(U32(0x007FFFFF).view(F))  # the largest subnormal
NAN, INF = float("nan"), float("inf")
FORMS = ("map", "blocks", "blocks_device", "file")
TRUNC, VS = 0.06, 0.01
CHUNK_FUSE = 16384   # blocks per allocation pass (kFuseChunk)
CHUNK_STAGE = 2048   # blocks per staging chunk of the host and file forms (kMapChunk)
WAVES = 8192         # waves of the largest k_fuse_blocks grid: a chunk with more blocks makes waves stride
N_LONG = CHUNK_FUSE + CHUNK_STAGE + 37
N_STAGED = 2 * CHUNK_STAGE + 37


class Voxels(NamedTuple):
    t: np.ndarray  # [n] float32
    c: np.ndarray  # [n] RGBW_DTYPE
    p: np.ndarray  # [n] float32


class VoxelCase(NamedTuple):
    name: str
    a: Voxels      # destination rows
    b: Voxels      # source rows


def voxels(n, t=0.0, rgb=(0, 0, 0), w=0, p=0.5):
    c = np.zeros(n, dtype=RGBW_DTYPE)
    c["r"], c["g"], c["b"], c["weight"] = rgb[0], rgb[1], rgb[2], w
    return Voxels(np.full(n, t, dtype=F), c, np.full(n, p, dtype=F))


def rows(items):
    """[(tsdf, (r, g, b, weight), prob), ...] -> Voxels; a tsdf given as an int is a bit pattern"""
    t = np.array([U32(r[0]).view(F) if isinstance(r[0], (int, np.integer)) else F(r[0]) for r in items], dtype=F)
    return Voxels(t, np.array([r[1] for r in items], dtype=RGBW_DTYPE), np.array([r[2] for r in items], dtype=F))


def concat(parts):
    return Voxels(*(np.concatenate([q[i] for q in parts]) for i in range(3)))


def cross(a, b):
    """every row of a against every row of b"""
    ia, ib = (v.reshape(-1) for v in np.meshgrid(np.arange(len(a.t)), np.arange(len(b.t)), indexing="ij"))
    return Voxels(*(v[ia] for v in a)), Voxels(*(v[ib] for v in b))


# ---------------------------------------------------------------------------------------------------------------------
# colours
@functools.lru_cache(maxsize=None)
def colour_pairs_from_frames():
    """every (num, wc) that ca, cb in 0 .. 255 and wa, wb in 1 .. 40 realise, with one realisation each:
    int64 arrays num, wc, ca, cb, wa, wb (wa <= wb: the sets of (wa, wb) and (wb, wa) are the same)"""
    code = np.full((81, 255 * 80 + 1), -1, dtype=np.int64)
    ca, cb = (v.reshape(-1) for v in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    for wa in range(1, 41):
        for wb in range(wa, 41):
            code[wa + wb, ca * wa + cb * wb] = ca | cb << 8 | wa << 16 | wb << 24
    wc, num = np.nonzero(code >= 0)
    k = code[wc, num]
    return num, wc, k & 255, k >> 8 & 255, k >> 16 & 255, k >> 24


@functools.lru_cache(maxsize=None)
def colour_ties():
    """for every even wc in 82 .. 510 and k in 0 .. 254: num = (k + 1/2) wc and num +- 1, those that some ca, cb <= 255
    and wa, wb in 1 .. 255 realise.  Same arrays as colour_pairs_from_frames, and `tie` (bool)."""
    out = []
    cas = np.arange(256)
    for wc in range(82, 511, 2):
        tie = np.arange(255) * wc + wc // 2
        nums = np.concatenate([tie - 1, tie, tie + 1])
        is_tie = np.concatenate([np.zeros(255, bool), np.ones(255, bool), np.zeros(255, bool)])
        todo = np.arange(len(nums))
        for wa in range(max(1, wc - 255), wc // 2 + 1):
            wb = wc - wa
            rem = nums[todo, None] - cas[None, :] * wa
            ok = (rem >= 0) & (rem % wb == 0) & (rem // wb <= 255)
            has, ca = ok.any(axis=1), ok.argmax(axis=1)
            i = todo[has]
            out.append(np.stack([nums[i], np.full(len(i), wc), ca[has], (nums[i] - ca[has] * wa) // wb,
                                 np.full(len(i), wa), np.full(len(i), wb), is_tie[i]], axis=1))
            todo = todo[~has]
            if not len(todo):
                break
    r = np.concatenate(out).astype(np.int64)
    return tuple(r[:, j] for j in range(6)) + (r[:, 6].astype(bool),)


def colours_case():
    """three (ca, cb) of one (wa, wb) per voxel; every second voxel with the two sides exchanged"""
    f, t = colour_pairs_from_frames(), colour_ties()
    ca, cb, wa, wb = (np.concatenate([f[j], t[j]]) for j in (2, 3, 4, 5))
    order = np.argsort(wa * 256 + wb, kind="stable")
    ca, cb, wa, wb = (v[order] for v in (ca, cb, wa, wb))
    # groups of equal (wa, wb), each padded to a multiple of three by repeating its last entry
    key = wa * 256 + wb
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    ends = np.r_[starts[1:], len(key)]
    take = np.concatenate([np.r_[np.arange(s, e), np.full((-(e - s)) % 3, e - 1, dtype=np.int64)]
                           for s, e in zip(starts, ends)])
    ca, cb, wa, wb = (v[take].reshape(-1, 3) for v in (ca, cb, wa, wb))
    n = len(ca)
    a, b = voxels(n, t=0.25, p=0.5), voxels(n, t=-0.5, p=0.5)
    swap = (np.arange(n) & 1) == 1
    for j, ch in enumerate(("r", "g", "b")):
        a.c[ch][:] = np.where(swap, cb[:, j], ca[:, j])
        b.c[ch][:] = np.where(swap, ca[:, j], cb[:, j])
    a.c["weight"][:] = np.where(swap, wb[:, 0], wa[:, 0])
    b.c["weight"][:] = np.where(swap, wa[:, 0], wb[:, 0])
    return VoxelCase("colours", a, b)


def colour_quotients(a, b):
    """(num, wc) of every channel of every voxel pair, exact integers: [n, 3] and [n]"""
    wa, wb = a.c["weight"].astype(np.int64), b.c["weight"].astype(np.int64)
    num = np.stack([a.c[ch].astype(np.int64) * wa + b.c[ch].astype(np.int64) * wb for ch in ("r", "g", "b")], axis=1)
    return num, wa + wb


# ---------------------------------------------------------------------------------------------------------------------
# tsdf
TSDF_VALUES = (0.0, -0.0, DENORM_MIN, -DENORM_MIN, 1e-39, FLT_MIN, 0.3, -0.7, 1.0, -1.0, 1.5, -3.0, 1e30, FLT_MAX,
               -FLT_MAX, INF, -INF, NAN)
TSDF_WEIGHTS = (1, 2, 39, 40, 41, 255)


def tsdf_case():
    side = lambda rgb, p: rows([(t, (*rgb, w), p) for t in TSDF_VALUES for w in TSDF_WEIGHTS])
    a, b = cross(side((10, 200, 77), 0.3), side((250, 3, 78), 0.6))
    # ... and one block of random bit patterns on both sides
    rng = np.random.default_rng(71)
    ra, rb = voxels(512), voxels(512)
    for v in (ra, rb):
        v.t.view(U32)[:] = rng.integers(0, 1 << 32, 512, dtype=np.uint64).astype(U32)
        for ch in ("r", "g", "b"):
            v.c[ch][:] = rng.integers(0, 256, 512)
        v.c["weight"][:] = rng.integers(1, 256, 512)
        v.p[:] = rng.uniform(0.02, 0.98, 512)
    return VoxelCase("tsdf", concat([a, ra]), concat([b, rb]))


# ---------------------------------------------------------------------------------------------------------------------
# contributes()
FRESH = fuse_ref.FRESH_TSDF_BITS


def edge_rows(rgb, p):
    return [(0.3, (*rgb, 0), p), (-1.0, (*rgb, 0), p),                       # weight 0 with any tsdf
            (FRESH, (*rgb, 1), p), (FRESH - 1, (*rgb, 1), p), (FRESH + 1, (*rgb, 1), p),
            (-1.0, (*rgb, 2), p), (-1.0, (*rgb, 255), p),                    # -1.0 is fresh at weight 1 only
            (0.5, (*rgb, 1), p), (0.5, (*rgb, 5), p), (-0.25, (*rgb, 40), p)]


def edges_case():
    from test_fuse_ref import CASES
    a, b = cross(rows(edge_rows((11, 22, 33), 0.7)), rows(edge_rows((201, 202, 203), 0.2)))
    return VoxelCase("edges", concat([a, rows([c[0] for c in CASES])]), concat([b, rows([c[1] for c in CASES])]))


# ---------------------------------------------------------------------------------------------------------------------
# whole blocks and whole lanes (a lane of k_fuse_blocks owns voxels 8l .. 8l + 7 and writes nothing if none changed)
LIVE_A, LIVE_B = (0.5, (10, 20, 30, 7), 0.7), (-0.25, (50, 60, 70, 3), 0.4)
FRESH_A, DEAD_B = (-1.0, (4, 5, 6, 1), 0.5), (0.3, (9, 9, 9, 0), 0.9)
PATTERN_BLOCKS = ("all copied", "all averaged", "nothing contributes", "one lane", "one voxel per lane")


def patterns_case():
    i = np.arange(512)
    one_lane = (i >> 3) == 37
    per_lane = (i & 7) == ((i >> 3) % 8)  # lane l changes its voxel l mod 8
    pick = lambda mask, yes, no: rows([yes if m else no for m in mask])
    a = [rows([FRESH_A] * 512), rows([LIVE_A] * 512), rows([LIVE_A] * 512), rows([LIVE_A] * 512),
         pick((i & 8) != 0, FRESH_A, LIVE_A)]  # (odd lanes copy, even lanes average)
    b = [rows([LIVE_B] * 512), rows([LIVE_B] * 512), rows([DEAD_B] * 512), pick(one_lane, LIVE_B, DEAD_B),
         pick(per_lane, LIVE_B, DEAD_B)]
    # (distinct voxels inside a block: a lane that wrote its neighbour's words would show)
    for k, v in enumerate(a + b):
        v.c["g"][:] = (i + 17 * k) & 255
        v.t[v.c["weight"] > 1] += (i[v.c["weight"] > 1] * F(2.0 ** -11)).astype(F)
    return VoxelCase("patterns", concat(a), concat(b))


# ---------------------------------------------------------------------------------------------------------------------
# probabilities
def _next(x, to):
    return float(np.nextafter(F(x), F(to)))


PROB_GRID = (FLT_MIN, 1e-30, 1e-20, 1e-10, 1e-6, 1e-3, 0.02, 0.25, 0.5, _next(0.5, 1), 0.75, 0.98, 1 - 1e-3, 1 - 1e-6,
             _next(1, 0))
PROB_WEIGHTS = (1, 2, 3, 7, 20, 39, 40, 41, 100, 255)
PROB_SPECIAL = (0.0, 1.0, -0.0, NAN, INF, -INF, 2.0, -0.5)
PROB_SUBNORMAL = (DENORM_MIN, 1e-40, DENORM_MAX)


def prob_grid_case():
    side = lambda t, rgb: rows([(t, (*rgb, w), p) for p in PROB_GRID for w in PROB_WEIGHTS])
    return VoxelCase("prob_grid", *cross(side(0.25, (1, 2, 3)), side(-0.5, (4, 5, 6))))


def _paired(ps_a, ps_b, weights, both_orders=True):
    a, b = [], []
    for pa in ps_a:
        for pb in ps_b:
            for wa, wb in weights:
                for x, y in (((pa, wa), (pb, wb)), ((pb, wb), (pa, wa)))[:2 if both_orders else 1]:
                    a.append((0.25, (1, 2, 3, x[1]), x[0]))
                    b.append((-0.5, (4, 5, 6, y[1]), y[0]))
    return rows(a), rows(b)


def prob_special_case():
    every = PROB_SPECIAL + (0.5, 0.3, 0.9)
    return VoxelCase("prob_special", *_paired(PROB_SPECIAL, every, ((2, 2), (1, 3), (40, 1))))


def prob_subnormal_case():
    return VoxelCase("prob_subnormal", *_paired(PROB_SUBNORMAL, (0.5, 1.0) + PROB_SUBNORMAL, ((1, 39), (1, 1), (3, 5))))


def prob_float64(a, b):
    """the header's probability line in float64 on the float32 inputs (NaN where undefined)"""
    wa, wb = a.c["weight"].astype(np.float64), b.c["weight"].astype(np.float64)
    pa, pb = a.p.astype(np.float64), b.p.astype(np.float64)
    with np.errstate(all="ignore"):
        x = (wa * np.log(pa / (1 - pa)) + wb * np.log(pb / (1 - pb))) / (wa + wb)
        return 1 / (1 + np.exp(-x))


VOXEL_CASE_BUILDERS = dict(colours=colours_case, tsdf=tsdf_case, edges=edges_case, patterns=patterns_case,
                           prob_grid=prob_grid_case, prob_special=prob_special_case, prob_subnormal=prob_subnormal_case)
VOXEL_CASES = tuple(VOXEL_CASE_BUILDERS)


@functools.lru_cache(maxsize=None)
def voxel_case(name):
    return VOXEL_CASE_BUILDERS[name]()


# the padding of a case's last block: the source does not contribute, the destination keeps a known voxel
PAD_A, PAD_B = (0.125, (1, 2, 3, 5), 0.5), DEAD_B


def case_positions(n_blocks, seed):
    """n distinct block positions around the origin (both signs on every axis), in a seeded order"""
    side = 2
    while (2 * side) ** 3 < n_blocks:
        side += 1
    r = np.arange(-side, side)
    x, y, z = (v.reshape(-1) for v in np.meshgrid(r, r, r, indexing="ij"))
    pos = np.stack([x, y, z], axis=1).astype(np.int16)
    return pos[np.random.default_rng(seed).permutation(len(pos))[:n_blocks]]


def as_block_sets(case, seed=3):
    """(destination set, source set) of a voxel case: the rows in blocks of 512 at the same positions on both sides"""
    n = len(case.a.t)
    nb = -(-n // 512)
    pad = nb * 512 - n
    a, b = concat([case.a, rows([PAD_A] * pad)]), concat([case.b, rows([PAD_B] * pad)])
    pos = case_positions(nb, seed)
    return tuple((pos.copy(),) + tuple(v.reshape(nb, 512) for v in s) for s in (a, b))


# ---------------------------------------------------------------------------------------------------------------------
# block lists
def craft(positions, seed, weight_hi=40):
    """blocks with random tsdf in [-1, 1], weights 0 .. weight_hi (zeros and fresh voxels among them), random colour
    and probability -- as tests/test_gpu_resample.py crafts its maps"""
    rng = np.random.default_rng(seed)
    n = len(positions)
    t = rng.uniform(-1, 1, (n, 512)).astype(F)
    c = np.zeros((n, 512), dtype=RGBW_DTYPE)
    for ch in ("r", "g", "b"):
        c[ch] = rng.integers(0, 256, (n, 512))
    c["weight"] = rng.integers(0, weight_hi + 1, (n, 512))
    fresh = rng.random((n, 512)) < 0.08
    t[fresh], c["weight"][fresh] = F(-1), 1
    p = rng.uniform(0.02, 0.98, (n, 512)).astype(F)
    return np.array(positions, dtype=np.int16).reshape(-1, 3), t, c, p


def subset(s, sel):
    return tuple(v[sel] for v in s)


def home_buckets(pos, bucket_bits):
    """the directory's home bucket of block positions (block_hash of device_math.h)"""
    p = np.asarray(pos).astype(np.int64).astype(U32)  # two's complement, as the engine's (uint32_t)x
    with np.errstate(over="ignore"):
        h = (p[:, 0] * U32(73856093)) ^ (p[:, 1] * U32(19349669)) ^ (p[:, 2] * U32(83492791))
    return h & U32((1 << bucket_bits) - 1)


class ListCase(NamedTuple):
    dst: tuple
    src: tuple
    extra: dict


@functools.lru_cache(maxsize=None)
def long_list():
    """N_LONG source blocks: more than the 8 192 waves of a launch (waves stride) and more than one chunk of 16 384
    (a second chunk of 2 085).  The destination holds every other source position with other voxels, and five blocks
    of its own.  `staged`: the first N_STAGED blocks for the host and file forms (two staging chunks and a short
    third), against the destination restricted to those positions."""
    pos = case_positions(N_LONG, seed=5)
    src = craft(pos, seed=51)
    own = np.array([(60, 61, 62 + i) for i in range(5)], dtype=np.int16)
    dst = craft(np.concatenate([pos[::2], own]), seed=52)
    head = subset(src, slice(0, N_STAGED))
    dst_head = subset(dst, np.isin(fuse_ref.keys(dst[0]), fuse_ref.keys(head[0])) | (np.arange(len(dst[0])) >= len(pos[::2])))
    return ListCase(dst, src, dict(staged=ListCase(dst_head, head, {})))


def colliders(bucket_bits, k, avoid=(), span=24, seed=0):
    """k positions that share one home bucket of a 2^bucket_bits directory (brute force over a cube of positions), the
    bucket being none of `avoid`"""
    r = np.arange(-span, span)
    x, y, z = (v.reshape(-1) for v in np.meshgrid(r, r, r, indexing="ij"))
    pos = np.stack([x, y, z], axis=1).astype(np.int16)
    pos = pos[np.random.default_rng(seed).permutation(len(pos))]
    h = home_buckets(pos, bucket_bits)
    for bucket in np.unique(h):
        if int(bucket) in avoid:
            continue
        hit = pos[h == bucket]
        if len(hit) >= k:
            return hit[:k], int(bucket)
    raise AssertionError("no bucket with that many positions")


def distinct_homes(bucket_bits, n, avoid, span=24, seed=1):
    """n positions with n different home buckets, none of them in `avoid`"""
    r = np.arange(-span, span)
    x, y, z = (v.reshape(-1) for v in np.meshgrid(r, r, r, indexing="ij"))
    pos = np.stack([x, y, z], axis=1).astype(np.int16)
    pos = pos[np.random.default_rng(seed).permutation(len(pos))]
    h = home_buckets(pos, bucket_bits)
    _, first = np.unique(h, return_index=True)
    first = np.sort(first)
    first = first[~np.isin(h[first], list(avoid))][:n]
    assert len(first) == n
    return pos[first]


SHORT_LISTS = (1, 31, 32, 33)
SHORT_SHARD = (0, 2, 1)  # the destination owns every other pair of bx: refused blocks sit between the others


@functools.lru_cache(maxsize=None)
def short_lists():
    """lists of 1, 31, 32 and 33 blocks for a destination with 512 buckets and the shard filter SHORT_SHARD.  The
    positions come in fours that share a home bucket, three of them owned (so a call makes three passes and the done bits of the first
    pass are what keeps the later ones from fusing again), one of them refused (the 32 blocks of a `done` word
    hold fused and refused ones).  The destination holds every fourth owned position."""
    out = {}
    used = set()
    groups = []
    for g in range(9):
        while True:
            hit, bucket = colliders(9, 12, avoid=used, seed=100 + g)
            used.add(bucket)
            own = fuse_ref.shard_owned(hit, *SHORT_SHARD)
            even, odd = hit[own], hit[~own]
            if len(even) >= 3 and len(odd) >= 1:
                break
        groups.append(np.concatenate([even[:1], odd[:1], even[1:3]]))
    pos = np.concatenate(groups)  # owned, refused, owned, owned | owned, refused, ...
    for n in SHORT_LISTS:
        src = craft(pos[:n], seed=60 + n)
        owned = np.flatnonzero(fuse_ref.shard_owned(pos[:n], *SHORT_SHARD))
        dst = craft(np.concatenate([pos[:n][owned[::4]], np.array([(70, 70, 70)], dtype=np.int16)]), seed=160 + n)
        out[n] = ListCase(dst, src, {})
    return out


PASSES = 8  # allocation passes of a chunk (kFusePasses)


@functools.lru_cache(maxsize=None)
def passes_run_out(k=11, others=40, held=24):
    """a source whose k new blocks share one home bucket of the destination's 512-bucket directory: an allocation pass
    places one block per home bucket, so k - 8 of them are still without a place after 8 passes.  With them: `others`
    new blocks, each alone in its home bucket, and `held` blocks the destination already has (alone in theirs)."""
    col, bucket = colliders(9, k, seed=7)
    rest = distinct_homes(9, others + held, avoid={bucket}, seed=8)
    rest = rest[~np.isin(fuse_ref.keys(rest), fuse_ref.keys(col))]
    new, there = rest[:others], rest[others:]
    order = np.random.default_rng(9).permutation(k + len(rest))
    src = craft(np.concatenate([col, new, there])[order], seed=71)
    dst = craft(np.concatenate([there, np.array([(80, 80, 80)], dtype=np.int16)]), seed=72)
    return ListCase(dst, src, dict(colliders=col, others=new, held=there, bucket=bucket))


@functools.lru_cache(maxsize=None)
def chained(n=700):
    """about 700 blocks for a source AND a destination directory of 512 buckets: most blocks hang on a chain on both
    sides.  No home bucket is shared by more than 8 positions, so import_blocks (8 passes) places them all."""
    for seed in range(200, 260):
        pos = case_positions(n, seed)
        if np.unique(home_buckets(pos, 9), return_counts=True)[1].max() <= PASSES:
            break
    else:
        raise AssertionError("no seed gives at most 8 per bucket")
    src = craft(pos, seed=81)
    dst = craft(pos[::2], seed=82)
    return ListCase(dst, src, dict(seed=seed))


SHARD_SETTINGS = tuple((r, 3, s) for s in (0, 1, 2) for r in range(3))


def effective_shard(shard):
    """the setting as the engine reads it: shard_slab_bits 0 selects the default, 2 (ratsdf.h), like block_bits 0"""
    return shard[0], shard[1], shard[2] if shard[2] > 0 else 2



@functools.lru_cache(maxsize=None)
def positions_and_shards():
    """blocks at the ends of the int16 voxel range (block coordinates -4096 and 4095) on every axis and at mixed signs;
    bx on both sides of 0 and around multiples of 2 and 4 (slabs of 2 and 4 blocks), for the biased floor-mod of shard_owned"""
    xs = (-4096, -4095, -4093, -4092, -4091, -13, -12, -9, -8, -7, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 7, 8, 9, 11,
          12, 13, 4091, 4092, 4093, 4095)
    yz = ((0, 0), (-4096, 4095), (4095, -4096), (-1, 7), (5, -3))
    pos = np.array([(x, y, z) for x in xs for (y, z) in yz] + [(-4096, -4096, -4096), (4095, 4095, 4095)], dtype=np.int16)
    pos = pos[np.random.default_rng(13).permutation(len(pos))]
    src = craft(pos, seed=91)
    dst = craft(pos[::2], seed=92)
    return ListCase(dst, src, {})


# ---------------------------------------------------------------------------------------------------------------------
# planted mistakes: each is the restatement with ONE line wrong
def _fuse_voxels_with(at, ac, ap, bt, bc, bp, contributes=fuse_ref.contributes, rounding="away", cap=40,
                      copy_keeps_colour=False, swap_weights=False):
    """fuse_ref.fuse_voxels with switches for the wrong lines"""
    at, bt, ap, bp = (np.asarray(v, dtype=F) for v in (at, bt, ap, bp))
    cb, ca = contributes(bt, bc), contributes(at, ac)
    copied, averaged = cb & ~ca, cb & ca
    wa, wb = ac["weight"].astype(F), bc["weight"].astype(F)
    wc = wa + wb
    with np.errstate(all="ignore"):
        t = (at * wb + bt * wa) / wc if swap_weights else (at * wa + bt * wb) / wc
        col = {}
        for ch in ("r", "g", "b"):
            q = (ac[ch].astype(F) * wa + bc[ch].astype(F) * wb) / wc
            q = np.where(averaged, q, F(0)).astype(np.float64)
            col[ch] = {"away": np.floor(q + 0.5), "even": np.rint(q), "truncate": np.floor(q)}[rounding].astype(np.uint8)
        w = np.minimum(wc, F(cap)).astype(np.uint8)
        x = (wa * fuse_ref.logit(ap) + wb * fuse_ref.logit(bp)) / wc
        p = F(1) / (F(1) + np.exp(-x, dtype=F))
    ot, oc, op = at.copy(), ac.copy(), ap.copy()
    ot[copied], oc[copied], op[copied] = bt[copied], bc[copied], bp[copied]
    if copy_keeps_colour:
        for ch in ("r", "g", "b"):
            oc[ch][copied] = ac[ch][copied]
    ot[averaged], op[averaged] = t[averaged], p[averaged]
    for ch in ("r", "g", "b"):
        oc[ch][averaged] = col[ch][averaged]
    oc["weight"][averaged] = w[averaged]
    return ot, oc, op, copied, averaged


def _bits(t):
    return np.ascontiguousarray(t, dtype=F).view(U32)


VOXEL_MISTAKES = {
    "colours rounded half to even": dict(rounding="even"),
    "colours truncated": dict(rounding="truncate"),
    "the weight cap at 41": dict(cap=41),
    "fresh decided by weight 1 alone": dict(contributes=lambda t, c: c["weight"] > 1),
    "fresh decided by tsdf == -1.0 at any weight":
        dict(contributes=lambda t, c: (c["weight"] != 0) & (_bits(t) != FRESH)),
    "a copy keeps the destination's colour": dict(copy_keeps_colour=True),
    "wa and wb swapped in the tsdf": dict(swap_weights=True),
}
LIST_MISTAKES = ("a block fused twice", "the second chunk read from the first chunk's offsets",
                 "C remainder instead of floor-mod in the shard rule")
MISTAKES = tuple(VOXEL_MISTAKES) + LIST_MISTAKES


def same_voxels(x, y):
    """two results of fuse_voxels agree as the GPU test compares them: tsdf bit for bit (NaN against NaN), colour and
    weight exactly, the probability NaN in the same places and within parity's 1e-4, the branch masks equal"""
    nt = np.isnan(y[0])
    if not (np.array_equal(np.isnan(x[0]), nt) and np.array_equal(_bits(x[0])[~nt], _bits(y[0])[~nt])):
        return False
    if not (np.array_equal(x[1], y[1]) and np.array_equal(x[3], y[3]) and np.array_equal(x[4], y[4])):
        return False
    npb = np.isnan(y[2])
    return np.array_equal(np.isnan(x[2]), npb) and bool(np.all(np.abs(x[2][~npb] - y[2][~npb]) <= 1e-4))


def same_sets(x, y):
    gx, gy = fuse_ref.by_position(x), fuse_ref.by_position(y)
    if len(gx[0]) != len(gy[0]) or not np.array_equal(gx[0], gy[0]):
        return False
    known = fuse_ref.contributes(gy[1], gy[2])
    return (np.array_equal(_bits(gx[1]), _bits(gy[1])) and np.array_equal(gx[2]["weight"], gy[2]["weight"])
            and np.array_equal(gx[2][known], gy[2][known]) and bool(np.all(np.abs(gx[3] - gy[3]) <= 1e-4)))


def fuse_twice(dst, src, shard=None, every=7):
    """WRONG: every `every`-th block of the list is fused a second time"""
    out, _ = fuse_ref.fuse(dst, src, shard)
    again, _ = fuse_ref.fuse(out, subset(src, slice(0, None, every)), shard)
    return again


def fuse_first_chunk_offsets(dst, src, chunk):
    """WRONG: the blocks of the second and later chunks take their voxels from the first chunk's rows"""
    i = np.arange(len(src[0]))
    j = np.where(i >= chunk, i % chunk, i)
    return fuse_ref.fuse(dst, (src[0],) + tuple(v[j] for v in src[1:]))[0]


def shard_owned_c_remainder(pos, shard_rank, shard_count, slab_bits):
    """WRONG: C's % (truncating) instead of floor-mod"""
    s = np.asarray(pos)[:, 0].astype(np.int64) >> slab_bits
    return np.fmod(s, shard_count) == shard_rank


def failing_cases(mistake):
    """the names of the cases whose expected result differs under `mistake`"""
    out = []
    if mistake in VOXEL_MISTAKES:
        for name in VOXEL_CASES:
            c = voxel_case(name)
            right = fuse_ref.fuse_voxels(*c.a, *c.b)
            wrong = _fuse_voxels_with(*c.a, *c.b, **VOXEL_MISTAKES[mistake])
            if not same_voxels(wrong, right):
                out.append(name)
    elif mistake == "a block fused twice":
        for n, c in short_lists().items():
            if not same_sets(fuse_twice(c.dst, c.src, SHORT_SHARD), fuse_ref.fuse(c.dst, c.src, SHORT_SHARD)[0]):
                out.append(f"short_lists[{n}]")
        for name, c in (("chained", chained()), ("passes_run_out", passes_run_out())):
            if not same_sets(fuse_twice(c.dst, c.src), fuse_ref.fuse(c.dst, c.src)[0]):
                out.append(name)
    elif mistake == "the second chunk read from the first chunk's offsets":
        c = long_list().extra["staged"]
        if not same_sets(fuse_first_chunk_offsets(c.dst, c.src, CHUNK_STAGE), fuse_ref.fuse(c.dst, c.src)[0]):
            out.append("long_list[staged]")
        # (the whole list against kFuseChunk: the tail alone, the first chunk is the same either way)
        c = long_list()
        tail = np.arange(CHUNK_FUSE, N_LONG)
        wrong = (c.src[0][tail],) + tuple(v[tail - CHUNK_FUSE] for v in c.src[1:])
        if not same_sets(fuse_ref.fuse(c.dst, wrong)[0], fuse_ref.fuse(c.dst, subset(c.src, tail))[0]):
            out.append("long_list")
    elif mistake == "C remainder instead of floor-mod in the shard rule":
        c = positions_and_shards()
        for shard in SHARD_SETTINGS:
            shard = effective_shard(shard)
            if not np.array_equal(shard_owned_c_remainder(c.src[0], *shard), fuse_ref.shard_owned(c.src[0], *shard)):
                out.append(f"positions_and_shards{list(shard)}")
    else:
        raise KeyError(mistake)
    return out
