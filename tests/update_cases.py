"""Crafted prior voxels and frames for the frame update (k_integrate: integrate_block / finish_block in
ra-slam_amd/csrc/kernels_integrate.h; the oracle's integrate_block).  Written once, checked without a GPU in
tests/test_update_cases.py (the cases hold what they are for, and the oracle follows the reference's formula) and run
against the HIP engine in tests/test_gpu_update_cases.py and, at one voxel per lane, in tests/diagnostic_build_cases.py.
Same role as fuse_cases.py and resample_cases.py: no engine, no GPU and no torch at import.

Geometry: voxels of 2 cm, truncation 6 voxels, max depth 4 m, identity pose, 160 x 120 images with fx = fy = 140, so
that x-adjacent voxels at 0.8 .. 1.28 m lie 2.2 .. 3.5 pixels apart.  A case imports 62 blocks: a slab of 4 x 4 x 3
pool blocks at z = 0.8 .. 1.28 m and 14 carve blocks to its left, where every frame's depth is 0 (visible, never
updated: the carve predicate is taken on the priors alone).  (The pool `far` has 16 blocks astride z = 4 m instead of
the slab: its frame 0 stands at max_depth, before and behind them.)  Three frames follow:
  frame 0   depth only in a window whose rays stay inside the slab (no block is allocated: every visible block is an
            imported one, and the restated update mask can be counted against updated_voxels); rows 21 .. 59 a wall at
            1 m with a one-pixel checkerboard of holes, rows 60 .. 96 the wall without holes
  frame 1   the whole width right of the carve columns: a wall at 1.06 m with the other checkerboard, a wall at 1.3 m
            (past the slab: fresh blocks are allocated and updated beside the imported ones in one launch) and, in rows
            90 .. 119, depth == max_depth (w_new = 0) and its float predecessor (w_new ~ 2.4e-7) in stripes
  frame 2   walls at 0.95 m and 0.9 m (checkerboard), the far stripes exchanged
Colours come in bands of four rows (0, 255, random); ht / lt are ordinary (lt = 1 - ht) with column stripes of
(0, 1), (1, 0) and a few tiles of (0, 0).

The prior of a case is a table of entries laid over the pool voxels: the voxels are sorted into eight strata (updates
in frame 0 or not, its lane partner (voxel index ^ 1, the x-neighbour 2k / 2k + 1 of the packed path) updates or not,
even or odd x), each stratum is permuted by a seeded generator and the entries are dealt round it.  Every entry then
sits on updating and idle voxels, beside updating and idle partners, on even and odd x; `occurrences` counts it.

The numpy restatement here is float32 operation by operation (identity rotation: the quaternion terms vanish), the
pixel pick with round-half-away: `predict` gives the update mask and each updating voxel's pixel, ts and w_new.
"""
import functools
from typing import NamedTuple

import numpy as np

from ratsdf._abi import RGBW_DTYPE

F, U32 = np.float32, np.uint32
VS, MD, W, H = 0.02, 4.0, 160, 120
TRUNC = 6 * VS
FX, CX, CY = 140.0, 80.0, 60.0
INTR, POSE = (FX, FX, CX, CY), (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
CARVE_COLS = 60                      # depth is 0 in columns 0 .. 59 of every frame
WINDOW = (62, 136, 21, 97)           # u0, u1, v0, v1 of frame 0: rays that stay inside the slab
CFG = dict(block_bits=12, bucket_bits=12)

FLT_MIN = float(U32(0x00800000).view(F))
FLT_MAX = float(np.finfo(F).max)
DENORM_MIN = float(U32(1).view(F))
DENORM_MAX = float(U32(0x007FFFFF).view(F))
MD_PRED = float(np.nextafter(F(MD), F(0)))


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(U32)


def fbits(word):
    return U32(word).view(F)


def _next(x, to):
    return F(np.nextafter(F(x), F(to)))


# ---------------------------------------------------------------------------------------------------------------------
# block positions
POOL_POS = np.array([(x, y, z) for z in (5, 6, 7) for y in (-2, -1, 0, 1) for x in (-1, 0, 1, 2)], dtype=np.int16)
# the far pool: blocks astride z = max_depth on the optical axis' right, inside frame 0's window
FAR_POS = np.array([(x, y, z) for z in (24, 25) for y in (-1, 0) for x in (0, 1, 2, 3)], dtype=np.int16)
_CARVE_AT = [(x, y, z) for z in (5, 6) for y in (-2, -1, 0, 1) for x in (-3, -2)]
SINGLE_LOW_AT = (0, 1, 130, 260, 390, 511)  # each of a block's four waves of 128 voxels, first and second voxel of a lane


# ---------------------------------------------------------------------------------------------------------------------
# frames
class Frame(NamedTuple):
    rgb: np.ndarray
    depth: np.ndarray
    ht: object
    lt: object

    def args(self):
        return (self.rgb, self.depth, self.ht, self.lt, MD, INTR, POSE)


def _far(u):
    """depth == max_depth in the even four-column stripes, its predecessor in the odd ones"""
    return np.where((u // 4) % 2 == 0, F(MD), F(MD_PRED)).astype(F)


@functools.lru_cache(maxsize=None)
def frame(i, far0=False, holes_b=False, semantic=True):
    """frame i (0, 1, 2) of a case.  far0: frame 0's walls stand at max_depth / its predecessor instead of 1 m;
    holes_b: frame 0's second wall has the checkerboard too; semantic=False: a TSDF-only frame (ht = lt = None)"""
    rng = np.random.default_rng(900 + i)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    noise = rng.uniform(-0.01, 0.01, (H, W)).astype(F)
    odd = ((u + v + i) & 1) == 1
    depth = np.zeros((H, W), dtype=F)
    if i == 0:
        u0, u1, v0, v1 = WINDOW
        win = (u >= u0) & (u < u1) & (v >= v0) & (v < v1)
        wall = _far(u) if far0 else (F(1.0) + noise).astype(F)
        depth[win] = wall[win]
        depth[win & odd & ((v < 60) | holes_b)] = 0
    else:
        a, b, c = (v < 60), (v >= 60) & (v < 90), (v >= 90)
        da, db = ((1.06, 1.3), (0.95, 0.9))[i - 1]
        depth[a] = (F(da) + noise)[a]
        depth[b] = (F(db) + noise)[b]
        depth[c] = _far(u + 4 * (i - 1))[c]
        depth[(a if i == 1 else b) & odd] = 0
        depth[:, :CARVE_COLS] = 0
    band = ((v // 4) + i) % 3
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    rgb[band == 0] = 0
    rgb[band == 1] = 255
    ht = lt = None
    if semantic:
        ht = rng.uniform(0.05, 0.95, (H, W)).astype(F)
        lt = (F(1) - ht).astype(F)
        stripe = ((u // 8) + i) % 5
        ht[stripe == 1], lt[stripe == 1] = 0, 1
        ht[stripe == 3], lt[stripe == 3] = 1, 0
        both = (stripe == 4) & ((v // 8) % 4 == 0)
        ht[both], lt[both] = 0, 0
    for a_ in (rgb, depth, ht, lt):
        if a_ is not None:
            a_.setflags(write=False)
    return Frame(rgb, depth, ht, lt)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement (oracle lines 483-506; voxel_tsdf.cu:183-228)
@functools.lru_cache(maxsize=None)
def _range_image():
    """img_depth_to_range: |K^-1 (x, y, 1)|, float32 in the oracle's order"""
    fxi = F(1) / F(FX)
    cxi, cyi = (-F(CX)) * fxi, (-F(CY)) * fxi
    y, x = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    px, py, pz = fxi * x + cxi * F(1), fxi * y + cyi * F(1), F(1)
    return np.sqrt(px * px + (py * py + pz * pz)).astype(F)


def _round_away(q):
    q = q.astype(np.float64)
    return np.where(q >= 0, np.floor(q + 0.5), np.ceil(q - 0.5)).astype(np.int64)


class Prediction(NamedTuple):
    upd: np.ndarray   # [n, 512] bool: the frame updates the voxel
    k: np.ndarray     # [n, 512] pixel index (0 where the voxel falls outside the image)
    ts: np.ndarray    # [n, 512] float32 truncated signed distance of the update (where upd)
    wn: np.ndarray    # [n, 512] float32 w_new (where upd)


def predict(pos, fr):
    """which voxels of the blocks at `pos` the frame updates, and with which pixel, ts and w_new"""
    pos = np.asarray(pos).astype(np.int64).reshape(-1, 3)
    vi = np.arange(512)
    g = [(pos[:, a, None] * 8 + ((vi >> s) & 7)[None, :]).astype(F) * F(VS) for a, s in ((0, 0), (1, 3), (2, 6))]
    x, y, z = g  # identity pose: camera coordinates = world coordinates
    with np.errstate(all="ignore"):
        pu = (F(FX) * x + F(CX) * z) / z
        pv = (F(FX) * y + F(CY) * z) / z
        iu, iv = _round_away(pu), _round_away(pv)
        inb = (iu >= 0) & (iu < W) & (iv >= 0) & (iv < H)
        k = np.where(inb, iv * W + iu, 0)
        d = fr.depth.reshape(-1)[k]
        ok = inb & ~((d == 0) | (d > F(MD)))
        sdf = (_range_image().reshape(-1)[k] * (d - z)).astype(F)
        upd = ok & (sdf > -F(TRUNC))
        ts = np.minimum(F(1), sdf / F(TRUNC)).astype(F)
        wn = ((F(1) - d / F(MD)) * F(4)).astype(F)
    return Prediction(upd, k, ts, wn)


def partner(a):
    """a[n, 512] seen from each voxel's lane partner (the x-neighbour of the pair 2k, 2k + 1)"""
    return a[:, np.arange(512) ^ 1]


# ---------------------------------------------------------------------------------------------------------------------
# priors
class Entry(NamedTuple):
    t: object = None   # tsdf: a float, an int (bit pattern), or None = ordinary, drawn in [-1, 1]
    w: int = 7
    rgb: object = None  # (r, g, b) or None = random
    p: object = None   # probability or None = ordinary, drawn in (0.02, 0.98)


BYTES = (0, 1, 127, 128, 254, 255)
WEIGHTS = (0, 1, 2, 39, 40, 41, 44, 127, 128, 254, 255)
EDGE_WEIGHTS = (0, 1, 40, 255)
NAN_POS, NAN_NEG = 0x7FC12345, 0xFFC00ABC  # quiet NaNs of both signs with a payload
_P9 = float(F(0.9))
TSDF_WORDS = (0.0, -0.0, DENORM_MIN, -DENORM_MIN, DENORM_MAX, -DENORM_MAX, FLT_MIN, -FLT_MIN,
              _P9, float(_next(_P9, 0)), float(_next(_P9, 1)), -_P9, -float(_next(_P9, 0)), -float(_next(_P9, 1)),
              1.0, -1.0, 1e30, -1e30, FLT_MAX, -FLT_MAX, float("inf"), -float("inf"), NAN_POS, NAN_NEG)
PROBS = (0.0, 1.0, 1e-40, FLT_MIN, float(_next(1, 0)), float(_next(0.5, 1)), 1.5, -0.25, float("inf"), float("nan"))

ENTRIES = dict(
    weights=tuple(Entry(w=w, rgb=(BYTES[i], BYTES[(i + 1) % 6], BYTES[(i + 3) % 6])) for w in WEIGHTS for i in range(6)),
    tsdf=tuple(Entry(t=t, w=w) for t in TSDF_WORDS for w in EDGE_WEIGHTS),
    prob=tuple(Entry(p=p, w=w) for p in PROBS for w in EDGE_WEIGHTS),
    wnew=tuple(Entry(t=t, w=w) for w in (0, 255) for t in (0.25, -0.75, -0.0, 1.0)),
    # words whose exact bits a store of a voxel that did not update would lose or that only an import brings
    # depth == max_depth on voxels before and BEHIND it: w_new = 0 with ts < 0, the one way to a numerator of -0
    far=tuple(Entry(t=t, w=w) for t in (-0.0, 0.0, -0.5, 0.5, -DENORM_MIN, NAN_POS) for w in (0, 1, 255)),
    holes=(Entry(t=NAN_POS, w=7), Entry(t=NAN_NEG, w=40), Entry(t=-0.0, w=3), Entry(t=0.5, w=0), Entry(t=0.3, w=12),
           Entry(t=-0.6, w=255, p=float(_next(1, 0)))),
)
POOLS = tuple(ENTRIES)
# (far0, holes_b) of frame 0 and which of the three frames carry ht / lt
FRAME_KW = dict(weights=(False, False, (True, True, True)), tsdf=(False, False, (True, True, True)),
                prob=(False, False, (True, False, True)), wnew=(True, False, (True, True, True)),
                holes=(False, True, (True, True, True)), far=(True, False, (True, True, True)))
POOL_BLOCKS = dict(far=FAR_POS)  # (every other pool: POOL_POS)


def frames(pool):
    far0, holes_b, sem = FRAME_KW[pool]
    return tuple(frame(i, far0 if i == 0 else False, holes_b if i == 0 else False, sem[i]) for i in range(3))


def carve_blocks():
    """(names, positions, tsdf [14, 512], weight [14], verdict [14] bool): blocks full of one word except where said.
    The verdict is the reference's rule (space_carving_kernel): an fminf chain over |t|, carved iff it is >= 0.9f."""
    nan, inf = F(np.nan), F(np.inf)
    full = lambda t: np.full(512, t, dtype=F)

    def with_one(t, at, one):
        b = full(t)
        b[at] = one
        return b
    mixed = full(inf)
    mixed[1::3] = nan
    made = [("NaN only", full(nan), 5), ("NaN with one 0.95", with_one(nan, 77, 0.95), 5), ("0.9f", full(_P9), 5),
            ("0.9f with one predecessor", with_one(_P9, 333, _next(_P9, 0)), 5), ("-0.9f", full(-_P9), 5),
            ("+inf", full(inf), 5), ("inf mixed with NaN", mixed, 5), ("the fresh word", full(-1.0), 1)]
    made += [(f"1.0 with 0.5 at voxel {at}", with_one(1.0, at, 0.5), 5) for at in SINGLE_LOW_AT]
    t = np.stack([m[1] for m in made])
    with np.errstate(invalid="ignore"):
        verdict = np.fmin.reduce(np.abs(t), axis=1) >= F(0.9)  # np.fmin: a NaN never wins, as fminf
    return ([m[0] for m in made], np.array(_CARVE_AT[:len(made)], dtype=np.int16), t,
            np.array([m[2] for m in made], dtype=np.uint8), verdict)


class Case(NamedTuple):
    pool: str
    blocks: tuple        # (positions [n, 3], tsdf, rgbw, prob): pool blocks first, then the carve blocks
    entry: np.ndarray    # [n_pool, 512] index into ENTRIES[pool] of every pool voxel
    frames: tuple
    n_pool: int


@functools.lru_cache(maxsize=None)
def case(pool):
    entries = ENTRIES[pool]
    fr = frames(pool)
    pool_pos = POOL_BLOCKS.get(pool, POOL_POS)
    n = len(pool_pos)
    rng = np.random.default_rng(sum(map(ord, pool)))
    upd = predict(pool_pos, fr[0]).upd
    xpar = np.broadcast_to((np.arange(512) & 1)[None, :], upd.shape)
    stratum = (upd * 4 + partner(upd) * 2 + xpar).reshape(-1)
    entry = np.zeros(n * 512, dtype=np.int64)
    for s in range(8):
        at = np.flatnonzero(stratum == s)
        entry[rng.permutation(at)] = (np.arange(len(at)) + 5 * s) % len(entries)
    entry = entry.reshape(n, 512)
    # the ordinary words, then each entry's own
    t = rng.uniform(-1, 1, (n, 512)).astype(F)
    p = rng.uniform(0.02, 0.98, (n, 512)).astype(F)
    c = np.zeros((n, 512), dtype=RGBW_DTYPE)
    for ch in ("r", "g", "b"):
        c[ch] = rng.integers(0, 256, (n, 512))
    for j, e in enumerate(entries):
        m = entry == j
        c["weight"][m] = e.w
        if e.t is not None:
            t[m] = fbits(e.t) if isinstance(e.t, int) else F(e.t)
        if e.rgb is not None:
            c["r"][m], c["g"][m], c["b"][m] = e.rgb
        if e.p is not None:
            p[m] = F(e.p)
    _, cpos, ct, cw, _ = carve_blocks()
    cc = np.zeros(ct.shape, dtype=RGBW_DTYPE)
    cc["r"], cc["g"], cc["b"], cc["weight"] = 9, 99, 199, cw[:, None]
    blocks = (np.concatenate([pool_pos, cpos]), np.concatenate([t, ct]), np.concatenate([c, cc]),
              np.concatenate([p, np.full(ct.shape, 0.25, dtype=F)]))
    for a in blocks + (entry,):
        a.setflags(write=False)
    return Case(pool, blocks, entry, fr, n)


def occurrences(cs):
    """per entry of the case's table, over frame 0: [n_entries, 6] counts of voxels that update, stay untouched,
    have an updating partner, belong to a pair of which exactly one updates, and lie on even / odd x"""
    upd = predict(cs.blocks[0][:cs.n_pool], cs.frames[0]).upd
    pu = partner(upd)
    odd = np.broadcast_to((np.arange(512) & 1).astype(bool)[None, :], upd.shape)
    out = np.zeros((len(ENTRIES[cs.pool]), 6), dtype=np.int64)
    for j in range(len(out)):
        m = cs.entry == j
        out[j] = [(m & upd).sum(), (m & ~upd).sum(), (m & pu).sum(), (m & (upd != pu)).sum(), (m & ~odd).sum(),
                  (m & odd).sum()]
    return out


def one_of_a_pair(upd):
    """lane pairs of which exactly one voxel updates"""
    return int((upd != partner(upd)).sum()) // 2


# ---------------------------------------------------------------------------------------------------------------------
# what a frame must leave
def keys(pos):
    p = np.asarray(pos).astype(np.int64) & 0xFFFF
    return p[:, 0] | (p[:, 1] << 16) | (p[:, 2] << 32)


def by_position(s):
    o = np.argsort(keys(s[0]), kind="stable")
    return tuple(a[o] for a in s)


def align(before, after):
    """rows of `before` (a block set) for the blocks of `after`, and which blocks of `after` it holds"""
    kb, ka = keys(before[0]), keys(after[0])
    o = np.argsort(kb)
    at = np.searchsorted(kb[o], ka)
    at = o[np.minimum(at, len(kb) - 1)]
    return at, kb[at] == ka


def words(s, rows=slice(None)):
    """the three voxel words of a block set as uint32 [n, 512, 3]"""
    return np.stack([bits(s[1][rows]), np.ascontiguousarray(s[2][rows]).view(U32), bits(s[3][rows])], axis=-1)


def untouched_unchanged(before, after, fr, predict=None):
    """every voxel the frame does not update holds its three words bit for bit (blocks present on both sides).
    Returns how many such voxels there were; raises AssertionError naming the first that changed.
    (predict: another case module's restatement, e.g. proj_cases.predict; this module's by default)"""
    at, held = align(before, after)
    upd = (predict or globals()["predict"])(after[0][held], fr).upd
    wb, wa = words(before, at[held]), words(after, held)
    bad = (wb != wa).any(axis=-1) & ~upd
    assert not bad.any(), (f"{int(bad.sum())} voxels that the frame does not update changed, first at block "
                           f"{after[0][held][np.argwhere(bad)[0][0]].tolist()} voxel {int(np.argwhere(bad)[0][1])}: "
                           f"{wb[bad][0].tolist()} -> {wa[bad][0].tolist()}")
    return int((~upd).sum())


def formula_float64(before, fr):
    """the reference's expression (voxel_tsdf.cu:228, 236, 238) in float64 on the float32 operands, for the blocks of
    `before`: (upd, tsdf, tsdf bound, weight).  The bound is the four float32 roundings of (t wo + ts wn) / wc."""
    pr = predict(before[0], fr)
    t, wo = before[1].astype(np.float64), before[2]["weight"].astype(np.float64)
    ts, wn = pr.ts.astype(np.float64), pr.wn.astype(np.float64)
    wc = (before[2]["weight"].astype(F) + pr.wn).astype(np.float64)  # the float32 sum, as the divisor is
    with np.errstate(all="ignore"):
        q = (t * wo + ts * wn) / wc
        bound = 4 * 2.0 ** -24 * (np.abs(t) * wo + np.abs(ts) * wn) / wc
        w = np.minimum(np.floor(wc + 0.5), 40)
    return pr.upd, q, bound, w
