"""Crafted maps and engine-free expectations for the two surface read-outs on awkward voxel VALUES: surface points
(ratsdf_surface_points[_device], include/ratsdf_surface.h) and the welded mesh (ratsdf_surface_mesh[_device],
include/ratsdf_surface_mesh.h).  Written once and run without a GPU (tests/test_surface_cases.py) and against the HIP
engine (tests/test_gpu_surface_cases.py).  Same role as fuse_cases.py, resample_cases.py and readout_cases.py: no GPU
and no torch at import.

Every set is a BlockSet for import_blocks over the 3 x 3 x 3 blocks -1 .. 1 (voxels -8 .. 15), every voxel observed
with weight 3, colour from the voxel index and a probability of its own, read out over one box that is not block
aligned and sticks out of the map on every side.  What is expected never comes from an engine: the records are
surface_ref.surface_points / surface_mesh_ref.surface_mesh fed from the BlockSet.

`evaluate` restates the per-edge formula of the header a second time, edge by edge on flat arrays and not on shifted
dense ones, for two reasons: it hands out every intermediate (f, t0 - t1, d_b, the products, g_b, len^2, len), which the
CPU test needs to count the classes of records a set holds, and it takes a `Variant` whose fields each plant ONE
mistake, which the CPU test uses to show that the named set tells the mistake from the contract.  Its default output is
asserted to be surface_ref's, byte for byte.

The sets:
  ladder_small / ladder_large   one tilted, perturbed plane (crossings on all three axes, in blocks and across seams)
                   scaled by 2^e, a new e every two z layers: from all-normal arithmetic down to subnormal tsdf words
                   (len^2 subnormal, len^2 underflowing to 0) and up to len^2 and t0 - t1 overflowing
  nonfinite        the plane with +inf, -inf, a quiet NaN and a negative NaN with a payload planted on a lattice five
                   voxels apart (local indices 0, 5, 2, 7, 4: inside blocks, at their first and at their last voxel)
  quotients        endpoint pairs with f exactly 0.5, one ulp either side, rounding to 1.0, 0, -0.0 and subnormal, on
                   every axis, at owner local index 7 and inside a block
  probabilities    the plane with NaN, -0.0, +inf, subnormal and ordinary probability words, read at four min_prob
"""
import functools
from collections import Counter
from typing import NamedTuple

import numpy as np

import surface_mesh_ref as smr
import surface_ref as sr
from raycast_cases import BlockSet

F = np.float32
VS, TRUNC = 0.02, 0.12
ENGINE = dict(block_bits=10)
BLOCK_LO, BLOCK_HI = (-1, -1, -1), (1, 1, 1)            # voxels -8 .. 15 per axis
ORIGIN, DIMS = (-9, -10, -9), (26, 26, 25)              # not block aligned; one voxel beyond the map on five sides
WEIGHT = 3
TINY = np.finfo(F).tiny                                 # 2^-126, the smallest normal float32
UNIT = np.eye(3, dtype=np.int64)


def bits(word):
    """the float32 with the bits `word`"""
    return np.uint32(word).view(F)


PLUS_INF, MINUS_INF, QUIET_NAN, PAYLOAD_NAN = 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFD2C3B4
DENORMAL = float(bits(1))


# ---------------------------------------------------------------------------------------------------------------------
# the maps
def _grid():
    """block positions [27, 3] int16 and the voxel indices [27, 512, 3] of the map's blocks"""
    r = [np.arange(a, b + 1) for a, b in zip(BLOCK_LO, BLOCK_HI)]
    pos = np.stack(np.meshgrid(*r, indexing="ij"), -1).reshape(-1, 3)
    i = np.arange(512)
    loc = np.stack([i & 7, (i >> 3) & 7, i >> 6], -1)
    return pos.astype(np.int16), pos[:, None, :].astype(np.int64) * 8 + loc[None, :, :]


def _noise(v, seed):
    """a hash of the voxel index, uniform in [0, 1), float64"""
    h = (v[..., 0] * 374761393 + v[..., 1] * 668265263 + v[..., 2] * 2147483647 + seed * 144665) & 0xFFFFFFFF
    h = ((h ^ (h >> 13)) * 1274126177) & 0xFFFFFFFF
    h ^= h >> 16
    return h.astype(np.float64) / 2.0 ** 32


def _plane(v):
    """the tilted, perturbed plane (float64): steep along x (2.2 per voxel: at a crossing |t0| + |t1| is about 2), 0.9
    along y, 0.6 along z, plus noise of +-0.2, clipped to +-1.9 so that 2^127 times it is finite"""
    x, y, z = (v[..., b].astype(np.float64) for b in range(3))
    d = 2.2 * (x - 3.3 - 0.41 * (y - 3.0) - 0.27 * (z - 3.0)) + 0.4 * (_noise(v, 1) - 0.5)
    return np.clip(d, -1.9, 1.9)


def _blockset(pos, v, tsdf, prob=None):
    rgbw = np.zeros(tsdf.shape, dtype=sr.RGBW)
    rgbw["r"], rgbw["g"], rgbw["b"] = v[..., 0] & 255, v[..., 1] & 255, v[..., 2] & 255
    rgbw["weight"] = WEIGHT
    if prob is None:
        prob = (0.05 + 0.9 * _noise(v, 2)).astype(F)    # one per voxel: a wrongly chosen endpoint shows
    return BlockSet(pos, np.ascontiguousarray(tsdf, dtype=F), rgbw, np.ascontiguousarray(prob, dtype=F))


# the exponent of each pair of z layers, z = -8 .. 15.  The two smallest steps lie between large ones: there d_z is an
# ordinary number while d_x and d_y are a few units of 2^-149, so len is not 0 and a wrongly rounded d_x shows in the
# normal.
SMALL_EXPONENTS = (0, -147, -40, -142, -62, -66, -70, -74, -80, -100, -126, -135)
LARGE_EXPONENTS = (0, 40, 62, 63, 64, 66, 90, 120, 125, 126, 127, 127)


def _ladder(exponents):
    pos, v = _grid()
    e = np.array(exponents, dtype=np.float64)[(v[..., 2] + 8) >> 1]
    return _blockset(pos, v, np.ldexp(_plane(v), e.astype(np.int64)).astype(F))


class Planted(NamedTuple):
    voxel: tuple
    word: int          # the tsdf bits


NONFINITE_WORDS = (PLUS_INF, MINUS_INF, QUIET_NAN, PAYLOAD_NAN)
LATTICE = (-8, -3, 2, 7, 12)                            # local indices 0, 5, 2, 7, 4


def nonfinite_planted():
    out = []
    for k, z in enumerate(LATTICE):
        for j, y in enumerate(LATTICE):
            for i, x in enumerate(LATTICE):
                out.append(Planted((x, y, z), NONFINITE_WORDS[(i + j + 2 * k) % 4]))
    return out


def _plant(tsdf, v, planted):
    t = tsdf.copy()
    for p in planted:
        at = np.all(v == np.array(p.voxel), axis=-1)
        assert at.sum() == 1
        t.view(np.uint32)[at] = p.word
    return t


class Pair(NamedTuple):
    kind: str
    axis: int
    seam: bool
    owner: tuple
    t0: float
    t1: float
    f_bits: int        # what t0 / (t0 - t1) must be


def _quotient_values():
    """kind -> (t0, t1, the bits of f).  The two neighbours of 0.5 are searched for among quotients near 1 / 2."""
    half = F(0.5)
    below, above = np.nextafter(half, F(0)), np.nextafter(half, F(1))
    out = {"half": (F(0.375), F(-0.375), half), "one": (F(-1.0), F(2.0 ** -30), F(1.0)),
           "zero": (F(0.0), F(-0.5), F(0.0)), "minus_zero": (F(-0.0), F(-0.5), F(-0.0)),
           "subnormal": (F(2.0 ** -140), F(-1.0), F(2.0 ** -140))}
    for name, target in (("half_below", below), ("half_above", above)):
        found = None
        for j in range(-16, 17):
            for k in range(-16, 17):
                t0, t1 = F(1.0 + j * 2.0 ** -23), F(-(1.0 + k * 2.0 ** -23))
                if found is None and F(t0 / F(t0 - t1)).view(np.uint32) == target.view(np.uint32):
                    found = (t0, t1, target)
        assert found is not None, name
        out[name] = found
    for t0, t1, f in out.values():
        assert F(t0 / F(t0 - t1)).view(np.uint32) == F(f).view(np.uint32)
    return out


QUOTIENT_KINDS = ("half", "half_below", "half_above", "one", "zero", "minus_zero", "subnormal")


@functools.lru_cache(maxsize=None)
def quotient_pairs():
    """every kind on every axis, inside block 0 (owner local 3) and at a seam (owner local 7 of block 0 or of block -1:
    the upper endpoint is voxel 0 of the next block)"""
    values = _quotient_values()
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for q, kind in enumerate(QUOTIENT_KINDS):
            for s in (0, 1):
                k = 2 * q + s
                owner = [0, 0, 0]
                owner[a] = 3 if s == 0 else (7 if q % 2 == 0 else -1)
                owner[b] = -6 + 4 * (k % 5)
                owner[c] = 5 + 4 * (k // 5)
                t0, t1, f = values[kind]
                out.append(Pair(kind, a, bool(s), tuple(owner), float(t0), float(t1), int(F(f).view(np.uint32))))
    cells = [p.owner for p in out] + [tuple(np.add(p.owner, UNIT[p.axis])) for p in out]
    assert len(set(cells)) == len(cells), "two pairs share a voxel"
    return tuple(out)


MIN_PROB_BETWEEN = 4 * DENORMAL                         # between the probability words 3 and 5
PROB_WORDS = (None, 0x7FC00000, 0xFFC54321, 0x80000000, PLUS_INF, 3, 5, 0x80000002, 0, None)   # None: an ordinary one


class Case(NamedTuple):
    name: str
    blocks: BlockSet
    min_probs: tuple = (0.0,)
    mesh: bool = True          # part of mesh_values
    origin: tuple = ORIGIN
    dims: tuple = DIMS


@functools.lru_cache(maxsize=None)
def case(name):
    pos, v = _grid()
    if name == "ladder_small":
        return Case(name, _ladder(SMALL_EXPONENTS))
    if name == "ladder_large":
        return Case(name, _ladder(LARGE_EXPONENTS))
    if name == "nonfinite":
        return Case(name, _blockset(pos, v, _plant((_plane(v) * 0.5).astype(F), v, nonfinite_planted())))
    if name == "quotients":
        t = (0.5 + 0.3 * (_noise(v, 3) - 0.5)).astype(F)                    # positive everywhere
        planted = []
        for p in quotient_pairs():
            planted.append(Planted(p.owner, int(F(p.t0).view(np.uint32))))
            planted.append(Planted(tuple(np.add(p.owner, UNIT[p.axis])), int(F(p.t1).view(np.uint32))))
        return Case(name, _blockset(pos, v, _plant(t, v, planted)))
    if name == "probabilities":
        pick = (_noise(v, 4) * len(PROB_WORDS)).astype(np.int64)
        prob = (0.05 + 0.9 * _noise(v, 2)).astype(F)
        for i, w in enumerate(PROB_WORDS):
            if w is not None:
                prob.view(np.uint32)[pick == i] = w
        return Case(name, _blockset(pos, v, (_plane(v) * 0.5).astype(F), prob),
                    min_probs=(0.0, -0.0, MIN_PROB_BETWEEN, float("inf")), mesh=False)
    raise KeyError(name)


CASES = ("ladder_small", "ladder_large", "nonfinite", "quotients", "probabilities")
MESH_CASES = tuple(n for n in CASES if n != "probabilities")        # mesh_values


def blocks_of(c):
    return sr.blocks_of(*c.blocks)


def sign_map(blocks):
    """the same map with every tsdf word replaced by +-1 of equal "negative" bit (t < 0: NaN, -0.0 and 0.0 are not
    negative).  The weight is 3: -1.0 is no fresh voxel here."""
    with np.errstate(invalid="ignore"):
        t = np.where(blocks.tsdf < 0, F(-1), F(1)).astype(F)
    assert (blocks.rgbw["weight"] == WEIGHT).all()
    return BlockSet(blocks.pos, t, blocks.rgbw, blocks.prob)


# ---------------------------------------------------------------------------------------------------------------------
# the per-edge restatement, with every intermediate and with planted mistakes
class Variant(NamedTuple):
    """the contract when every field is at its default; each other value is ONE mistake a kernel could make"""
    flush_in: bool = False         # subnormal tsdf words read as zero
    flush_out: bool = False        # subnormal results of every operation flushed to zero
    fma: bool = False              # g_b = fma(d0, 1 - f, d1 * f), len^2 = fma(g2, g2, fma(g1, g1, g0 * g0))
    tie_gt: bool = False           # the upper endpoint iff f > 0.5f
    negative: str = "lt"           # "signbit": -0.0 (and a NaN with the sign set) is negative; "not_ge": !(t >= 0)
    flat: str = "contract"         # "zero_only": flat iff len == 0; "none": always g_b / len
    split_half: bool = False       # the central difference as tu * 0.5f - td * 0.5f
    prob_flushed: bool = False     # prob < min_prob on operands with subnormals flushed
    seam_own_block: bool = False   # at a seam the upper endpoint's prob and rgbw taken from the owner's block
    f64: bool = False              # NOT a mistake: the same formulas in float64 (the distance of the fp32 contract from
    #                                the real-number one is measured against it)


CONTRACT = Variant()


def flush(x):
    x = np.asarray(x)
    return np.where(np.abs(x) < TINY, np.copysign(x.dtype.type(0), x), x)


class _Arith:
    def __init__(self, variant):
        self.v, self.T = variant, (np.float64 if variant.f64 else F)

    def r(self, x):
        x = np.asarray(x, dtype=self.T)
        return flush(x) if self.v.flush_out else x

    def sub(self, a, b):
        return self.r(a - b)

    def add(self, a, b):
        return self.r(a + b)

    def mul(self, a, b):
        return self.r(a * b)

    def div(self, a, b):
        return self.r(a / b)

    def sqrt(self, a):
        return self.r(np.sqrt(a))

    def fma(self, a, b, c):
        """a * b + c with one rounding (the product of two float32 is exact in float64; the second rounding of the sum
        can differ from a true fma's in rare ties, which does not matter for a variant that is wrong anyway)"""
        a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
        return self.r((a * b + c).astype(self.T))


class Edges(NamedTuple):
    """the records of a box in the header's order, and per record what they were made of"""
    rec: np.ndarray            # sr.POINT
    owner: np.ndarray          # [n, 3] int64
    axis: np.ndarray           # [n]
    t0: np.ndarray
    t1: np.ndarray
    den: np.ndarray            # t0 - t1
    f: np.ndarray
    u: np.ndarray              # 1 - f
    d0: np.ndarray             # [n, 3]
    d1: np.ndarray
    p0: np.ndarray             # d0 * (1 - f)
    p1: np.ndarray             # d1 * f
    g: np.ndarray
    sq: np.ndarray             # g * g
    len2: np.ndarray
    len: np.ndarray
    up: np.ndarray             # the upper endpoint is the chosen one
    pos: np.ndarray            # [n, 3] pos and normal in the working precision (float64 for Variant.f64)
    normal: np.ndarray


def evaluate(blocks, origin, dims, vs=VS, min_weight=1, min_prob=0.0, variant=CONTRACT):
    """include/ratsdf_surface.h edge by edge.  blocks: surface_ref's dict."""
    var, A = variant, _Arith(variant)
    T_ = A.T
    o = np.array([int(x) for x in origin], dtype=np.int64)
    n = np.array([int(x) for x in dims], dtype=np.int64)
    lo, hi = o - 1, o + n + 1
    t, obs, p, c = sr._dense(blocks, lo, hi, int(min_weight))
    if var.flush_in:
        t = flush(t)
    t = t.astype(T_)

    def at(arr, w):
        return arr[w[:, 2] - lo[2], w[:, 1] - lo[1], w[:, 0] - lo[0]]

    def negative(x):
        if var.negative == "signbit":
            return np.signbit(x)
        if var.negative == "not_ge":
            return ~(x >= 0)
        return x < 0

    def diff(w, b):
        up, dn = at(obs, w + UNIT[b]), at(obs, w - UNIT[b])
        tu, td, tw = at(t, w + UNIT[b]), at(t, w - UNIT[b]), at(t, w)
        half = T_(0.5)
        both = A.sub(A.mul(tu, half), A.mul(td, half)) if var.split_half else A.mul(A.sub(tu, td), half)
        return np.where(up & dn, both, np.where(up, A.sub(tu, tw), np.where(dn, A.sub(tw, td), T_(0))))

    zz, yy, xx = np.meshgrid(*[np.arange(o[b], o[b] + n[b]) for b in (2, 1, 0)], indexing="ij")
    box = np.stack([xx, yy, zz], axis=-1).reshape(-1, 3)
    vsT, mp = T_(F(vs)), F(min_prob)
    parts = []
    with np.errstate(all="ignore"):
        for a in range(3):
            t0, t1 = at(t, box), at(t, box + UNIT[a])
            cross = at(obs, box) & at(obs, box + UNIT[a]) & (negative(t0) != negative(t1))
            v = box[cross]
            w = v + UNIT[a]
            t0, t1 = t0[cross], t1[cross]
            den = A.sub(t0, t1)
            f = A.div(t0, den)
            u = A.sub(T_(1), f)
            d0 = np.stack([diff(v, b) for b in range(3)], axis=1)
            d1 = np.stack([diff(w, b) for b in range(3)], axis=1)
            p1 = A.mul(d1, f[:, None])
            if var.fma:
                p0 = A.mul(d0, u[:, None])
                g = A.fma(d0, u[:, None], p1)
                sq = A.mul(g, g)
                len2 = A.fma(g[:, 2], g[:, 2], A.fma(g[:, 1], g[:, 1], sq[:, 0]))
            else:
                p0 = A.mul(d0, u[:, None])
                g = A.add(p0, p1)
                sq = A.mul(g, g)
                len2 = A.add(A.add(sq[:, 0], sq[:, 1]), sq[:, 2])
            ln = A.sqrt(len2)
            if var.flat == "zero_only":
                flat = ln == 0
            elif var.flat == "none":
                flat = np.zeros(len(ln), dtype=bool)
            else:
                flat = (ln == 0) | ~np.isfinite(ln)
            up = (f > T_(0.5)) if var.tie_gt else (f >= T_(0.5))
            chosen = np.where(up[:, None], w, v)
            if var.seam_own_block:
                chosen = np.where((up & ((v[:, a] & 7) == 7))[:, None], v - 7 * UNIT[a], chosen)
            prob = at(p, chosen)
            keep = ~((flush(prob) < flush(mp)) if var.prob_flushed else (prob < mp))
            rec = np.zeros(len(v), dtype=sr.POINT)
            pos = np.stack([A.mul(A.add(v[:, b].astype(T_), f) if b == a else v[:, b].astype(T_), vsT)
                            for b in range(3)], axis=1)
            normal = np.where(flat[:, None], T_(0), A.div(g, ln[:, None]))
            rec["pos"], rec["normal"] = pos, normal
            rec["prob"] = prob
            rec["rgbw"] = at(c, chosen).view(sr.RGBW)
            e = Edges(rec, v, np.full(len(v), a), t0, t1, den, f, u, d0, d1, p0, p1, g, sq, len2, ln, up, pos, normal)
            parts.append(Edges(*(x[keep] for x in e)))
    e = Edges(*(np.concatenate(x) for x in zip(*parts)))
    v = e.owner
    local = (v[:, 0] & 7) + 8 * (v[:, 1] & 7) + 64 * (v[:, 2] & 7)
    order = np.lexsort((e.axis, local, v[:, 0] >> 3, v[:, 1] >> 3, v[:, 2] >> 3))
    return Edges(*(x[order] for x in e))


# ---------------------------------------------------------------------------------------------------------------------
# expectations: computed once, shared, never changed
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def expected_points(name, min_prob=0.0):
    """surface_ref's records of the set's box"""
    c = case(name)
    with np.errstate(all="ignore"):
        return _frozen(sr.surface_points(blocks_of(c), c.origin, c.dims, VS, 1, min_prob))


@functools.lru_cache(maxsize=None)
def expected_edges(name, min_prob=0.0, variant=CONTRACT, over_mesh=False):
    """`evaluate` on the set's box (over_mesh: on the owners of the mesh's vertices, one voxel more per axis, and
    without a min_prob)"""
    c = case(name)
    dims = tuple(d + 1 for d in c.dims) if over_mesh else c.dims
    min_prob = float("-inf") if over_mesh else min_prob
    return evaluate(blocks_of(c), c.origin, dims, VS, 1, min_prob, variant)


@functools.lru_cache(maxsize=None)
def expected_mesh(name, signs_only=False):
    """surface_mesh_ref's (vertices, triangles) of the set's box; signs_only: of the +-1 map"""
    c = case(name)
    b = sign_map(c.blocks) if signs_only else c.blocks
    with np.errstate(all="ignore"):
        return _frozen(*smr.surface_mesh(sr.blocks_of(*b), c.origin, c.dims, VS, 1))


# ---------------------------------------------------------------------------------------------------------------------
# the comparison rule
def _floats(rec):
    """[n, 7] pos, normal, prob"""
    return np.concatenate([rec["pos"], rec["normal"], rec["prob"][:, None]], axis=1)


def exempt(want, edges):
    """[n, 3] bool: the float fields where only "is NaN" is compared -- pos[a] of the records whose f is NaN.  A NaN
    that went through arithmetic has no agreed bits (numpy alone yields 0xFFC00000 and 0x7FC00000 here).  Asserts the
    cap: a NaN of the restatement's pos or normal lies nowhere else; a NaN probability is a copied word and compares
    as bytes."""
    assert len(want) == len(edges.rec)
    allowed = np.zeros((len(want), 3), dtype=bool)
    allowed[np.arange(len(want)), edges.axis] = np.isnan(edges.f)
    assert not np.isnan(want["normal"]).any(), "the flat rule makes a NaN normal impossible"
    assert np.array_equal(np.isnan(want["pos"]), allowed), "pos is NaN exactly where f is"
    return allowed


def differing(got, want, allowed):
    """how many records differ: byte for byte, but where `allowed` (exempt()) both sides need only be NaN.  -1: the
    counts differ."""
    if got.dtype.itemsize != want.dtype.itemsize or got.shape != want.shape:
        return -1
    g = np.ascontiguousarray(got).copy().view(sr.POINT)
    w = np.ascontiguousarray(want)
    both_nan = allowed & np.isnan(g["pos"])
    g["pos"].view(np.uint32)[both_nan] = w["pos"].view(np.uint32)[both_nan]
    a, b = g.view(np.uint8).reshape(len(g), -1), w.view(np.uint8).reshape(len(w), -1)
    return int((a != b).any(axis=1).sum())


def changed(a, b):
    """how many records a wrong variant changes: the records of one list that the other does not hold, as multisets
    (a variant may drop one record and add another: rows would shift), the larger of the two directions"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    ca, cb = Counter(r.tobytes() for r in a), Counter(r.tobytes() for r in b)       # (records can repeat: f = 0 or 1)
    return max(sum((ca - cb).values()), sum((cb - ca).values()))


def special_records(e):
    """[n] bool: records with an intermediate that is not an ordinary normal number (the capacities of the device
    forms cut inside a run of them)"""
    x = np.concatenate([e.t0[:, None], e.t1[:, None], e.den[:, None], e.f[:, None], e.d0, e.d1, e.g, e.len2[:, None],
                        e.rec["prob"][:, None]], axis=1)
    return (~np.isfinite(x) | ((x != 0) & (np.abs(x) < TINY)) | (np.signbit(x) & (x == 0))).any(axis=1)


def cut_inside_specials(e):
    """a capacity with a special record on either side of the cut, near the middle of the list (where the specials
    stand alone, as the planted pairs of `quotients` do: with a special record as the last one written)"""
    s = special_records(e)
    both = np.flatnonzero(s[:-1] & s[1:]) + 1
    if len(both) == 0:
        both = np.flatnonzero(s) + 1
    assert len(both) > 0
    return int(both[np.argmin(np.abs(both - len(s) // 2))])
