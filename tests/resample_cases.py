"""Crafted sources, poses and block lists for transformed map fusion (include/ratsdf_resample.h:
ratsdf_resample_blocks_device, ratsdf_fuse_map_transformed).  Written once, checked without a GPU in
tests/test_resample_cases.py (the cases are not vacuous, and planted mistakes fail them) and run against the HIP engine
in tests/test_gpu_resample_cases.py.  Same role as fuse_cases.py: no GPU and no torch at import.

What is expected never comes from an engine: it is tests/resample_ref.py (then tests/fuse_ref.py for the fusion step)
applied to crafted sources that go into their engines with import_blocks, so every voxel word is known.

Poses (`POSES`, by name; `pose_of` turns one into the seven floats for a source with a given centre):
  worst_{x,y,z}_{fwd,inv}   the rotation that takes e_a to (1, 1, 1) / sqrt(3) (54.7 degrees about e_a x n) and its
                            inverse, about the source's own centre: a row of the kernel's A, resp. of A^-1, with the
                            largest 1-norm a rotation has -- the footprint the 27-block table is sized for
  ..._up, ..._down          the same with the quaternion times sqrt(1.0009), sqrt(0.9991): accepted, and A is no rotation
  third_111, half_{x,y,z}   120 degrees about (1, 1, 1) and the half turns about the ORIGIN: quaternions float32 holds
                            exactly, so with vs = 2^-6 the source lattice maps onto the destination's.  Each with a
                            source-frame shift s (g = A d - s): `whole` (3, -5, 8), `half_x`, `half_yz`, `half_xyz`
                            (0.5 voxel: ties of roundf on both sides of zero) and `eps` (1e-9 voxel: g = -1e-9 at
                            d' = 0, whose fraction rounds to 1.0f)
  quarter_{x,y,z}           90 degrees about an axis with the same shifts.  sqrt(1/2) is no float32, so 2 s^2 is 1 +
                            1.3e-7 after se3_inverse and g misses the lattice by up to 1e-5 voxel: fractions next to 0,
                            next to 0.5 and next to 1 with their tiny weight factors, all eight corners needed
  diag_z, diag_xy           45 degrees about z and about (1, 1, 0), about the centre, generic translation
  overflowing               finite, accepted, but Ti.t / vs is not finite at vs = 0.01: nothing contributes anywhere

Sources (`source(key)`): dense 3 x 3 x 3 blocks (every voxel live: a probe that misses the table is a zeroed voxel in the
middle of a full block) at the origin and at three ends of the grid; the sparse `craft` maps (zero weights, fresh
voxels) straddling the origin and as one lone block; `values`, 2 x 2 x 2 blocks of awkward floats, weights 1 and 255 and
arbitrary probability words; `chained`, the dense source behind 600 filler blocks in a 512-bucket directory.

`resample_with` is a copy of the restatement with one switch per wrong line (`MISTAKES`) that also hands out what the
coverage conditions are about (fractions, needed corners, the table's base and reach).
"""
import functools
import math
from typing import NamedTuple

import numpy as np

import fuse_cases as fc
import fuse_ref
import resample_ref as rr
from fuse_ref import F
from ratsdf._abi import RGBW_DTYPE
from sample_ref import round_half_away

U32 = np.uint32
VS, VS_LATTICE, TRUNC = 0.01, 2.0 ** -6, 0.06
SMALL = tuple(0.1 * v for v in (0.1234, -0.0567, 0.0891))  # metres: no multiple of either voxel size
EPS = 1e-9
N111 = np.ones(3) / math.sqrt(3.0)


# ---------------------------------------------------------------------------------------------------------------------
# poses
def quat(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return np.array([*(a * math.sin(angle / 2)), math.cos(angle / 2)])


def linear(q):
    """the linear map of quat_rotate(q, .) for the float32 values of q, in float64 (a rotation only if |q| = 1)"""
    x, y, z, w = (float(F(v)) for v in q)
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + 2.0 * w * K + 2.0 * (K @ K)


class PoseSpec(NamedTuple):
    name: str
    family: str      # worst | scaled | lattice | quarter | diagonal | overflowing
    q: tuple
    shift: tuple     # source-frame shift in voxels about the origin, or None: about the source's centre, plus SMALL
    vs: float


def _specs():
    out = []
    for a, ax in enumerate("xyz"):
        e = np.eye(3)[a]
        fwd = quat(np.cross(e, N111), math.acos(1.0 / math.sqrt(3.0)))
        inv = fwd * np.array([-1.0, -1.0, -1.0, 1.0])
        for d, q in (("fwd", fwd), ("inv", inv)):
            out.append(PoseSpec(f"worst_{ax}_{d}", "worst", tuple(q), None, VS))
            out.append(PoseSpec(f"worst_{ax}_{d}_up", "scaled", tuple(q * math.sqrt(1.0009)), None, VS))
            out.append(PoseSpec(f"worst_{ax}_{d}_down", "scaled", tuple(q * math.sqrt(0.9991)), None, VS))
    s = math.sqrt(0.5)
    turns = [("third_111", "lattice", (0.5, 0.5, 0.5, 0.5)), ("half_x", "lattice", (1.0, 0.0, 0.0, 0.0)),
             ("half_y", "lattice", (0.0, 1.0, 0.0, 0.0)), ("half_z", "lattice", (0.0, 0.0, 1.0, 0.0)),
             ("quarter_x", "quarter", (s, 0.0, 0.0, s)), ("quarter_y", "quarter", (0.0, s, 0.0, s)),
             ("quarter_z", "quarter", (0.0, 0.0, s, s))]
    for name, family, q in turns:
        for sname, shift in SHIFTS.items():
            out.append(PoseSpec(f"{name}+{sname}", family, q, shift, VS_LATTICE))
    out.append(PoseSpec("third_111+none", "lattice", (0.5, 0.5, 0.5, 0.5), (0.0, 0.0, 0.0), VS_LATTICE))
    out.append(PoseSpec("diag_z", "diagonal", tuple(quat((0, 0, 1), math.pi / 4)), None, VS))
    out.append(PoseSpec("diag_xy", "diagonal", tuple(quat((1, 1, 0), math.pi / 4)), None, VS))
    out.append(PoseSpec("overflowing", "overflowing", (0.0, 0.0, 0.0, 1.0), None, VS))
    return {p.name: p for p in out}


SHIFTS = dict(whole=(3.0, -5.0, 8.0), half_x=(0.5, 0.0, 0.0), half_yz=(0.0, 0.5, 0.5), half_xyz=(0.5, 0.5, 0.5),
              eps=(EPS, EPS, EPS))
POSES = _specs()
OVERFLOWING = (0.0, 0.0, 0.0, 1.0, 3e38, 0.0, 0.0)


def pose_of(name, centre=(0.0, 0.0, 0.0)):
    """the seven floats of POSES[name] for a source whose centre is `centre` (voxels)"""
    p = POSES[name]
    if p.family == "overflowing":
        return OVERFLOWING
    M = linear(p.q)
    if p.shift is not None:   # g = A d - s  <=>  t = M s
        t = (M @ np.asarray(p.shift, dtype=np.float64)) * p.vs
    else:
        # the centre stays where it is, but for the small offset, under the map the CONTRACT defines: g = A (d - t)
        # with A of the inverse quaternion conj(q) / |q|^2 -- for |q| != 1 that is not the inverse of M, and 1e-3 of
        # scale would carry a source at the end of the grid 30 voxels away
        x, y, z, w = (float(F(v)) for v in p.q)
        n2 = x * x + y * y + z * z + w * w
        A = linear((-x / n2, -y / n2, -z / n2, w / n2))
        c = np.asarray(centre, dtype=np.float64) * float(F(p.vs))
        t = c - np.linalg.solve(A, c) + np.asarray(SMALL)
    return tuple(float(F(v)) for v in p.q) + tuple(float(v) for v in t)


def names(*families):
    return [n for n, p in POSES.items() if p.family in families]


# ---------------------------------------------------------------------------------------------------------------------
# sources
GRID3 = np.array([(x, y, z) for z in range(3) for y in range(3) for x in range(3)], dtype=np.int64)
ENDS = ((-4096, -4096, -4096), (4093, 4093, 4093), (4090, -4096, 4000))


@functools.lru_cache(maxsize=None)
def dense(origin=(0, 0, 0)):
    """3 x 3 x 3 blocks from block `origin`: every voxel contributes (weights 2 .. 40, so none is fresh)"""
    rng = np.random.default_rng([int(v) + 4096 for v in origin])
    n = 27
    t = rng.uniform(-1, 1, (n, 512)).astype(F)
    c = np.zeros((n, 512), dtype=RGBW_DTYPE)
    for ch in ("r", "g", "b"):
        c[ch] = rng.integers(0, 256, (n, 512))
    c["weight"] = rng.integers(2, 41, (n, 512))
    p = rng.uniform(0.02, 0.98, (n, 512)).astype(F)
    return (GRID3 + np.asarray(origin, dtype=np.int64)).astype(np.int16), t, c, p


def _place(block_set, xyz, voxels):
    """write Voxels rows at global voxel coordinates xyz [(k, 3)] of a block set (all inside it)"""
    pos, t, c, p = block_set
    where = {int(k): i for i, k in enumerate(fuse_ref.keys(pos))}
    xyz = np.asarray(xyz, dtype=np.int64)
    b = np.array([where[int(k)] for k in fuse_ref.keys(xyz >> 3)])
    v = (xyz[:, 0] & 7) + 8 * (xyz[:, 1] & 7) + 64 * (xyz[:, 2] & 7)
    t[b, v], c[b, v], p[b, v] = voxels.t, voxels.c, voxels.p


FRESH = fuse_ref.FRESH_TSDF_BITS
VALUE_TSDF = (0.0, -0.0, fc.DENORM_MIN, -fc.DENORM_MIN, fc.DENORM_MAX, -fc.DENORM_MAX, fc.FLT_MIN, 1.5, -3.0, 1e30,
              fc.FLT_MAX, -fc.FLT_MAX, fc.INF, -fc.INF, fc.NAN, FRESH - 1, FRESH + 1)  # (an int is a bit pattern)
VALUE_WEIGHTS = (1, 2, 254, 255)


@functools.lru_cache(maxsize=None)
def values():
    """2 x 2 x 2 blocks around the origin.  Ordinary voxels (tsdf in [-1, 1], weights 2 .. 40); every value of
    VALUE_TSDF at every weight of VALUE_WEIGHTS on scattered single voxels; 2 x 2 x 2 cells that are subnormal throughout
    at weight 255, FLT_MAX throughout at weight 1 and +-FLT_MAX alternating (sums that overflow, inf - inf); one fresh
    voxel.  The probability words are random bit patterns."""
    rng = np.random.default_rng(77)
    pos = np.array([(x, y, z) for z in (-1, 0) for y in (-1, 0) for x in (-1, 0)], dtype=np.int16)
    n = len(pos)
    t = rng.uniform(-1, 1, (n, 512)).astype(F)
    c = np.zeros((n, 512), dtype=RGBW_DTYPE)
    for ch in ("r", "g", "b"):
        c[ch] = rng.integers(0, 256, (n, 512))
    c["weight"] = rng.integers(2, 41, (n, 512))
    p = rng.integers(0, 1 << 32, (n, 512), dtype=np.uint64).astype(U32).view(F)
    s = (pos, t, c, p)
    corner = np.array([[(j >> a) & 1 for a in range(3)] for j in range(8)])
    sign = np.where(corner.sum(axis=1) & 1, -1.0, 1.0)
    taken = {(0, -7, 3)}
    for at, tv, w in (((2, 2, 2), np.where(sign > 0, fc.DENORM_MAX, fc.DENORM_MIN), 255),
                      ((-6, -6, -6), np.full(8, fc.FLT_MAX), 1),
                      ((4, -4, -6), sign * fc.FLT_MAX, 9),
                      ((-3, 5, 1), np.where(sign > 0, -fc.DENORM_MAX, 0.0), 255)):
        cell = fc.rows([(float(tv[j]), (10 + j, 20 + j, 30 + j, w), 0.5) for j in range(8)])
        cell.p.view(U32)[:] = rng.integers(0, 1 << 32, 8, dtype=np.uint64).astype(U32)
        _place(s, np.asarray(at) + corner, cell)
        taken |= {tuple(v) for v in (np.asarray(at) + corner).tolist()}
    _place(s, [(0, -7, 3)], fc.rows([(FRESH, (1, 2, 3, 1), 0.5)]))
    special = fc.rows([(tv, (7 * i & 255, 200 - i, 3 * i & 255, w), 0.25) for i, (tv, w) in
                       enumerate((tv, w) for tv in VALUE_TSDF for w in VALUE_WEIGHTS)])
    k = len(special.t)
    cells = rng.permutation(16 ** 3)
    xyz = np.stack([cells & 15, (cells >> 4) & 15, cells >> 8], axis=1) - 8
    xyz = np.array([v for v in xyz.tolist() if tuple(v) not in taken][:k])  # distinct voxels, none of the above
    special.p.view(U32)[:] = rng.integers(0, 1 << 32, k, dtype=np.uint64).astype(U32)
    _place(s, xyz, special)
    return s


@functools.lru_cache(maxsize=None)
def chained(n=600):
    """(filler set, dense set, seed): the dense source at the origin and `n` filler blocks around it for a source engine
    with 512 buckets.  A bucket has two entries of its own and a chained block takes the first entry of a bucket that
    is still empty, so such a directory is full near 700 blocks (fuse_cases.chained fits; 727 did not: import_blocks
    returned RATSDF_ERR_CAPACITY): 627 leave room.  No home bucket holds more than 8 of them; the fillers go in first
    (`chained_imports`), so a dense block that shares its home bucket with a filler sits behind it."""
    d = dense()
    for seed in range(300, 400):
        pos = fc.case_positions(n + 60, seed)
        pos = pos[~np.isin(fuse_ref.keys(pos), fuse_ref.keys(d[0]))][:n]
        if np.unique(fc.home_buckets(np.concatenate([pos, d[0]]), 9), return_counts=True)[1].max() <= fc.PASSES:
            break
    else:
        raise AssertionError("no seed gives at most 8 per bucket")
    return fc.craft(pos, seed=83), d, seed


def chained_imports(step=100):
    """the chained source as the calls of import_blocks that build it: the fillers a hundred at a time, then the dense
    blocks one by one (an insertion can lose a pass to another one of the same call, and import_blocks makes 8 passes:
    small calls keep well clear of that)"""
    filler, d, _ = chained()
    return ([tuple(a[lo:lo + step] for a in filler) for lo in range(0, len(filler[0]), step)]
            + [tuple(a[i:i + 1] for a in d) for i in range(len(d[0]))])


def join(a, b):
    return tuple(np.concatenate([x, y]) for x, y in zip(a, b))


def source(key):
    """key: ("dense", (ox, oy, oz)) | ("sparse_straddle",) | ("sparse_lone",) | ("values",) | ("chained",)"""
    if key[0] == "dense":
        return dense(tuple(key[1]))
    if key[0] == "sparse_straddle":
        return _sparse(tuple((x, y, z) for z in (-1, 0) for y in (-1, 0) for x in (-1, 0)), 11)
    if key[0] == "sparse_lone":
        return _sparse(((0, 0, 0),), 12)
    if key[0] == "values":
        return values()
    if key[0] == "chained":
        return join(*chained()[:2])
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def _sparse(positions, seed):
    return fc.craft(positions, seed=seed)


def centre(key):
    """the middle of the source in voxels (what the poses without a shift turn about)"""
    if key[0] in ("dense", "chained"):
        o = key[1] if key[0] == "dense" else (0, 0, 0)
        return tuple(8.0 * v + 11.5 for v in o)
    return (-0.5, -0.5, -0.5) if key[0] != "sparse_lone" else (3.5, 3.5, 3.5)


# ---------------------------------------------------------------------------------------------------------------------
# cases
class Case(NamedTuple):
    name: str
    key: tuple    # of source()
    pose_name: str
    pose: tuple
    vs: float


def case(key, pose_name):
    tag = key[0] if key[0] != "dense" else "dense" + str(list(key[1])).replace(" ", "")
    return Case(f"{tag}|{pose_name}", key, pose_name, pose_of(pose_name, centre(key)), POSES[pose_name].vs)


ORIGIN = ("dense", (0, 0, 0))
END_POSES = {ENDS[0]: ("worst_x_inv", "worst_x_inv_down", "worst_x_inv_up"),
             ENDS[1]: ("worst_y_fwd", "worst_y_fwd_up", "worst_y_fwd_down", "third_111+none"),
             ENDS[2]: ("worst_z_inv", "worst_z_fwd_down")}
DENSE_CASES = tuple(case(ORIGIN, n) for n in names("worst", "scaled", "lattice", "quarter", "diagonal"))
END_CASES = tuple(case(("dense", e), n) for e in ENDS for n in END_POSES[e])
TIE_CASES = tuple(case((k,), n) for k in ("sparse_straddle", "sparse_lone") for n in names("lattice", "quarter"))
VALUE_CASES = tuple(case(("values",), n) for n in ("third_111+whole", "half_z+eps", "half_x+half_x", "half_y+half_xyz",
                                                  "quarter_z+whole", "diag_xy"))
RECORD_CASES = DENSE_CASES + END_CASES
ALL_CASES = RECORD_CASES + TIE_CASES + VALUE_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
WHOLE_CASES = (case(ORIGIN, "worst_x_inv"), case(("dense", ENDS[1]), "worst_y_fwd_up"), case(("chained",), "diag_z"))
CANDIDATE_LIMIT = 600


@functools.lru_cache(maxsize=None)
def expected(name):
    """(candidate blocks of the brute force, the restatement's block set over them, counts), once per process"""
    c = BY_NAME[name]
    src = source(c.key)
    cand = rr.padded_blocks(c.pose, c.vs, src[0])
    want, cnt = rr.resample_blocks(c.pose, c.vs, cand, rr.set_lookup(src))
    return cand, want, cnt


def record_differences(rec, want_set):
    """[n, 1536] bool: the words of device records that differ from the restatement's.  Bit for bit, but where the
    restatement's tsdf is NaN any NaN will do (sign and payload are the processor's)"""
    w = rr.records(want_set)
    bad = np.asarray(rec, dtype=U32) != w
    nan = np.isnan(w[:, :512].view(F)) & np.isnan(np.ascontiguousarray(rec[:, :512], dtype=U32).view(F))
    bad[:, :512] &= ~nan
    return bad


def crafted_destination(res_pos, seed):
    """a destination that holds every other block of `res_pos` and two blocks of its own (at a corner of the grid that
    no case reaches)"""
    own = np.array([(-4000, 4000, -4000), (-4001, 4000, -4000)], dtype=np.int16)
    return fc.craft(np.concatenate([np.asarray(res_pos, dtype=np.int16)[::2], own]), seed=seed)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement once more, with a switch per wrong line, and its inner values handed out
def resample_with(pose, vs, block_pos, lookup, *, reach_limit=None, rounding="away", wmin_all=False,
                  unneeded_read=False, unneeded_veto=False, l_max=32766, u_float64=False, normalise_q=False,
                  flush=False):
    """rr.resample_blocks with switches for the wrong lines: (block set, counts, inner values).  `reach_limit`: the
    kernel's table modelled with columns 0 .. reach_limit from 8 * base (base = the smallest floor of the block's
    in-range voxels >> 3); a corner beyond reads as absent.  None: no table, the contract."""
    pos = np.asarray(block_pos, dtype=np.int16).reshape(-1, 3)
    n = len(pos)
    m = 512 * n
    G = rr.transform(pose, vs)
    if normalise_q:  # WRONG
        q = G[0]
        with np.errstate(all="ignore"):
            s = np.sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]))
            G = (tuple(v / s for v in q), G[1])
    d = rr.block_voxels(pos)
    with np.errstate(all="ignore"):
        g = np.stack(rr.se3_apply(G, tuple(d[:, a].astype(F) for a in range(3))), axis=1)
        l = np.floor(g)
        ok = np.all(np.isfinite(g) & (l >= F(-32768)) & (l <= F(l_max)), axis=1)
    g, l = np.where(ok[:, None], g, F(0)), np.where(ok[:, None], l, F(0))
    f = g - l
    u = F(1) - f
    if u_float64:  # WRONG: 1 - (g - l) in float64, where the fraction of g = -1e-9 does not round to 1
        u = (1.0 - (g.astype(np.float64) - l.astype(np.float64))).astype(F)
    li = l.astype(np.int64)
    rnd = {"away": round_half_away, "even": np.rint, "floor_half": lambda x: np.floor(x + F(0.5))}[rounding]
    near = (rnd(g) != l).astype(np.int64)
    factor_ok = (u != 0, f != 0)
    need = np.empty((8, m), dtype=bool)
    corners = np.empty((8, m, 3), dtype=np.int64)
    for k in range(8):
        i, j, q = k >> 2, (k >> 1) & 1, k & 1
        need[k] = factor_ok[i][:, 0] & factor_ok[j][:, 1] & factor_ok[q][:, 2]
        corners[k] = li + np.array([i, j, q])
    # the table of the kernel
    any_ok = ok.reshape(n, 512).any(axis=1)
    lowest = np.where(ok[:, None], li, np.iinfo(np.int64).max).reshape(n, 512, 3).min(axis=1)
    base = np.where(any_ok[:, None], lowest >> 3, 0)
    rel = corners - 8 * np.repeat(base, 512, axis=0)[None]
    in_range = np.all((corners >= -32768) & (corners <= 32767), axis=2)
    alloc, t, c, p = lookup(np.clip(corners, -32768, 32767).reshape(-1, 3))
    alloc = np.asarray(alloc, dtype=bool).reshape(8, m) & in_range
    if reach_limit is not None:
        alloc &= np.all((rel >= 0) & (rel <= reach_limit), axis=2)
    t = np.asarray(t, dtype=F).reshape(8, m)
    c = np.asarray(c, dtype=RGBW_DTYPE).reshape(8, m)
    p = np.asarray(p, dtype=F).reshape(8, m)
    good = alloc & fuse_ref.contributes(t, c)
    looked_at = np.ones_like(need) if unneeded_veto else need  # (all eight: WRONG)
    contrib = ok & np.all(~looked_at | good, axis=0)
    tt = t if unneeded_read else np.where(need, t, F(0))      # (the voxel read instead of 0: WRONG)
    weight = np.where(alloc, c["weight"], 0)
    wmin = np.where(np.ones_like(need) if wmin_all else need, weight, 255).min(axis=0).astype(np.uint8)

    def mul(a, b):
        with np.errstate(all="ignore"):
            r = (a * b).astype(F)
            if flush:  # WRONG: a subnormal product reads as zero
                r = np.where(np.abs(r) < F(fc.FLT_MIN), np.copysign(F(0), r), r)
        return r
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    with np.errstate(all="ignore"):
        c00, c01 = mul(tt[0], uz) + mul(tt[1], fz), mul(tt[2], uz) + mul(tt[3], fz)
        c10, c11 = mul(tt[4], uz) + mul(tt[5], fz), mul(tt[6], uz) + mul(tt[7], fz)
        c0, c1 = mul(c00, uy) + mul(c01, fy), mul(c10, uy) + mul(c11, fy)
        ts = mul(c0, ux) + mul(c1, fx)
    assert ts.dtype == F
    kn = (near[:, 0] << 2) | (near[:, 1] << 1) | near[:, 2]
    cols = np.arange(m)
    rc = c[kn, cols].copy()
    rc["weight"] = wmin
    rt, rp = ts.copy(), p[kn, cols].copy()
    rt[~contrib], rp[~contrib] = F(0), F(0)
    rc[~contrib] = np.zeros(1, dtype=RGBW_DTYPE)
    live = (need & ok[None])[:, :, None]
    inner = dict(g=g, l=li, f=f, ok=ok, need_n=need.sum(axis=0), kn=kn, contrib=contrib, base=base, any_ok=any_ok,
                 wmin=wmin, tsdf=rt,
                 reach=np.where(live, rel, -1).reshape(8, n, 512, 3).max(axis=(0, 2)) if n else np.zeros((0, 3), int))
    out = (pos, rt.reshape(n, 512), rc.reshape(n, 512), rp.reshape(n, 512))
    return out, contrib.reshape(n, 512).sum(axis=1).astype(np.int32), inner


# each: the switch, and the cases to try it on
def _named(cases, want, limit=4):
    return [c.name for c in cases if want(c)][:limit]


_half = lambda c: "+half_" in c.name and c.key[0] == "sparse_straddle" and POSES[c.pose_name].family == "lattice"
MISTAKES = {
    "the table limited to reach 20": (dict(reach_limit=20), _named(RECORD_CASES, lambda c: "worst_y" in c.name, 8)),
    "roundf as round-half-even": (dict(rounding="even"), _named(TIE_CASES, _half)),
    "roundf as floor(g + 0.5)": (dict(rounding="floor_half"), _named(TIE_CASES, _half)),
    "the smallest weight over all eight corners": (dict(wmin_all=True), _named(TIE_CASES, lambda c: True)),
    "a corner that is not needed read instead of 0": (dict(unneeded_read=True), _named(VALUE_CASES, lambda c: True)),
    "a corner that is not needed can veto":
        (dict(unneeded_veto=True), _named(TIE_CASES, lambda c: c.key[0] == "sparse_lone")),
    "the range test on l <= 32767": (dict(l_max=32767), _named(END_CASES, lambda c: c.key[1] == ENDS[1])),
    "u as 1 - f in float64": (dict(u_float64=True), _named(TIE_CASES, lambda c: c.name.endswith("+eps"))),
    "G.q normalised": (dict(normalise_q=True), _named(RECORD_CASES, lambda c: c.name.endswith(("_up", "_down")))),
    "subnormal products flushed to zero": (dict(flush=True), _named(VALUE_CASES, lambda c: True)),
}


def same_records(x_set, x_cnt, y_set, y_cnt):
    return bool(np.array_equal(x_cnt, y_cnt) and not record_differences(rr.records(x_set), y_set).any())


def failing_cases(mistake):
    """the names of the cases (among those named for it) whose expected records differ under `mistake`"""
    kw, tried = MISTAKES[mistake]
    out = []
    for name in tried:
        c = BY_NAME[name]
        cand, want, cnt = expected(name)
        wrong, wrong_cnt, _ = resample_with(c.pose, c.vs, cand, rr.set_lookup(source(c.key)), **kw)
        if not same_records(wrong, wrong_cnt, want, cnt):
            out.append(name)
    return out


def half_z_half_x_by_hand(src):
    """{destination voxel: (tsdf, rgbw, prob)} of `src` under half_z+half_x, worked without the restatement: half_z
    turns (x, y, z) to (-x, -y, z), so with the shift (0.5, 0, 0) destination voxel d samples g = (-dx - 0.5, -dy, dz):
    l = -dx - 1 and f = u = 0.5 on x, the lattice itself on y and z.  roundf is half away from zero: for g < 0
    (dx >= 0) the nearest voxel is the floor -dx - 1, for g > 0 (dx <= -1) it is floor + 1 = -dx.  Also returns how
    many of the voxels have g < 0 and g > 0."""
    pos, t, c, p = src
    live = fuse_ref.contributes(t, c).reshape(-1)
    xyz = rr.block_voxels(pos)
    tab = {tuple(v): i for v, i in zip(xyz[live].tolist(), np.flatnonzero(live).tolist())}
    t, c, p = t.reshape(-1), c.reshape(-1), p.reshape(-1)
    out, n_neg, n_pos = {}, 0, 0
    lo_x, hi_x = int(xyz[:, 0].min()), int(xyz[:, 0].max())
    for (x, y, z), hi in tab.items():  # hi = source voxel -dx
        lo = tab.get((x - 1, y, z))    # source voxel -dx - 1
        if lo is None:
            continue
        dx = -x
        near = lo if dx >= 0 else hi
        col = c[near].copy()
        col["weight"] = min(c[lo]["weight"], c[hi]["weight"])
        out[(dx, -y, z)] = (F(t[lo] * F(0.5) + t[hi] * F(0.5)), col, p[near])
        n_neg, n_pos = n_neg + (dx >= 0), n_pos + (dx < 0)
    assert lo_x < 0 < hi_x
    return out, n_neg, n_pos
