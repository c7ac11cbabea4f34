"""The label score of include/ratsdf_score.h restated in numpy: the contract of ratsdf_score_labels[_device].

score(): brute force over all pairs (selected voxel, kept point) in float32 with the header's expression order,
lexicographic argmin over (d2, original index), then the counts.  The voxels are given in gather order (the rows of a
BlockSet picked by an engine's directory dump: tests/query_cases.rows_of), so nothing here asks an engine for a value.

The keyword arguments of score() and of grid_nearest() switch on the WRONG variants that tests/test_score_cases.py shows
the crafted cases tell apart from the contract; grid_nearest() is a per-voxel grid search of the kind the device runs
(rings of cells, a conservative stopping bound), there to carry the two variants that only a grid can get wrong.
"""
import numpy as np

from query_cases import LOCAL, wrap16
from ratsdf._abi import LABEL_SCORE_DTYPE, VOXEL_LABEL_DTYPE

F = np.float32
QNAN_BITS = 0x7FC00000
IGNORE, LOW, HIGH = 0, 1, 2


def voxel_positions(pos, vs):
    """[n, 512, 3] float32: (float)grid_index * voxel_size of every voxel of the blocks at `pos`, grid index =
    (short)((short)(block << 3) + local)"""
    g = wrap16(wrap16(np.asarray(pos).astype(np.int64).reshape(-1, 3) << 3)[:, None, :] + LOCAL[None])
    return g.astype(F) * F(vs)


def kept_points(points):
    """indices of the points with three finite coordinates"""
    return np.flatnonzero(np.isfinite(np.asarray(points, dtype=F).reshape(-1, 3)).all(axis=1))


def pair_d2(q, p, fma=False):
    """d2 of the header for queries q [m, 1, 3] against points p [1, k, 3], float32.  fma (WRONG): the sums contracted
    into fused multiply-adds, d2 = fma(dz, dz, fma(dy, dy, dx * dx)), emulated in float64"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = (p - q).astype(F)
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        if fma:
            inner = (dy.astype(np.float64) * dy.astype(np.float64) + (dx * dx).astype(np.float64)).astype(F)
            return (dz.astype(np.float64) * dz.astype(np.float64) + inner.astype(np.float64)).astype(F)
        return ((dx * dx + dy * dy).astype(F) + dz * dz).astype(F)


def nearest(q, points, max_dist, ties_highest=False, fma=False):
    """for float32 queries q [m, 3]: (original index or -2, d2) of the point that minimises (d2, index) among the kept
    points with d2 <= max_dist * max_dist.  ties_highest (WRONG): the highest index among equals"""
    points = np.asarray(points, dtype=F).reshape(-1, 3)
    keep = kept_points(points)
    md2 = F(max_dist) * F(max_dist)
    idx = np.full(len(q), -2, dtype=np.int64)
    best = np.full(len(q), np.inf, dtype=F)
    if len(keep) == 0 or len(q) == 0:
        return idx, best
    p = points[keep][None]
    step = max(1, (1 << 22) // len(keep))
    for a in range(0, len(q), step):
        d2 = pair_d2(q[a:a + step, None, :], p, fma)
        ok = (d2 <= md2).any(axis=1)
        d2 = np.where(d2 <= md2, d2, F(np.inf))
        lo = d2.min(axis=1)
        eq = d2 == lo[:, None]
        k = (eq.shape[1] - 1 - np.argmax(eq[:, ::-1], axis=1)) if ties_highest else np.argmax(eq, axis=1)
        idx[a:a + step] = np.where(ok, keep[k], -2)
        best[a:a + step] = lo
    return idx, best


def prob_bin(p):
    """bin(p) = p >= 1 ? 255 : p > 0 ? (int)(p * 256.0f) : 0.  round_ (WRONG) is in score()"""
    p = np.asarray(p, dtype=F)
    with np.errstate(invalid="ignore"):
        inner = np.where(p > 0, np.minimum(p * F(256), F(255)), F(0))
        return np.where(p >= 1, 255, np.nan_to_num(inner, nan=0.0).astype(np.int64)).astype(np.int64)


def score(pos, tsdf, weight, prob, vs, points, labels, tsdf_below=0.1, max_dist=1.0, p_cutoff=0.5, min_weight=0,
          select_le=False, ties_highest=False, fma=False, cutoff_ge=False, bin_round=False, nearest_fn=None):
    """(LABEL_SCORE_DTYPE record, VOXEL_LABEL_DTYPE [n * 512]) of the blocks at pos [n, 3] in the order given, with
    voxel arrays [n, 512].  The keywords after min_weight are the WRONG variants: `<=` selection, ties by highest
    index, contracted d2, `>=` cutoff, rounded bin; nearest_fn(q, points, max_dist) replaces the search."""
    pos = np.asarray(pos).reshape(-1, 3)
    n = len(pos)
    labels = np.asarray(labels, dtype=np.uint8).reshape(-1)
    t = np.ascontiguousarray(tsdf, dtype=F).reshape(-1)
    w = np.asarray(weight).reshape(-1).astype(np.int64)
    pr = np.ascontiguousarray(prob, dtype=F).reshape(-1)
    with np.errstate(invalid="ignore"):
        sel = (np.abs(t) <= F(tsdf_below)) if select_le else (np.abs(t) < F(tsdf_below))
    sel &= w >= int(min_weight)
    q = voxel_positions(pos, vs).reshape(-1, 3)
    rec = np.zeros(n * 512, dtype=VOXEL_LABEL_DTYPE)
    rec["nearest"] = -1
    rec["dist2"].view(np.uint32)[...] = QNAN_BITS
    s = np.flatnonzero(sel)
    if nearest_fn is None:
        idx, d2 = nearest(q[s], points, max_dist, ties_highest, fma)
    else:
        idx, d2 = nearest_fn(q[s], points, max_dist)
    rec["nearest"][s] = idx
    m = idx >= 0
    rec["dist2"][s[m]] = d2[m]
    out = np.zeros((), dtype=LABEL_SCORE_DTYPE)
    out["voxels"] = n * 512
    out["selected"] = len(s)
    out["unmatched"] = int((~m).sum())
    lab = labels[idx[m]]
    p = pr[s[m]]
    out["unannotated"] = int((lab == IGNORE).sum())
    ann = lab != IGNORE
    lab, p = lab[ann], p[ann]
    with np.errstate(invalid="ignore"):
        pred = (p >= F(p_cutoff)) if cutoff_ge else (p > F(p_cutoff))
    high = lab == HIGH
    out["confusion"] = [int((pred & high).sum()), int((pred & ~high).sum()), int((~pred & high).sum()),
                        int((~pred & ~high).sum())]
    if bin_round:
        with np.errstate(invalid="ignore"):
            b = np.clip(np.nan_to_num(np.rint(p.astype(np.float64) * 256.0), nan=0.0), 0, 255).astype(np.int64)
    else:
        b = prob_bin(p)
    np.add.at(out["hist"], (high.astype(np.int64), b), 1)
    return out, rec


def identities(rec):
    """the two sums the header states"""
    return (int(rec["selected"]) == int(rec["unmatched"]) + int(rec["unannotated"]) + int(rec["confusion"].sum()) and
            int(rec["hist"].sum()) == int(rec["confusion"].sum()))


# ---------------------------------------------------------------------------------------------------------------------
# a grid search, per voxel: cells of edge `cell` aligned to the world's origin, rings of growing Chebyshev radius.
def grid_nearest(q, points, max_dist, cell, truncate=False, first_hit=False):
    """nearest() through a grid.  After ring r everything in the cells within r of the query's has been looked at, so
    any other point is at least r * cell away along some axis: the search ends when the best d2 is below
    (r * cell * (1 - 1e-5))^2, or that bound exceeds max_dist^2.
    truncate (WRONG): the query's cell index by truncation towards zero, the points' by floor.
    first_hit (WRONG): ends after the first ring that held a point, whatever the bound says."""
    points = np.asarray(points, dtype=F).reshape(-1, 3)
    keep = kept_points(points)
    md2 = F(max_dist) * F(max_dist)
    cells = {}
    for i in keep:
        cells.setdefault(tuple(np.floor(points[i].astype(np.float64) / cell).astype(np.int64)), []).append(i)
    idx = np.full(len(q), -2, dtype=np.int64)
    best = np.full(len(q), np.inf, dtype=F)
    rings = int(np.ceil(float(max_dist) / cell)) + 2
    for j, v in enumerate(np.asarray(q, dtype=F)):
        u = v.astype(np.float64) / cell
        c = (np.trunc(u) if truncate else np.floor(u)).astype(np.int64)
        bi, bd = -2, F(np.inf)
        for r in range(rings + 1):
            cand = []
            for dx in range(-r, r + 1):
                for dy in range(-r, r + 1):
                    for dz in range(-r, r + 1):
                        if max(abs(dx), abs(dy), abs(dz)) == r:
                            cand += cells.get((c[0] + dx, c[1] + dy, c[2] + dz), [])
            if cand:
                cand = np.array(sorted(cand))
                for k, d in zip(cand, pair_d2(v[None, None, :], points[cand][None])[0]):
                    if d <= md2 and (bi < 0 or d < bd or (d == bd and k < bi)):
                        bi, bd = int(k), d
            bound = (r * cell * (1 - 1e-5)) ** 2
            if (first_hit and bi >= 0) or float(bd if bi >= 0 else md2) < bound:
                break
        idx[j], best[j] = bi, bd
    return idx, best
