"""The label score against a mesh of include/ratsdf_score_mesh.h restated in numpy: the contract of
ratsdf_score_mesh[_device].

score(): brute force over all pairs (selected voxel, kept triangle) in float32 with the header's expression order
(tri_dist2: the closest point of Ericson 5.1.5, the first case that holds, then the clamp to the triangle's box),
lexicographic argmin over (dist2, original index), then the counts of ratsdf_score.h.  Voxel positions, the bins and
the record types are score_ref's; the voxels are given in gather order, so nothing here asks an engine for a value.

The keyword arguments switch on the WRONG variants that tests/test_score_mesh_cases.py shows the crafted cases tell
apart from the contract.  grid_nearest() is a per-voxel search over rings of cells in which a triangle counts for
every cell its axis-aligned box meets, with the conservative stopping bound the device uses; it carries the variants
that only a grid can get wrong.
"""
import numpy as np

from ratsdf._abi import LABEL_SCORE_DTYPE, VOXEL_LABEL_DTYPE
from score_ref import HIGH, IGNORE, LOW, QNAN_BITS, identities, prob_bin, voxel_positions  # noqa: F401

F = np.float32
D = np.float64
DIST_VARIANTS = ("nearest_vertex", "plane_distance", "box_distance", "no_clamp", "fma")


def as_mesh(vertices, triangles):
    return (np.ascontiguousarray(vertices, dtype=F).reshape(-1, 3),
            np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3))


def kept_triangles(vertices, triangles):
    """indices of the kept triangles (all indices are taken to be valid): nine finite coordinates, no two vertices
    equal in all three coordinates"""
    v, t = as_mesh(vertices, triangles)
    if len(t) == 0:
        return np.zeros(0, dtype=np.int64)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    finite = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(c).all(axis=1)
    with np.errstate(invalid="ignore"):
        same = (a == b).all(axis=1) | (a == c).all(axis=1) | (b == c).all(axis=1)
    return np.flatnonzero(finite & ~same)


def mixed_triangles(vertices, labels, triangles):
    """the number of kept triangles whose three vertex labels are not all equal"""
    v, t = as_mesh(vertices, triangles)
    k = kept_triangles(v, t)
    lab = np.asarray(labels, dtype=np.uint8)[t[k]]
    return int(((lab[:, 0] != lab[:, 1]) | (lab[:, 0] != lab[:, 2])).sum())


def dot(u, v, fma=False):
    """(ux * vx + uy * vy) + uz * vz in float32.  fma (WRONG): fma(uz, vz, fma(uy, vy, ux * vx)), emulated in float64"""
    if fma:
        inner = (u[..., 1].astype(D) * v[..., 1].astype(D) + (u[..., 0] * v[..., 0]).astype(D)).astype(F)
        return (u[..., 2].astype(D) * v[..., 2].astype(D) + inner.astype(D)).astype(F)
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def tri_dist2(p, a, b, c, variant=None, dtype=F):
    """dist2 of the header for positions p [m, 1, 3] against triangles a, b, c [1, k, 3]; every operation rounds to
    `dtype` (float32: the contract; float64: the independent check).  variant (WRONG): one of DIST_VARIANTS --
    the distance to the nearest of the three vertices, to the point of the "otherwise" formula without any region test
    or clamp, to the triangle's box, the contract without its final clamp, the contract with contracted dot products"""
    p, a, b, c = (np.asarray(x, dtype=dtype) for x in (p, a, b, c))
    fma = variant == "fma"
    with np.errstate(all="ignore"):
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        if variant == "nearest_vertex":
            d = [dot(x - p, x - p) for x in (a, b, c)]
            return np.minimum(np.minimum(d[0], d[1]), d[2])
        if variant == "box_distance":
            q = np.where(p < lo, lo, np.where(p > hi, hi, p + np.zeros_like(lo)))
            return dot(q - p, q - p)
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = dot(ab, ap, fma), dot(ac, ap, fma)
        bp = p - b
        d3, d4 = dot(ab, bp, fma), dot(ac, bp, fma)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = dot(ab, cp, fma), dot(ac, cp, fma)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e1, e2 = d4 - d3, d5 - d6
        one = np.asarray(1, dtype=dtype)
        den = one / ((va + vb) + vc)
        v7, w7 = vb * den, vc * den
        q = (a + ab * v7[..., None]) + ac * w7[..., None]
        if variant != "plane_distance":
            w6 = e1 / (e1 + e2)
            q = np.where(((va <= 0) & (e1 >= 0) & (e2 >= 0))[..., None], b + w6[..., None] * (c - b), q)
            w5 = d2 / (d2 - d6)
            q = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + w5[..., None] * ac, q)
            q = np.where(((d6 >= 0) & (d5 <= d6))[..., None], c, q)
            v3 = d1 / (d1 - d3)
            q = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + v3[..., None] * ab, q)
            q = np.where(((d3 >= 0) & (d4 <= d3))[..., None], b, q)
            q = np.where(((d1 <= 0) & (d2 <= 0))[..., None], a, q)
            if variant != "no_clamp":
                q = np.where(q < lo, lo, np.where(q > hi, hi, q))
        d = q - p
        return dot(d, d, fma)


def nearest(q, vertices, triangles, max_dist, ties_highest=False, variant=None):
    """for float32 queries q [m, 3]: (original index or -2, dist2) of the triangle that minimises (dist2, index) among
    the kept triangles with dist2 <= max_dist * max_dist.  ties_highest (WRONG): the highest index among equals"""
    v, t = as_mesh(vertices, triangles)
    keep = kept_triangles(v, t)
    md2 = F(max_dist) * F(max_dist)
    idx = np.full(len(q), -2, dtype=np.int64)
    best = np.full(len(q), np.inf, dtype=F)
    if len(keep) == 0 or len(q) == 0:
        return idx, best
    a, b, c = (v[t[keep, k]][None] for k in range(3))
    step = max(1, (1 << 19) // len(keep))
    for s in range(0, len(q), step):
        d2 = tri_dist2(q[s:s + step, None, :], a, b, c, variant)
        with np.errstate(invalid="ignore"):
            within = d2 <= md2
        ok = within.any(axis=1)
        d2 = np.where(within, d2, F(np.inf))
        lo = d2.min(axis=1)
        eq = d2 == lo[:, None]
        k = (eq.shape[1] - 1 - np.argmax(eq[:, ::-1], axis=1)) if ties_highest else np.argmax(eq, axis=1)
        idx[s:s + step] = np.where(ok, keep[k], -2)
        best[s:s + step] = lo
    return idx, best


def score(pos, tsdf, weight, prob, vs, vertices, labels, triangles, tsdf_below=0.1, max_dist=1.0, p_cutoff=0.5,
          min_weight=0, select_le=False, ties_highest=False, cutoff_ge=False, bin_round=False, variant=None,
          label_of=None, nearest_fn=None):
    """(LABEL_SCORE_DTYPE record, VOXEL_LABEL_DTYPE [n * 512]) of the blocks at pos [n, 3] in the order given, with
    voxel arrays [n, 512].  The keywords after min_weight are the WRONG variants: `<=` selection, ties by highest
    index, `>=` cutoff, rounded bin, a distance of DIST_VARIANTS, the triangle's label taken from its "last" vertex or
    from the vertex "nearest" to the voxel; nearest_fn(q, max_dist) replaces the search."""
    pos = np.asarray(pos).reshape(-1, 3)
    n = len(pos)
    v, t = as_mesh(vertices, triangles)
    labels = np.asarray(labels, dtype=np.uint8).reshape(-1)
    ts = np.ascontiguousarray(tsdf, dtype=F).reshape(-1)
    w = np.asarray(weight).reshape(-1).astype(np.int64)
    pr = np.ascontiguousarray(prob, dtype=F).reshape(-1)
    with np.errstate(invalid="ignore"):
        sel = (np.abs(ts) <= F(tsdf_below)) if select_le else (np.abs(ts) < F(tsdf_below))
    sel &= w >= int(min_weight)
    q = voxel_positions(pos, vs).reshape(-1, 3)
    rec = np.zeros(n * 512, dtype=VOXEL_LABEL_DTYPE)
    rec["nearest"] = -1
    rec["dist2"].view(np.uint32)[...] = QNAN_BITS
    s = np.flatnonzero(sel)
    if nearest_fn is None:
        idx, d2 = nearest(q[s], v, t, max_dist, ties_highest, variant)
    else:
        idx, d2 = nearest_fn(q[s], max_dist)
    rec["nearest"][s] = idx
    m = idx >= 0
    rec["dist2"][s[m]] = d2[m]
    out = np.zeros((), dtype=LABEL_SCORE_DTYPE)
    out["voxels"] = n * 512
    out["selected"] = len(s)
    out["unmatched"] = int((~m).sum())
    win = t[idx[m]].reshape(-1, 3)
    if label_of == "last":
        lab = labels[win[:, 2]]
    elif label_of == "nearest":
        with np.errstate(all="ignore"):
            d = np.stack([dot(v[win[:, k]] - q[s[m]], v[win[:, k]] - q[s[m]]) for k in range(3)], axis=1)
        lab = labels[win[np.arange(len(win)), np.argmin(d, axis=1)]] if len(win) else labels[:0]
    else:
        lab = labels[win[:, 0]]
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
            bins = np.clip(np.nan_to_num(np.rint(p.astype(D) * 256.0), nan=0.0), 0, 255).astype(np.int64)
    else:
        bins = prob_bin(p)
    np.add.at(out["hist"], (high.astype(np.int64), bins), 1)
    return out, rec


# ---------------------------------------------------------------------------------------------------------------------
# a grid search, per voxel: cells of edge `cell` aligned to the world's origin, rings of growing Chebyshev radius.  Cell
# indices are kept as float64 (whole numbers; exact below 2^53, monotone beyond), so coordinates of any size are filed.
def grid_nearest(q, vertices, triangles, max_dist, cell, truncate=False, first_hit=False, single_cell=False):
    """nearest() through a grid in which a kept triangle counts for every cell its axis-aligned box meets.  After ring
    r every triangle whose box meets a cell within r of the query's has been looked at, so the box of any other is at
    least r * cell away along some axis, and with it every point of the triangle the clamp can return: the search ends
    when the best dist2 is below (r * cell * (1 - 1e-5))^2, or that bound exceeds max_dist^2.
    truncate (WRONG): the query's cell index by truncation towards zero, the boxes' by floor.
    first_hit (WRONG): ends after the first ring that held a triangle within max_dist, whatever the bound says.
    single_cell (WRONG): a triangle is filed under the cell of its first vertex only."""
    v, t = as_mesh(vertices, triangles)
    keep = kept_triangles(v, t)
    md2 = F(max_dist) * F(max_dist)
    idx = np.full(len(q), -2, dtype=np.int64)
    best = np.full(len(q), np.inf, dtype=F)
    if len(keep) == 0:
        return idx, best
    a, b, c = (v[t[keep, k]] for k in range(3))
    if single_cell:
        lo = hi = np.floor(a.astype(D) / cell)
    else:
        lo = np.floor(np.minimum(np.minimum(a, b), c).astype(D) / cell)
        hi = np.floor(np.maximum(np.maximum(a, b), c).astype(D) / cell)
    rings = int(np.ceil(float(max_dist) / cell)) + 2
    for j, p in enumerate(np.asarray(q, dtype=F)):
        u = p.astype(D) / cell
        cq = np.trunc(u) if truncate else np.floor(u)
        bi, bd = -2, F(np.inf)
        before = np.zeros(len(keep), dtype=bool)
        for r in range(rings + 1):
            inside = ((lo <= cq + r) & (hi >= cq - r)).all(axis=1)
            cand = np.flatnonzero(inside & ~before)
            before = inside
            if len(cand):
                d = tri_dist2(p[None, None, :], a[cand][None], b[cand][None], c[cand][None])[0]
                for k, dk in zip(keep[cand], d):
                    if dk <= md2 and (bi < 0 or dk < bd or (dk == bd and k < bi)):
                        bi, bd = int(k), dk
            bound = (r * cell * (1 - 1e-5)) ** 2
            if (first_hit and bi >= 0) or float(bd if bi >= 0 else md2) < bound:
                break
        idx[j], best[j] = bi, bd
    return idx, best
