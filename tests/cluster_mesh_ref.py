"""numpy restatement of the clustered-mesh contract of include/ratsdf_cluster_mesh.h (test infrastructure).

`cluster_mesh(blocks, origin, dims, vs, factor, min_weight)` takes the map as surface_ref's dict (blocks_of) and returns
(vertices as surface_ref.POINT records, triangles int32 [n, 3]) in the header's orders.  Written in another shape than
the kernel: it starts from the welded mesh as LISTS (`welded`: surface_mesh_ref's dense-array construction, which also
keeps owner, axis and f of every vertex), the clusters are a dictionary from the cluster's coordinates to the list of
its members, the tree is an explicit np.float32 reduction over a dense k^3 array, and the triangles go through a Python
set and a sort by the header's key.

`Variant` plants ONE mistake a kernel could make per field; tests/test_cluster_mesh_ref.py shows on which named case
each one differs from the contract."""
from typing import NamedTuple

import numpy as np

import surface_mesh_ref as smr
import surface_ref as sr

F = np.float32
POINT = sr.POINT
_UNIT = np.eye(3, dtype=np.int64)
FACTORS = (2, 4, 8)


class Variant(NamedTuple):
    """the contract when every field is False"""
    sequential: bool = False       # the k^3 voxel sums added one after the other, j = 0, 1, 2, ...
    tie_gt: bool = False           # the upper endpoint iff f > 0.5f
    sort_triple: bool = False      # a triple sorted, not rotated: the winding is lost
    keep_duplicates: bool = False  # every surviving triple emitted
    world_pos: bool = False        # world positions summed, not positions relative to the cluster's base
    truncating_shift: bool = False  # the cluster of a voxel by a division that rounds towards zero


CONTRACT = Variant()


class Welded(NamedTuple):
    """the welded mesh of a box as lists, in the orders of ratsdf_surface_mesh.h"""
    vertices: np.ndarray           # sr.POINT
    triangles: np.ndarray          # [n, 3] int32
    owner: np.ndarray              # [v, 3] int64: the voxel that owns the vertex's edge
    axis: np.ndarray               # [v]
    f: np.ndarray                  # [v] float32: t0 / (t0 - t1)


def welded(blocks, origin, dims, vs, min_weight=1):
    """surface_mesh_ref.surface_mesh, and per vertex its edge and f: the owners of the crossings of the voxels
    [origin, origin + dims] in the header's order, picked down to those a complete cell of the box uses"""
    origin = np.array([int(v) for v in origin], dtype=np.int64)
    dims = np.array([int(v) for v in dims], dtype=np.int64)
    with np.errstate(all="ignore"):
        vertices, tri = smr.surface_mesh(blocks, origin, dims, vs, min_weight)
    X, Y, Z = (int(v) for v in dims)
    t, obs, _, _ = sr._dense(blocks, origin, origin + dims + 1, int(min_weight))
    neg = t < 0

    def sh(a, off, n=(X, Y, Z)):
        return a[off[2]:off[2] + n[2], off[1]:off[1] + n[1], off[0]:off[0] + n[0]]

    complete = np.ones((Z, Y, X), dtype=bool)
    for c in smr._CORNER:
        complete &= sh(obs, c)
    used = np.zeros((3,) + t.shape, dtype=bool)
    for e in range(12):
        sh(used[smr.EDGE_DIM[e]], smr._CORNER[smr.EDGE_LOWER[e]])[...] |= complete
    n1 = np.minimum(dims + 1, 32768 - origin)
    zero = np.zeros(3, dtype=np.int64)
    own, axis, fs = [], [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            t0, t1 = sh(t, zero, n1), sh(t, _UNIT[a], n1)
            cross = sh(obs, zero, n1) & sh(obs, _UNIT[a], n1) & (sh(neg, zero, n1) != sh(neg, _UNIT[a], n1))
            cross &= sh(used[a], zero, n1)
            z, y, x = np.nonzero(cross)
            own.append(np.stack([x, y, z], axis=1) + origin)
            axis.append(np.full(len(x), a))
            fs.append((t0 / (t0 - t1))[cross].astype(F))
    own, axis, fs = np.concatenate(own), np.concatenate(axis), np.concatenate(fs)
    order = smr._order(own, axis)
    own, axis, fs = own[order], axis[order], fs[order]
    assert len(own) == len(vertices)
    return Welded(vertices, tri, own, axis, fs)


def _tree(S, levels):
    """the header's fixed binary tree over axis 0 of S [2^levels, ...] float32: S[0] after the last level"""
    S = S.copy()
    j = np.arange(len(S))
    for l in range(levels):
        lower = j[(j & (1 << l)) == 0]                           # every j with bit l clear; the lower index on the left
        S[lower] = S[lower] + S[lower | (1 << l)]
    return S[0]


def _code(d):
    return int((d[0] + 1) + 3 * (d[1] + 1) + 9 * (d[2] + 1))


def cluster_of(u, s, variant=CONTRACT):
    u = np.asarray(u, dtype=np.int64)
    if variant.truncating_shift:
        return np.trunc(u / (1 << s)).astype(np.int64)
    return u >> s


def cluster_mesh(blocks, origin, dims, vs, factor=4, min_weight=1, variant=CONTRACT, mesh=None):
    k = int(factor)
    assert k in FACTORS
    s = {2: 1, 4: 2, 8: 3}[k]
    m = 8 >> s
    vs = F(vs)
    w = mesh if mesh is not None else welded(blocks, origin, dims, vs, min_weight)
    nv = len(w.vertices)
    up = (w.f > F(0.5)) if variant.tie_gt else (w.f >= F(0.5))
    chosen = w.owner + np.where(up[:, None], _UNIT[w.axis], 0) if nv else np.zeros((0, 3), np.int64)
    q = cluster_of(chosen, s, variant) if nv else np.zeros((0, 3), np.int64)

    # the clusters: a dictionary from q to the indices of its members
    clusters = {}
    for i in range(nv):
        clusters.setdefault(tuple(int(c) for c in q[i]), []).append(i)

    def order_key(c):
        blk = [c[b] >> (3 - s) for b in range(3)]
        l = [c[b] & (m - 1) for b in range(3)]
        return (blk[2], blk[1], blk[0], l[0] + m * l[1] + m * m * l[2])

    keys = sorted(clusters, key=order_key)
    index = {c: i for i, c in enumerate(keys)}
    out = np.zeros(len(keys), dtype=POINT)
    with np.errstate(all="ignore"):
        for ci, c in enumerate(keys):
            members = clusters[c]
            base = np.array(c, dtype=np.int64) << s
            # per voxel of the cluster, the members in the header's order: the axis, then owner u - e_a before owner u
            S = np.zeros((k * k * k, 7), dtype=F)                  # rel[3], normal[3], prob
            ints = np.zeros(4, dtype=np.int64)
            members = sorted(members, key=lambda i: (int(w.axis[i]), int(not up[i])))
            for i in members:
                a, f = int(w.axis[i]), w.f[i]
                u = chosen[i] - base
                if variant.truncating_shift:
                    u = u & (k - 1)
                j = int(u[0] + k * u[1] + k * k * u[2])
                val = np.zeros(7, dtype=F)
                for b in range(3):
                    if variant.world_pos:
                        pw = F(w.owner[i][b])
                        val[b] = ((pw + f) if b == a else pw) * vs
                    else:
                        rel = F(w.owner[i][b] - base[b])
                        val[b] = (rel + f) if b == a else rel
                val[3:6] = w.vertices["normal"][i]
                val[6] = w.vertices["prob"][i]
                S[j] = S[j] + val
                c4 = w.vertices["rgbw"][i]
                ints += np.array([c4["r"], c4["g"], c4["b"], c4["weight"]], dtype=np.int64)
            n = len(members)
            if variant.sequential:
                tot = np.zeros(7, dtype=F)
                for j in range(k * k * k):
                    tot = tot + S[j]
            else:
                tot = _tree(S, 3 * s)
            fn = F(n)
            for b in range(3):
                if variant.world_pos:
                    out["pos"][ci, b] = tot[b] / fn
                else:
                    out["pos"][ci, b] = (F(base[b]) + tot[b] / fn) * vs
            N = tot[3:6]
            ln = np.sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2])
            flat = (ln == 0) or not np.isfinite(ln)
            out["normal"][ci] = F(0) if flat else N / ln
            out["prob"][ci] = tot[6] / fn
            mean = (2 * ints + n) // (2 * n)
            assert (mean <= 255).all()
            out["rgbw"][ci] = tuple(int(x) for x in mean)

    # triangles: re-indexed, degenerate ones dropped, rotated, de-duplicated through a set, sorted by the header's key
    triples = []
    for tri in np.asarray(w.triangles):
        cs = [tuple(int(c) for c in q[i]) for i in tri]
        ids = [index[c] for c in cs]
        if ids[0] == ids[1] or ids[1] == ids[2] or ids[0] == ids[2]:
            continue
        if variant.sort_triple:
            r = sorted(range(3), key=lambda i: ids[i])
        else:
            first = ids.index(min(ids))
            r = [first, (first + 1) % 3, (first + 2) % 3]
        ids, cs = [ids[i] for i in r], [cs[i] for i in r]
        d2, d3 = np.subtract(cs[1], cs[0]), np.subtract(cs[2], cs[0])
        assert np.abs(d2).max() <= 1 and np.abs(d3).max() <= 1
        triples.append((ids[0], _code(d2), _code(d3), ids[1], ids[2]))
    if not variant.keep_duplicates:
        triples = set(triples)
    triples = sorted(triples)
    tri = np.array([(a, b, c) for a, _, _, b, c in triples], dtype=np.int32).reshape(-1, 3)
    return out, tri


def duplicates_removed(blocks, origin, dims, vs, factor, min_weight=1):
    """how many triples the duplicate removal takes out"""
    w = welded(blocks, origin, dims, vs, min_weight)
    a = cluster_mesh(blocks, origin, dims, vs, factor, min_weight, mesh=w)[1]
    b = cluster_mesh(blocks, origin, dims, vs, factor, min_weight, Variant(keep_duplicates=True), mesh=w)[1]
    return len(b) - len(a)


def differing(got, want):
    """how many records differ under the comparison rule of the awkward values: a float that is NaN on one side must be
    NaN on the other (any payload), every other word is equal bit for bit.  -1: the counts differ."""
    if got.dtype.itemsize != want.dtype.itemsize or got.shape != want.shape:
        return -1
    g = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), 8).copy()
    w_ = np.ascontiguousarray(want).view(np.uint32).reshape(len(want), 8).copy()
    gf, wf = g[:, :7].view(F), w_[:, :7].view(F)
    both = np.isnan(gf) & np.isnan(wf)
    g[:, :7][both] = 0
    w_[:, :7][both] = 0
    return int((g != w_).any(axis=1).sum())


def nan_count(rec):
    r = np.ascontiguousarray(rec).view(np.uint32).reshape(len(rec), 8)[:, :7].view(F)
    return int(np.isnan(r).sum())
