"""numpy restatement of the resampling contract of include/ratsdf_resample.h (test infrastructure).

A block set is what tests/fuse_ref.py works on: (positions [n, 3] int16, tsdf [n, 512] float32, rgbw [n, 512]
RGBW_DTYPE, prob [n, 512] float32).  A pose is (qx, qy, qz, qw, tx, ty, tz), dst_T_src: p_dst = R(q) p_src + t.

quat_rotate / se3_apply / se3_inverse are restated operation by operation in float32 (device_math.h), the trilinear
formula is the one of tests/sample_ref.py.  The candidate search is NOT the engine's: `blocks_with_contribution` is a
brute force over a padded box per source block (the float64 inverse of the map G itself defines, `forward_map`, two
voxels of padding), every voxel of every block in it evaluated."""
import numpy as np

import fuse_ref
from ratsdf._abi import RGBW_DTYPE
from sample_ref import round_half_away

F = np.float32
RECORD_WORDS = 1536


# ---- pose arithmetic (device_math.h), float32, one rounding per operation ---------------------------------------
def cross3(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def quat_rotate(q, v):
    """q = (x, y, z, w) float32 scalars, v = three float32 scalars or arrays"""
    qv = (q[0], q[1], q[2])
    uv = cross3(qv, v)
    uv = tuple(c + c for c in uv)
    c = cross3(qv, uv)
    return tuple((v[i] + q[3] * uv[i]) + c[i] for i in range(3))


def se3_apply(T, v):
    r = quat_rotate(T[0], v)
    return tuple(r[i] + T[1][i] for i in range(3))


def se3_inverse(T):
    q, t = T
    n2 = (q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3])
    if n2 > F(0):
        qi = ((-q[0]) / n2, (-q[1]) / n2, (-q[2]) / n2, q[3] / n2)
    else:
        qi = (F(0),) * 4
    return qi, quat_rotate(qi, (-t[0], -t[1], -t[2]))


def as_se3(pose):
    p = [F(v) for v in pose]
    assert len(p) == 7
    return tuple(p[:4]), tuple(p[4:])


def pose_ok(pose):
    """what the entry points accept: finite components, | |q|^2 - 1 | <= 1e-3"""
    p = np.array([F(v) for v in pose], dtype=np.float64)
    return bool(np.all(np.isfinite(p)) and abs(float(np.sum(p[:4] * p[:4])) - 1.0) <= 1e-3)


def transform(pose, vs):
    """G of the contract: the inverse pose in voxel units"""
    vs = F(vs)
    with np.errstate(all="ignore"):
        qi, ti = se3_inverse(as_se3(pose))
        return qi, tuple(c / vs for c in ti)


# ---- the source map ------------------------------------------------------------------------------------------
def set_lookup(block_set):
    """lookup(v): (m, 3) int voxel coordinates inside the int16 range -> (allocated, tsdf, rgbw, prob)"""
    pos, t, c, p = block_set
    t = np.ascontiguousarray(t, dtype=F).reshape(-1)
    c = np.ascontiguousarray(c, dtype=RGBW_DTYPE).reshape(-1)
    p = np.ascontiguousarray(p, dtype=F).reshape(-1)
    k = fuse_ref.keys(pos) if len(pos) else np.zeros(0, dtype=np.int64)
    assert len(np.unique(k)) == len(k)
    order = np.argsort(k, kind="stable")
    ks = k[order]

    def lookup(v):
        v = np.asarray(v, dtype=np.int64)
        if len(ks) == 0:
            m = len(v)
            return np.zeros(m, dtype=bool), np.zeros(m, dtype=F), np.zeros(m, dtype=RGBW_DTYPE), np.zeros(m, dtype=F)
        kk = fuse_ref.keys(v >> 3)
        i = np.minimum(np.searchsorted(ks, kk), len(ks) - 1)
        found = ks[i] == kk
        at = np.where(found, order[i] * 512 + (v[:, 0] & 7) + 8 * (v[:, 1] & 7) + 64 * (v[:, 2] & 7), 0)
        return found, t[at], c[at], p[at]
    return lookup


# ---- the contract --------------------------------------------------------------------------------------------
def resample_voxels(G, d, lookup):
    """destination voxels d [(m, 3) int] -> (tsdf f32[m], rgbw[m], prob f32[m], contributes bool[m]); a voxel that
    does not contribute is all zeros"""
    d = np.asarray(d, dtype=np.int64).reshape(-1, 3)
    m = len(d)
    o_t, o_c, o_p = np.zeros(m, dtype=F), np.zeros(m, dtype=RGBW_DTYPE), np.zeros(m, dtype=F)
    o_ok = np.zeros(m, dtype=bool)
    with np.errstate(all="ignore"):
        g = np.stack(se3_apply(G, tuple(d[:, a].astype(F) for a in range(3))), axis=1)
        assert g.dtype == F
        l = np.floor(g)
        ok = np.all(np.isfinite(g) & (l >= F(-32768)) & (l <= F(32766)), axis=1)
    if not ok.any():
        return o_t, o_c, o_p, o_ok
    g, l = g[ok], l[ok]
    f = g - l
    u = F(1) - f
    li = l.astype(np.int64)
    near = (round_half_away(g) != l).astype(np.int64)
    n = len(g)
    factor_ok = (u != F(0), f != F(0))  # [corner index][:, axis]
    need = np.empty((8, n), dtype=bool)
    corners = np.empty((8, n, 3), dtype=np.int64)
    for k in range(8):
        i, j, q = k >> 2, (k >> 1) & 1, k & 1
        need[k] = factor_ok[i][:, 0] & factor_ok[j][:, 1] & factor_ok[q][:, 2]
        corners[k] = li + np.array([i, j, q])
    alloc, t, c, p = lookup(corners.reshape(-1, 3))
    alloc = np.asarray(alloc, dtype=bool).reshape(8, n)
    t = np.asarray(t, dtype=F).reshape(8, n)
    c = np.asarray(c, dtype=RGBW_DTYPE).reshape(8, n)
    p = np.asarray(p, dtype=F).reshape(8, n)
    good = alloc & fuse_ref.contributes(t, c)
    contrib = np.all(~need | good, axis=0)
    t = np.where(need, t, F(0))  # a corner that is not needed reads as 0.0f
    wmin = np.where(need, c["weight"], 255).min(axis=0).astype(np.uint8)
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    with np.errstate(all="ignore"):
        c00 = t[0] * uz + t[1] * fz
        c01 = t[2] * uz + t[3] * fz
        c10 = t[4] * uz + t[5] * fz
        c11 = t[6] * uz + t[7] * fz
        c0 = c00 * uy + c01 * fy
        c1 = c10 * uy + c11 * fy
        ts = c0 * ux + c1 * fx
    assert ts.dtype == F
    kn = (near[:, 0] << 2) | (near[:, 1] << 1) | near[:, 2]
    cols = np.arange(n)
    assert need[kn, cols].all()  # the nearest voxel is always a needed corner
    rc = c[kn, cols].copy()
    rc["weight"] = wmin
    rt, rp = ts.copy(), p[kn, cols].copy()
    rt[~contrib], rp[~contrib] = F(0), F(0)
    rc[~contrib] = np.zeros(1, dtype=RGBW_DTYPE)
    o_t[ok], o_c[ok], o_p[ok], o_ok[ok] = rt, rc, rp, contrib
    return o_t, o_c, o_p, o_ok


def block_voxels(block_pos):
    """integer grid indices of the voxels of blocks [n, 3], in record order (x + 8y + 64z): (n * 512, 3)"""
    b = np.asarray(block_pos, dtype=np.int64).reshape(-1, 3)
    v = np.arange(512)
    local = np.stack([v & 7, (v >> 3) & 7, v >> 6], axis=1)
    return (b[:, None, :] * 8 + local[None, :, :]).reshape(-1, 3)


def resample_blocks(pose, vs, block_pos, lookup):
    """ratsdf_resample_blocks_device restated: (block set of the listed destination blocks, counts int32[n])"""
    pos = np.asarray(block_pos, dtype=np.int16).reshape(-1, 3)
    n = len(pos)
    t, c, p, ok = resample_voxels(transform(pose, vs), block_voxels(pos), lookup)
    return (pos, t.reshape(n, 512), c.reshape(n, 512), p.reshape(n, 512)), ok.reshape(n, 512).sum(axis=1).astype(np.int32)


def records(block_set):
    """the block set as the words of n device records {tsdf[512] | rgbw[512] | prob[512]}: (n, 1536) uint32"""
    _, t, c, p = block_set
    return np.concatenate([np.ascontiguousarray(t, dtype=F).view(np.uint32),
                           np.ascontiguousarray(c, dtype=RGBW_DTYPE).view(np.uint32).reshape(len(t), 512),
                           np.ascontiguousarray(p, dtype=F).view(np.uint32)], axis=1)


# ---- brute force: which destination blocks hold a contributing voxel -----------------------------------------
def forward_map(pose, vs):
    """the map the contract defines, turned round: a destination voxel d samples the source at g = A d + c with A the
    linear part of quat_rotate(G.q, .) and c = G.t, so a source point g lands on d = A^-1 (g - c).  Taken from G itself
    (float32, as the kernel gets it) in float64 -- NOT from the normalised pose: A = I + (R^T - I) / |q|^2 is no
    rotation when |q|^2 != 1, and 1e-3 of scale is 32 voxels at the end of the grid.  Returns (A^-1 [3, 3], c [3]),
    or None when c is not finite (no voxel is in range then)."""
    q, c = transform(pose, vs)
    x, y, z, w = (float(v) for v in q)
    c = np.array([float(v) for v in c], dtype=np.float64)
    if not (np.all(np.isfinite(c)) and np.all(np.isfinite([x, y, z, w]))):
        return None
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])  # qv x .
    A = np.eye(3) + 2.0 * w * K + 2.0 * (K @ K)              # v + w * 2 (qv x v) + qv x 2 (qv x v)
    return np.linalg.inv(A), c


def padded_blocks(pose, vs, src_pos, pad=2.0):
    """every destination block inside [-4096, 4095] that holds an integer voxel of the box around a source block's
    reach [8b - 1, 8b + 8], taken through `forward_map` (float64) and padded by `pad` voxels -- the padding covers the
    float32 evaluation of g alone (under 0.2 voxel at the end of the grid); distinct, sorted by (z, y, x)"""
    fm = forward_map(pose, vs)
    if fm is None:
        return np.zeros((0, 3), dtype=np.int16)
    Ai, c = fm
    found = set()
    corner = np.array([[(k >> a) & 1 for a in range(3)] for k in range(8)], dtype=np.float64)
    for b in np.asarray(src_pos, dtype=np.int64).reshape(-1, 3):
        g = 8.0 * b[None, :] - 1.0 + 9.0 * corner
        d = (g - c) @ Ai.T
        lo = np.maximum(np.ceil(d.min(axis=0) - pad), -32768).astype(np.int64) >> 3
        hi = np.minimum(np.floor(d.max(axis=0) + pad), 32767).astype(np.int64) >> 3
        if np.any(lo > hi):
            continue
        for bz in range(lo[2], hi[2] + 1):
            for by in range(lo[1], hi[1] + 1):
                for bx in range(lo[0], hi[0] + 1):
                    found.add((bz, by, bx))
    out = np.array(sorted(found), dtype=np.int64).reshape(-1, 3)[:, ::-1]
    return np.ascontiguousarray(out).astype(np.int16)


def blocks_with_contribution(pose, vs, src_set, pad=2.0):
    """the resampled map: (block set of the destination blocks with at least one contributing voxel, their counts)"""
    cand = padded_blocks(pose, vs, src_set[0], pad)
    if len(cand) == 0:
        return fuse_ref.empty_set(), np.zeros(0, dtype=np.int32)
    s, cnt = resample_blocks(pose, vs, cand, set_lookup(src_set))
    keep = cnt > 0
    return tuple(a[keep] for a in s), cnt[keep]


def fuse_transformed(dst_set, src_set, pose, vs, shard=None):
    """ratsdf_fuse_map_transformed restated: resample, drop the empty blocks, fuse (tests/fuse_ref.py)"""
    res, _ = blocks_with_contribution(pose, vs, src_set)
    return fuse_ref.fuse(dst_set, res, shard)
