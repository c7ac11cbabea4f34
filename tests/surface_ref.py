"""numpy restatement of the surface-point contract of include/ratsdf_surface.h (test infrastructure).

`surface_points(blocks, origin, dims, vs, min_weight, min_prob)` takes the map as a dict: block position (bx, by, bz)
-> (tsdf [512] float32, rgbw [512] RGBW_DTYPE, prob [512] float32), voxel x + 8y + 64z, and returns the header's
records in the header's order.  Every step is the header's fp32 formula on float32 arrays (numpy rounds each operation
on its own: no contraction; its float32 sqrt and division are correctly rounded).  `blocks_of(pos, tsdf, rgbw, prob)`
builds the dict from import_blocks' / multi.export_blocks' arrays."""
import numpy as np

F = np.float32
RGBW = np.dtype([("r", "u1"), ("g", "u1"), ("b", "u1"), ("weight", "u1")])
POINT = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("prob", "<f4"), ("rgbw", RGBW)])
LO, HI = -32768, 32767


def blocks_of(pos, tsdf, rgbw, prob):
    pos = np.asarray(pos).reshape(-1, 3)
    n = len(pos)
    t = np.asarray(tsdf, dtype=np.float32).reshape(n, 512)
    c = np.asarray(rgbw, dtype=RGBW).reshape(n, 512)
    p = np.asarray(prob, dtype=np.float32).reshape(n, 512)
    return {tuple(int(v) for v in pos[i]): (t[i], c[i], p[i]) for i in range(n)}


def solid(lo, hi, fn, weight=3, prob=0.5):
    """import_blocks' arrays of every block in lo .. hi (block coordinates, inclusive): tsdf = fn(x, y, z) of the
    voxel indices (int64 arrays [n, 512]), one weight and probability, colour from the voxel index"""
    r = [np.arange(a, b + 1) for a, b in zip(lo, hi)]
    pos = np.stack(np.meshgrid(*r, indexing="ij"), -1).reshape(-1, 3).astype(np.int16)
    i = np.arange(512)
    loc = np.stack([i & 7, (i >> 3) & 7, i >> 6], -1)
    g = pos[:, None, :].astype(np.int64) * 8 + loc[None, :, :]
    tsdf = np.asarray(fn(g[..., 0], g[..., 1], g[..., 2]), dtype=np.float32)
    rgbw = np.zeros(tsdf.shape, dtype=RGBW)
    rgbw["r"], rgbw["g"], rgbw["b"] = g[..., 0] & 255, g[..., 1] & 255, g[..., 2] & 255
    rgbw["weight"] = weight
    return pos, tsdf, rgbw, np.full(tsdf.shape, prob, dtype=np.float32)


def _dense(blocks, lo, hi, min_weight):
    """tsdf, observed, prob and the rgbw word of the voxels lo .. hi (inclusive), arrays [z][y][x]"""
    shape = tuple(int(v) for v in (hi - lo + 1)[::-1])
    t = np.zeros(shape, dtype=np.float32)
    p = np.zeros(shape, dtype=np.float32)
    c = np.zeros(shape, dtype=np.uint32)
    obs = np.zeros(shape, dtype=bool)
    for b in range(3):                      # voxels beyond the int16 range are never observed
        assert lo[b] >= LO - 1 and hi[b] <= HI + 2
    blo, bhi = lo // 8, hi // 8
    for key, (bt, bc, bp) in blocks.items():
        k = np.array(key, dtype=np.int64)
        if np.any(k < blo) or np.any(k > bhi) or np.any(k < -4096) or np.any(k > 4095):
            continue
        g0 = k * 8 - lo                     # dense coordinates of the block's voxel (0, 0, 0)
        a = np.maximum(g0, 0)
        e = np.minimum(g0 + 8, hi - lo + 1)
        src = (slice(a[2] - g0[2], e[2] - g0[2]), slice(a[1] - g0[1], e[1] - g0[1]), slice(a[0] - g0[0], e[0] - g0[0]))
        dst = (slice(a[2], e[2]), slice(a[1], e[1]), slice(a[0], e[0]))
        bt = np.asarray(bt, dtype=np.float32).reshape(8, 8, 8)
        w = np.asarray(bc, dtype=RGBW)["weight"].reshape(8, 8, 8)
        fresh = (w == 1) & (bt.view(np.uint32) == 0xBF800000)
        t[dst] = bt[src]
        p[dst] = np.asarray(bp, dtype=np.float32).reshape(8, 8, 8)[src]
        c[dst] = np.ascontiguousarray(bc, dtype=RGBW).view(np.uint32).reshape(8, 8, 8)[src]
        obs[dst] = ((w >= min_weight) & ~fresh)[src]
    return t, obs, p, c


def surface_points(blocks, origin, dims, vs, min_weight=1, min_prob=0.0):
    origin = np.array([int(v) for v in origin], dtype=np.int64)
    dims = np.array([int(v) for v in dims], dtype=np.int64)
    vs, min_prob = F(vs), F(min_prob)
    lo, hi = origin - 1, origin + dims - 1 + 2      # the owners, one voxel below and two above
    t, obs, p, c = _dense(blocks, lo, hi, int(min_weight))
    X, Y, Z = (int(v) for v in dims)

    def sh(a, off):                                 # the array at owner + off (off: x, y, z)
        return a[1 + off[2]:1 + off[2] + Z, 1 + off[1]:1 + off[1] + Y, 1 + off[0]:1 + off[0] + X]

    unit = np.eye(3, dtype=np.int64)

    def diff(off, b):                               # d_b(owner + off)
        up, dn = sh(obs, off + unit[b]), sh(obs, off - unit[b])
        tu, td, tw = sh(t, off + unit[b]), sh(t, off - unit[b]), sh(t, off)
        return np.where(up & dn, (tu - td) * F(0.5), np.where(up, tu - tw, np.where(dn, tw - td, F(0))))

    zero = np.zeros(3, dtype=np.int64)
    vz, vy, vx = np.meshgrid(*[np.arange(origin[b], origin[b] + dims[b]) for b in (2, 1, 0)], indexing="ij")
    v = [vx, vy, vz]
    d0 = [diff(zero, b) for b in range(3)]
    t0 = sh(t, zero)
    parts = []
    with np.errstate(all="ignore"):
        for a in range(3):
            t1 = sh(t, unit[a])
            cross = sh(obs, zero) & sh(obs, unit[a]) & ((t0 < 0) != (t1 < 0))
            f = t0 / (t0 - t1)
            g = [d0[b] * (F(1) - f) + diff(unit[a], b) * f for b in range(3)]
            ln = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
            flat = (ln == 0) | ~np.isfinite(ln)
            up = f >= F(0.5)
            prob = np.where(up, sh(p, unit[a]), sh(p, zero))
            keep = cross & ~(prob < min_prob)
            rec = np.zeros(int(keep.sum()), dtype=POINT)
            for b in range(3):
                pos = ((v[b].astype(np.float32) + f) if b == a else v[b].astype(np.float32)) * vs
                rec["pos"][:, b] = pos[keep]
                rec["normal"][:, b] = np.where(flat, F(0), g[b] / ln)[keep]
            rec["prob"] = prob[keep]
            rec["rgbw"] = np.where(up, sh(c, unit[a]), sh(c, zero))[keep].view(RGBW)
            local = (vx & 7) + 8 * (vy & 7) + 64 * (vz & 7)
            key = np.stack([np.full(len(rec), a), local[keep], (vx >> 3)[keep], (vy >> 3)[keep], (vz >> 3)[keep]])
            parts.append((rec, key))
    rec = np.concatenate([r for r, _ in parts])
    key = np.concatenate([k for _, k in parts], axis=1)
    return rec[np.lexsort(key)]                     # the last key row (block z) is the most significant


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype.itemsize == b.dtype.itemsize and a.shape == b.shape and np.array_equal(a.view(np.uint8),
                                                                                         b.view(np.uint8))
