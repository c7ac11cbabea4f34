"""numpy restatement of the point-sampling contract of include/ratsdf_sample.h (test infrastructure).

`sample(points, vs, lookup)` returns SAMPLE_DTYPE records.  `lookup(v)` takes an (m, 3) int array of voxel coordinates
(all inside the int16 range) and returns (allocated bool[m], tsdf f32[m], rgbw RGBW_DTYPE[m], prob f32[m]) -- e.g. the
CPU oracle's test_retrieve (`oracle_lookup`), so the expected values do not come from the engine under test.
All arithmetic is float32, one rounding per operation, in the order the header writes it."""
import numpy as np

from ratsdf._abi import RGBW_DTYPE, SAMPLE_ALLOCATED, SAMPLE_DTYPE, SAMPLE_NEAREST, SAMPLE_OBSERVED

F = np.float32
QNAN = np.uint32(0x7FC00000).view(np.float32)


def round_half_away(g):
    """roundf: half away from zero, exactly (g - trunc(g) is exact in float32)"""
    t = np.trunc(g)
    fr = g - t
    return (t + np.where(np.abs(fr) >= F(0.5), np.sign(g), F(0))).astype(np.float32)


def mirrored_tsdf(g, corner):
    """VoxelHashTable::RetrieveTSDF (voxel_hash.cu:161-188) restated: the corner at floor + 1 weighted by (floor + 1 - g)
    -- the pairing the point query does NOT use.  corner(i, j, k) -> tsdf at floor + (i, j, k)."""
    pl = np.floor(g)
    al = (pl + F(1)) - g
    t = {}
    for i in range(8):  # bit set: floor, clear: floor + 1 (kernels_raycast.h: retrieve_tsdf)
        t[i] = corner(0 if (i >> 2) & 1 else 1, 0 if (i >> 1) & 1 else 1, 0 if i & 1 else 1)
    ax, ay, az = al[:, 0], al[:, 1], al[:, 2]
    t00 = t[0] * az + t[1] * (F(1) - az)
    t01 = t[2] * az + t[3] * (F(1) - az)
    t10 = t[4] * az + t[5] * (F(1) - az)
    t11 = t[6] * az + t[7] * (F(1) - az)
    t0 = t00 * ay + t01 * (F(1) - ay)
    t1 = t10 * ay + t11 * (F(1) - ay)
    return t0 * ax + t1 * (F(1) - ax)


def sample(points, vs, lookup, floor=np.floor, nearest=None, guard=True):
    """the contract.  floor / nearest / guard exist so that a test can state a WRONG variant (trunc for floor, another
    rounding for roundf, no range guard: the corners then wrap to int16) and show that its cases tell it apart"""
    nearest = round_half_away if nearest is None else nearest
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    vs = F(vs)
    out = np.zeros(n, dtype=SAMPLE_DTYPE)
    out["tsdf"] = QNAN
    out["grad"] = QNAN
    with np.errstate(invalid="ignore", over="ignore"):
        g = p / vs
        l = floor(g)
        ok = np.all((l >= F(-32768)) & (l <= F(32766)), axis=1)  # NaN fails every comparison
        if not guard:
            ok = np.all(np.isfinite(l) & (np.abs(l) < F(2 ** 31)), axis=1)
    if not ok.any():
        return out
    g, l = g[ok], l[ok]
    f = g - l
    u = F(1) - f
    li = l.astype(np.int64)
    near = (nearest(g) != l).astype(np.int64)  # 0: floor, 1: floor + 1
    m = g.shape[0]
    corners = np.empty((8, m, 3), dtype=np.int64)
    for k in range(8):
        corners[k] = li + np.array([k >> 2, (k >> 1) & 1, k & 1])
    if not guard:
        corners = ((corners + 32768) & 0xFFFF) - 32768
    alloc, tsdf, rgbw, prob = lookup(corners.reshape(-1, 3))
    alloc = np.asarray(alloc, dtype=bool).reshape(8, m)
    t = np.asarray(tsdf, dtype=np.float32).reshape(8, m)
    rgbw = np.asarray(rgbw, dtype=RGBW_DTYPE).reshape(8, m)
    prob = np.asarray(prob, dtype=np.float32).reshape(8, m)
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    c00 = t[0] * uz + t[1] * fz
    c01 = t[2] * uz + t[3] * fz
    c10 = t[4] * uz + t[5] * fz
    c11 = t[6] * uz + t[7] * fz
    c0 = c00 * uy + c01 * fy
    c1 = c10 * uy + c11 * fy
    ts = c0 * ux + c1 * fx
    gx = (c1 - c0) / vs
    gy = ((c01 - c00) * ux + (c11 - c10) * fx) / vs
    gz = (((t[1] - t[0]) * uy + (t[3] - t[2]) * fy) * ux + ((t[5] - t[4]) * uy + (t[7] - t[6]) * fy) * fx) / vs
    all_alloc = alloc.all(axis=0)
    wmin = rgbw["weight"].min(axis=0)
    kn = (near[:, 0] << 2) | (near[:, 1] << 1) | near[:, 2]
    cols = np.arange(m)
    n_alloc = alloc[kn, cols]
    rec = out[ok]
    rec["tsdf"] = np.where(all_alloc, ts, QNAN)
    rec["grad"] = np.where(all_alloc[:, None], np.stack([gx, gy, gz], axis=1), QNAN)
    rec["prob"] = np.where(n_alloc, prob[kn, cols], F(0))
    nr = rgbw[kn, cols].copy()
    nr[~n_alloc] = np.zeros(1, dtype=RGBW_DTYPE)
    rec["rgbw"] = nr
    rec["min_weight"] = np.where(all_alloc, wmin, 0)
    rec["flags"] = (np.where(all_alloc, SAMPLE_ALLOCATED, 0) | np.where(all_alloc & (wmin >= 1), SAMPLE_OBSERVED, 0) |
                    np.where(n_alloc, SAMPLE_NEAREST, 0))
    out[ok] = rec
    return out


def oracle_lookup(engine):
    """corner values from an engine's test_retrieve (the CPU oracle's, for an independent reference)"""
    def lookup(v):
        v = np.asarray(v)
        uniq, inv = np.unique(v, axis=0, return_inverse=True)
        rgbw, tsdf, prob, blocks = engine.test_retrieve(uniq.astype(np.int16))
        inv = inv.reshape(-1)
        return (blocks["idx"] >= 0)[inv], tsdf[inv], rgbw[inv], prob[inv]
    return lookup


def dict_lookup(voxels):
    """corner values from {(x, y, z): (tsdf, (r, g, b, w), prob)}; absent keys are unallocated"""
    def lookup(v):
        m = len(v)
        alloc = np.zeros(m, dtype=bool)
        tsdf = np.full(m, -10, dtype=np.float32)
        rgbw = np.zeros(m, dtype=RGBW_DTYPE)
        prob = np.zeros(m, dtype=np.float32)
        for i, key in enumerate(map(tuple, np.asarray(v).tolist())):
            if key in voxels:
                t, c, pr = voxels[key]
                alloc[i], tsdf[i], prob[i] = True, t, pr
                rgbw[i] = tuple(c)
        return alloc, tsdf, rgbw, prob
    return lookup


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
