"""numpy restatement of the map-fusion contract (include/ratsdf_fuse.h) on block sets.

A block set is (positions [n, 3] int16, tsdf [n, 512] float32, rgbw [n, 512] RGBW_DTYPE, prob [n, 512] float32) -- what
Engine.dump_directory() + dump_voxels() give and import_blocks() / fuse_blocks() take.  Every operation is a float32
operation, evaluated as the header writes it; the probability is the header's log-odds form (NOT the reference's
two-exponential form).
"""
import numpy as np

from ratsdf._abi import RGBW_DTYPE

F = np.float32
FRESH_TSDF_BITS = 0xBF800000  # -1.0f

# the pair of views the GPU tests fuse (checked on the CPU oracle in tests/test_fuse_ref.py)
FRAMES_A = tuple(range(0, 24, 2))
FRAMES_B = tuple(range(30, 54, 2))
FRAMES_AFTER = tuple(range(54, 61))
VOXEL_SIZE, TRUNCATION, MAX_DEPTH = 0.01, 0.06, 4.0


def integrate_frames(engines, ids):
    """frames `ids` of the synthetic room (quarter scale, noise, holes) into every engine of `engines`"""
    from ratsdf import synthetic
    for i in ids:
        f = synthetic.frame("room", i, scale=0.25, noise=True, holes=True)
        for e in engines:
            e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], MAX_DEPTH, f["intrinsics"], f["pose"])


def dump_set(engine):
    """the engine's map as a block set, in directory order"""
    _, blocks = engine.dump_directory()
    pos = np.stack([blocks["x"], blocks["y"], blocks["z"]], axis=1).astype(np.int16)
    t, c, p = engine.dump_voxels(blocks["idx"])
    return pos, t, c, p


def empty_set():
    return (np.zeros((0, 3), np.int16), np.zeros((0, 512), F), np.zeros((0, 512), RGBW_DTYPE), np.zeros((0, 512), F))


def keys(pos):
    """one int64 per block position (for matching block sets by position)"""
    p = np.asarray(pos).astype(np.int64) & 0xFFFF
    return p[:, 0] | (p[:, 1] << 16) | (p[:, 2] << 32)


def by_position(s):
    """the block set sorted by position key"""
    o = np.argsort(keys(s[0]), kind="stable")
    return tuple(a[o] for a in s)


def contributes(tsdf, rgbw):
    w = rgbw["weight"]
    return (w != 0) & ~((w == 1) & (np.ascontiguousarray(tsdf, dtype=F).view(np.uint32) == FRESH_TSDF_BITS))


def logit(p):
    p = np.asarray(p, dtype=F)
    with np.errstate(all="ignore"):
        return np.log(p / (F(1) - p), dtype=F)


def fuse_voxels(at, ac, ap, bt, bc, bp):
    """a <- b voxel by voxel.  Returns (tsdf, rgbw, prob, copied mask, averaged mask)."""
    at, bt, ap, bp = (np.asarray(v, dtype=F) for v in (at, bt, ap, bp))
    cb, ca = contributes(bt, bc), contributes(at, ac)
    copied, averaged = cb & ~ca, cb & ca
    wa, wb = ac["weight"].astype(F), bc["weight"].astype(F)
    wc = wa + wb
    with np.errstate(all="ignore"):
        t = (at * wa + bt * wb) / wc
        col = {}
        for ch in ("r", "g", "b"):
            q = (ac[ch].astype(F) * wa + bc[ch].astype(F) * wb) / wc
            q = np.where(averaged, q, F(0))
            col[ch] = np.floor(q.astype(np.float64) + 0.5).astype(np.uint8)  # roundf: half away from zero, q >= 0
        w = np.minimum(wc, F(40)).astype(np.uint8)
        x = (wa * logit(ap) + wb * logit(bp)) / wc
        p = F(1) / (F(1) + np.exp(-x, dtype=F))
    ot, oc, op = at.copy(), ac.copy(), ap.copy()
    ot[copied], oc[copied], op[copied] = bt[copied], bc[copied], bp[copied]
    ot[averaged], op[averaged] = t[averaged], p[averaged]
    for ch in ("r", "g", "b"):
        oc[ch][averaged] = col[ch][averaged]
    oc["weight"][averaged] = w[averaged]
    assert ot.dtype == F and op.dtype == F
    return ot, oc, op, copied, averaged


def shard_owned(pos, shard_rank, shard_count, slab_bits):
    """owner of a block = floormod(bx >> slab_bits, shard_count)"""
    if shard_count <= 1:
        return np.ones(len(pos), dtype=bool)
    return np.mod(np.asarray(pos)[:, 0].astype(np.int64) >> slab_bits, shard_count) == shard_rank


def fuse(dst, src, shard=None):
    """dst <- src.  shard = (rank, count, slab_bits) of the destination, or None.  Returns (result set, info): the
    destination's blocks in their order, then the source's new blocks in theirs; info has the statistics of
    ratsdf_fuse_stats and `colour_known` [n, 512] bool: False where the colour is whatever the destination's pool block
    held (a voxel of a newly allocated block that the source does not contribute to)."""
    dpos, dt, dc, dp = dst
    spos, st, sc, sp = src
    own = shard_owned(spos, *shard) if shard is not None else np.ones(len(spos), dtype=bool)
    dk, sk = keys(dpos), keys(spos)
    assert len(np.unique(dk)) == len(dk) and len(np.unique(sk)) == len(sk), "positions must be distinct"
    where = {int(k): i for i, k in enumerate(dk)}
    new = np.array([own[i] and int(k) not in where for i, k in enumerate(sk)], dtype=bool)
    n_new = int(new.sum())
    fresh_c = np.zeros((n_new, 512), dtype=RGBW_DTYPE)
    fresh_c["weight"] = 1
    pos = np.concatenate([dpos, spos[new]])
    t = np.concatenate([np.asarray(dt, dtype=F), np.full((n_new, 512), -1, dtype=F)])
    c = np.concatenate([dc, fresh_c])
    p = np.concatenate([np.asarray(dp, dtype=F), np.full((n_new, 512), 0.5, dtype=F)])
    known = np.ones(t.shape, dtype=bool)
    known[len(dpos):] = False
    where = {int(k): i for i, k in enumerate(keys(pos))}
    rows = np.array([where[int(k)] for k in sk[own]], dtype=np.int64)
    src_rows = np.flatnonzero(own)
    copied_n = averaged_n = 0
    if len(rows):
        ot, oc, op, cm, am = fuse_voxels(t[rows], c[rows], p[rows], st[src_rows], sc[src_rows], sp[src_rows])
        t[rows], c[rows], p[rows] = ot, oc, op
        known[rows] |= cm | am
        copied_n, averaged_n = int(cm.sum()), int(am.sum())
    info = dict(blocks_seen=len(spos), blocks_allocated=n_new, blocks_skipped=int((~own).sum()),
                voxels_copied=copied_n, voxels_averaged=averaged_n, colour_known=known)
    return (pos, t, c, p), info


def assert_sets_match(got, want, colour_known=None, prob_tol=1e-4, what="", tsdf_tol=None, tsdf_nan_payload=True):
    """block sets equal by position: block set, tsdf / weight / colour bit for bit (colour only where known), the
    probability NaN exactly where `want`'s is, else within prob_tol.  Returns the largest probability difference.
    tsdf_nan_payload=False: where `want`'s tsdf is NaN any NaN will do (two processors may pick different payloads);
    everywhere else bit for bit as before."""
    g, w = by_position(got), by_position(want)
    assert len(g[0]) == len(w[0]), f"{what}: {len(g[0])} blocks, expected {len(w[0])}"
    assert np.array_equal(g[0], w[0]), f"{what}: block sets differ"
    if colour_known is None:
        known = np.ones(w[1].shape, dtype=bool)
    else:
        known = colour_known[np.argsort(keys(want[0]), kind="stable")]
    gt, wt = g[1].view(np.uint32), np.ascontiguousarray(w[1], dtype=F).view(np.uint32)
    bad = gt != wt
    if not tsdf_nan_payload:
        bad &= ~(np.isnan(g[1]) & np.isnan(w[1]))
    if tsdf_tol is not None:  # (inputs that are not the oracle's own: the parity bar instead of bit equality)
        bad = ~(np.abs(g[1] - w[1]) <= tsdf_tol)
    assert not bad.any(), (f"{what}: tsdf differs in {int(bad.sum())} voxels, first at block/voxel "
                           f"{np.argwhere(bad)[0].tolist()}: {g[1][bad][0]!r} != {w[1][bad][0]!r}")
    assert np.array_equal(g[2]["weight"], w[2]["weight"]), f"{what}: weights differ"
    for ch in ("r", "g", "b"):
        bad = (g[2][ch] != w[2][ch]) & known
        assert not bad.any(), f"{what}: colour {ch} differs in {int(bad.sum())} voxels"
    gn, wn = np.isnan(g[3]), np.isnan(w[3])
    assert np.array_equal(gn, wn), f"{what}: probability NaN pattern differs ({int(gn.sum())} vs {int(wn.sum())})"
    d = np.abs(np.where(wn, F(0), g[3]) - np.where(wn, F(0), w[3]))
    worst = float(d.max()) if d.size else 0.0
    assert worst <= prob_tol, f"{what}: probability differs by {worst}"
    return worst


def set_from_map_file(data):
    """the live blocks of a checkpoint file (bytes) as a block set, in entry order"""
    import mapfile_ref
    m = mapfile_ref.parse(data)
    live = m["blocks"][m["blocks"]["idx"] >= 0]
    pos = np.stack([live["x"], live["y"], live["z"]], axis=1).astype(np.int16)
    return pos, m["tsdf"], m["rgbw"], m["prob"]
