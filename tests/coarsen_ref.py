"""numpy restatement of the coarsening contract of include/ratsdf_coarsen.h (test infrastructure).

A block set is what tests/fuse_ref.py works on: (positions [n, 3] int16, tsdf [n, 512] float32, rgbw [n, 512]
RGBW_DTYPE, prob [n, 512] float32).  Coarse voxel D = 8 * block + local sits on fine voxel 2 * D; its 27 taps are the
fine voxels 2 * D + o.

`coarsen_blocks` is the vectorised, branch-free form (an absent tap enters both sums as 0.0f): per coarse block B it
lays the 3 x 3 x 3 fine blocks at 2B - 1 side by side, cuts the 17^3 region of the taps out of them and sums the 27 taps
in the contract's order, every step a float32 operation.  `coarsen_voxel_skipping` is the contract read literally, one
voxel at a time with a dictionary of blocks, and SKIPS absent taps; tests/test_coarsen_ref.py holds the two against each
other bit for bit."""
import numpy as np

import fuse_ref
from ratsdf._abi import RGBW_DTYPE

F = np.float32
RECORD_WORDS = 1536
OFFSETS = [(ox, oy, oz) for oz in (-1, 0, 1) for oy in (-1, 0, 1) for ox in (-1, 0, 1)]  # ox fastest


def tap_factor(ox, oy, oz):
    return (2 - abs(ox)) * (2 - abs(oy)) * (2 - abs(oz))


def _key(b):
    """one int64 per fine block position inside [-4096, 4095] (NOT masked to 16 bits: nothing wraps)"""
    b = np.asarray(b, dtype=np.int64)
    return (b[..., 0] + 4096) | ((b[..., 1] + 4096) << 13) | ((b[..., 2] + 4096) << 26)


# ---- the branch-free form, block by block ------------------------------------------------------------------------
def regions(src_set, block_pos):
    """per coarse block of block_pos [n, 3]: the 17^3 fine voxels 16B - 1 .. 16B + 15 as arrays indexed [n, fz, fy, fx]:
    (present bool, tsdf f32, rgbw, prob f32).  A voxel outside the int16 range or in no block of the set is not present
    and reads as zeros."""
    pos, t, c, p = src_set
    n_src = len(pos)
    assert np.all((np.asarray(pos) >= -4096) & (np.asarray(pos) <= 4095))
    # one more block at the end: the absent one
    tp = np.concatenate([np.ascontiguousarray(t, dtype=F).reshape(n_src, 8, 8, 8), np.zeros((1, 8, 8, 8), dtype=F)])
    cp = np.concatenate([np.ascontiguousarray(c, dtype=RGBW_DTYPE).reshape(n_src, 8, 8, 8),
                         np.zeros((1, 8, 8, 8), dtype=RGBW_DTYPE)])
    pp = np.concatenate([np.ascontiguousarray(p, dtype=F).reshape(n_src, 8, 8, 8), np.zeros((1, 8, 8, 8), dtype=F)])
    ks = _key(pos) if n_src else np.zeros(0, dtype=np.int64)
    assert len(np.unique(ks)) == len(ks)
    order = np.argsort(ks, kind="stable")
    ks = ks[order]
    B = np.asarray(block_pos, dtype=np.int64).reshape(-1, 3)
    n = len(B)
    i = np.arange(3)
    # fine block (2B - 1 + i) per axis, table index [n, iz, iy, ix]
    fb = np.empty((n, 3, 3, 3, 3), dtype=np.int64)
    fb[..., 0] = (2 * B[:, 0] - 1)[:, None, None, None] + i[None, None, None, :]
    fb[..., 1] = (2 * B[:, 1] - 1)[:, None, None, None] + i[None, None, :, None]
    fb[..., 2] = (2 * B[:, 2] - 1)[:, None, None, None] + i[None, :, None, None]
    inside = np.all((fb >= -4096) & (fb <= 4095), axis=-1)
    rows = np.full((n, 3, 3, 3), n_src, dtype=np.int64)
    if n_src:
        kk = _key(np.clip(fb, -4096, 4095))
        at = np.minimum(np.searchsorted(ks, kk), n_src - 1)
        found = inside & (ks[at] == kk)
        rows = np.where(found, order[at], n_src)
    allocated = np.broadcast_to((rows != n_src)[..., None, None, None], (n, 3, 3, 3, 8, 8, 8))

    def lay(a):  # [n, iz, iy, ix, lz, ly, lx] -> [n, 24, 24, 24] -> the 17^3 region (fine voxel 7 of the low column on)
        return a.transpose(0, 1, 4, 2, 5, 3, 6).reshape(n, 24, 24, 24)[:, 7:, 7:, 7:]
    rt, rc, rp, ra = lay(tp[rows]), lay(cp[rows]), lay(pp[rows]), lay(allocated)
    present = ra & fuse_ref.contributes(rt, rc)
    return present, rt, rc, rp


def _tap(a, ox, oy, oz):
    """the tap at offset o of every coarse voxel of the block: [n, 17, 17, 17] -> [n, 8, 8, 8] (z, y, x)"""
    return a[:, 1 + oz:17 + oz:2, 1 + oy:17 + oy:2, 1 + ox:17 + ox:2]


def coarsen_blocks(src_set, block_pos, chunk=128):
    """ratsdf_coarsen_blocks_device restated: (block set of the listed coarse blocks, counts int32[n]); a voxel that
    does not contribute is all zeros"""
    pos = np.asarray(block_pos, dtype=np.int16).reshape(-1, 3)
    n = len(pos)
    o_t, o_c, o_p = np.zeros((n, 512), dtype=F), np.zeros((n, 512), dtype=RGBW_DTYPE), np.zeros((n, 512), dtype=F)
    cnt = np.zeros(n, dtype=np.int32)
    for lo in range(0, n, chunk):
        present, rt, rc, rp = regions(src_set, pos[lo:lo + chunk])
        m = len(present)
        t0 = np.where(present, rt, F(0))                          # absent: t_o = 0.0f
        w0 = np.where(present, rc["weight"], 0).astype(F)         # absent: c_o = 0.0f
        num, den = np.zeros((m, 8, 8, 8), dtype=F), np.zeros((m, 8, 8, 8), dtype=F)
        with np.errstate(all="ignore"):
            for ox, oy, oz in OFFSETS:
                c_o = F(tap_factor(ox, oy, oz)) * _tap(w0, ox, oy, oz)
                num = num + c_o * _tap(t0, ox, oy, oz)
                den = den + c_o
            ts = num / den
        assert ts.dtype == F and num.dtype == F and den.dtype == F
        ok = _tap(present, 0, 0, 0)
        o_t[lo:lo + m] = np.where(ok, ts, F(0)).reshape(m, 512)
        o_c[lo:lo + m] = np.where(ok, _tap(rc, 0, 0, 0), np.zeros(1, dtype=RGBW_DTYPE)).reshape(m, 512)
        o_p[lo:lo + m] = np.where(ok, _tap(rp, 0, 0, 0), F(0)).reshape(m, 512)
        cnt[lo:lo + m] = ok.reshape(m, 512).sum(axis=1)
    return (pos, o_t, o_c, o_p), cnt


def present_taps(src_set, block_pos):
    """[n, 512, 27] bool: which taps of every coarse voxel are present (offsets in OFFSETS order)"""
    present = regions(src_set, block_pos)[0]
    n = len(present)
    return np.stack([_tap(present, *o).reshape(n, 512) for o in OFFSETS], axis=-1)


def records(block_set):
    """the block set as the words of n device records {tsdf[512] | rgbw[512] | prob[512]}: (n, 1536) uint32"""
    _, t, c, p = block_set
    return np.concatenate([np.ascontiguousarray(t, dtype=F).view(np.uint32),
                           np.ascontiguousarray(c, dtype=RGBW_DTYPE).view(np.uint32).reshape(len(t), 512),
                           np.ascontiguousarray(p, dtype=F).view(np.uint32)], axis=1)


# ---- the contract read literally, one voxel at a time -------------------------------------------------------------
def block_dict(src_set):
    pos, t, c, p = src_set
    return {tuple(int(v) for v in pos[i]): (np.asarray(t[i], dtype=F), c[i], np.asarray(p[i], dtype=F))
            for i in range(len(pos))}


def coarsen_voxel_skipping(blocks, D):
    """coarse voxel D (three ints) over block_dict(): (tsdf f32, rgbw record, prob f32) or None when it does not
    contribute.  Absent taps are skipped, not added as zeros."""
    def tap(v):
        if any(a < -32768 or a > 32767 for a in v):
            return None
        blk = blocks.get((v[0] >> 3, v[1] >> 3, v[2] >> 3))
        if blk is None:
            return None
        i = (v[0] & 7) + 8 * (v[1] & 7) + 64 * (v[2] & 7)
        t, c, p = blk[0][i], blk[1][i], blk[2][i]
        w = int(c["weight"])
        if w == 0 or (w == 1 and t.view(np.uint32) == fuse_ref.FRESH_TSDF_BITS):
            return None
        return t, c, p
    c0 = [2 * int(d) for d in D]
    centre = tap(c0)
    if centre is None:
        return None
    num, den = F(0), F(0)
    with np.errstate(all="ignore"):
        for ox, oy, oz in OFFSETS:
            s = tap((c0[0] + ox, c0[1] + oy, c0[2] + oz))
            if s is None:
                continue
            c_o = F(tap_factor(ox, oy, oz)) * F(int(s[1]["weight"]))
            num = F(num + F(c_o * s[0]))
            den = F(den + c_o)
        return F(num / den), centre[1], centre[2]


# ---- the whole map -------------------------------------------------------------------------------------------------
def candidates(src_pos):
    """coarse block (x >> 1, y >> 1, z >> 1) of every source block, distinct, sorted by (z, y, x): [m, 3] int16"""
    b = np.asarray(src_pos, dtype=np.int64).reshape(-1, 3) >> 1
    if len(b) == 0:
        return np.zeros((0, 3), dtype=np.int16)
    b = np.unique(b[:, ::-1], axis=0)[:, ::-1]
    return np.ascontiguousarray(b).astype(np.int16)


def coarsen_map(src_set):
    """the coarse map: (block set of the candidates with at least one contributing voxel, their counts)"""
    cand = candidates(src_set[0])
    if len(cand) == 0:
        return fuse_ref.empty_set(), np.zeros(0, dtype=np.int32)
    s, cnt = coarsen_blocks(src_set, cand)
    keep = cnt > 0
    return tuple(a[keep] for a in s), cnt[keep]


def fuse_coarsened(dst_set, src_set, shard=None):
    """ratsdf_fuse_map_coarsened restated: coarsen, drop the empty blocks, fuse (tests/fuse_ref.py)"""
    res, _ = coarsen_map(src_set)
    return fuse_ref.fuse(dst_set, res, shard)
