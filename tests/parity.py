"""Map comparison used by the parity tests: HIP engine vs CPU oracle on the same inputs.

Bar (BASELINE.json north_star): hash indices / block IDs / free list bit-exact; tsdf and
probability within 1e-4 absolute; weight and rgb exact (they are integers derived from the same
fp32 operations in the same order; the only differing functions are expf/logf, which do not feed
them).
"""
import numpy as np

TOL = 1e-4


def assert_stats_equal(a, b, keys=("visible_blocks", "updated_voxels", "allocated_blocks",
                                   "deleted_blocks", "active_blocks")):
    sa, sb = a.last_frame_stats(), b.last_frame_stats()
    for k in keys:
        assert sa[k] == sb[k], f"frame stat {k}: {sa[k]} != {sb[k]} ({sa} vs {sb})"


def assert_directory_equal(a, b):
    ea, ba = a.dump_directory()
    eb, bb = b.dump_directory()
    assert len(ea) == len(eb), f"active entries {len(ea)} != {len(eb)}"
    assert np.array_equal(ea, eb), "hash entry indices differ"
    for f in ("x", "y", "z", "offset", "idx"):
        assert np.array_equal(ba[f], bb[f]), f"directory field {f} differs"
    return ea, ba


def assert_heap_equal(a, b):
    fa, ha = a.dump_heap()
    fb, hb = b.dump_heap()
    assert fa == fb, f"num_free {fa} != {fb}"
    assert np.array_equal(ha[:fa], hb[:fb]), "free list contents differ"


def assert_pool_consistent(e):
    """The directory and the free list partition the voxel pool: no pool index is named by two live entries, the
    free list heap[:num_free] repeats none, free and named indices are disjoint and together make the whole pool, and
    num_active_blocks() counts the live entries.  Two entries naming one pool block share its voxels and corrupt each
    other's TSDF without any statistic noticing.  The pool size is the engine's own (1 << block_bits)."""
    _, blocks = e.dump_directory()
    nf, heap = e.dump_heap()
    n_pool = 1 << e.block_bits
    assert 0 <= nf <= n_pool, f"num_free {nf} outside [0, {n_pool}]"
    named = blocks["idx"].astype(np.int64)
    free = np.asarray(heap[:nf], dtype=np.int64)
    for what, v in (("named", named), ("free", free)):
        bad = v[(v < 0) | (v >= n_pool)]
        assert bad.size == 0, f"{what} pool indices outside [0, {n_pool}): {bad[:8].tolist()}"
    u, c = np.unique(named, return_counts=True)
    dup = u[c > 1]
    assert dup.size == 0, (f"{dup.size} pool indices named by two live entries: {dup[:8].tolist()} "
                           f"(entries {[np.flatnonzero(named == d).tolist() for d in dup[:4]]} of the directory dump)")
    uf, cf = np.unique(free, return_counts=True)
    rep = uf[cf > 1]
    assert rep.size == 0, f"{rep.size} pool indices on the free list twice: {rep[:8].tolist()}"
    both = np.intersect1d(u, uf)
    assert both.size == 0, f"{both.size} pool indices both free and named: {both[:8].tolist()}"
    lost = n_pool - u.size - uf.size
    assert lost == 0, f"{lost} pool blocks neither free nor named ({u.size} named, {uf.size} free, pool {n_pool})"
    n_active = e.num_active_blocks()
    assert n_active == len(named), f"num_active_blocks {n_active} != {len(named)} live entries"


def assert_voxels_close(a, b, pool_idx, tol=TOL, chunk=4096):
    worst = dict(tsdf=0.0, prob=0.0)
    for lo in range(0, len(pool_idx), chunk):
        idx = pool_idx[lo:lo + chunk]
        ta, ca, pa = a.dump_voxels(idx)
        tb, cb, pb = b.dump_voxels(idx)
        assert np.array_equal(ca["weight"], cb["weight"]), "voxel weights differ"
        for ch in ("r", "g", "b"):
            assert np.array_equal(ca[ch], cb[ch]), f"voxel colour {ch} differs"
        dt = float(np.max(np.abs(ta - tb))) if ta.size else 0.0
        dp = float(np.max(np.abs(pa - pb))) if pa.size else 0.0
        worst["tsdf"] = max(worst["tsdf"], dt)
        worst["prob"] = max(worst["prob"], dp)
        assert dt <= tol, f"tsdf differs by {dt}"
        assert dp <= tol, f"probability differs by {dp}"
    return worst


def assert_maps_equal(a, b, tol=TOL):
    assert_pool_consistent(a)
    _, blocks = assert_directory_equal(a, b)
    assert_heap_equal(a, b)
    assert a.num_active_blocks() == b.num_active_blocks()
    return assert_voxels_close(a, b, blocks["idx"], tol)
