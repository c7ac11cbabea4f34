"""Map coarsening of the HIP engine (include/ratsdf_coarsen.h) against the numpy restatement of its contract
(tests/coarsen_ref.py, then tests/fuse_ref.py for the fusion step).  The maps are crafted with import_blocks, so every
voxel word is known; the expected values never come from the engine under test."""
import numpy as np
import pytest

import coarsen_ref as cr
import fuse_ref
from parity import TOL, assert_pool_consistent
from test_gpu_resample import CFG, CLUSTER, STAT_KEYS, TRUNC, check_stats, craft, snapshot

pytestmark = pytest.mark.gpu

F = np.float32
VS = 0.01
VS2 = float(F(2) * F(VS))


def engine(vs, block_set=None, trunc=TRUNC, **kw):
    import ratsdf
    e = ratsdf.TSDFGrid(vs, trunc, **{**CFG, **kw})
    if block_set is not None:
        for lo in range(0, len(block_set[0]), 1024):
            e.import_blocks(*(a[lo:lo + 1024] for a in block_set))
    return e


def full_snapshot(e):
    """directory, free list and every voxel word"""
    return snapshot(e) + tuple(a.tobytes() for a in fuse_ref.dump_set(e))


def coarsen_on_device(src, positions):
    """ratsdf_coarsen_blocks_device over `positions`: (records [n, 1536] uint32, counts int32[n])"""
    import torch
    from ratsdf import multi
    n = len(positions)
    pos = multi._pos_tensor(positions, "cuda")
    rec = torch.full((n, 1536), -1, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    src.coarsen_blocks_device(n, pos.data_ptr(), rec.data_ptr(), cnt.data_ptr())
    src.synchronize()
    return rec.cpu().numpy().view(np.uint32), cnt.cpu().numpy()


@pytest.fixture(scope="module")
def cluster():
    return craft(CLUSTER, seed=11)


@pytest.fixture(scope="module")
def coarse_cluster(cluster):
    """the restatement's coarse cluster: (block set of the non-empty candidates, counts)"""
    return cr.coarsen_map(cluster)


def test_records_equal_the_restatement_bit_for_bit(cluster):
    cand = cr.candidates(cluster[0])
    assert len(cand) == 10
    offered = np.concatenate([cand, np.array([(5, -3, 2), (0, 7, 7)], dtype=np.int16)])
    want, want_cnt = cr.coarsen_blocks(cluster, offered)
    # guards against a vacuous pass, on the restatement
    taps = cr.present_taps(cluster, offered)
    contributing = taps[:, :, 13]
    assert int((contributing & (taps.sum(axis=2) < 27)).sum()) > 100           # taps missing
    x, y, z = np.arange(512) & 7, (np.arange(512) >> 3) & 7, np.arange(512) >> 6
    halo = np.zeros(contributing.shape, dtype=bool)
    for i, o in enumerate(cr.OFFSETS):  # the tap lies in the low column of the table: offset -1 from local index 0
        halo |= taps[:, :, i] & (((o[0] < 0) & (x == 0)) | ((o[1] < 0) & (y == 0)) | ((o[2] < 0) & (z == 0)))[None, :]
    assert int((contributing & halo).sum()) > 100                             # a present tap in the 2B - 1 column
    assert (want_cnt[:10] > 0).all() and not want_cnt[10:].any()
    assert taps[10].any() and not taps[11].any()  # (5, -3, 2) sees the halo plane of fine block 9, (0, 7, 7) nothing
    src = engine(VS, cluster)
    try:
        before = full_snapshot(src)
        rec, cnt = coarsen_on_device(src, offered)
        print(f"{len(offered)} coarse blocks, {int(want_cnt.sum())} contributing voxels; records differ in "
              f"{int((rec != cr.records(want)).sum())} words")
        assert np.array_equal(cnt, want_cnt)
        assert np.array_equal(rec, cr.records(want))
        assert not rec[10:].any() and not cnt[10:].any()
        assert full_snapshot(src) == before
        # without counts
        import torch
        from ratsdf import multi
        out = torch.zeros((2, 1536), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        src.coarsen_blocks_device(2, multi._pos_tensor(offered[:2], "cuda").data_ptr(), out.data_ptr())
        src.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), cr.records(want)[:2])
    finally:
        src.close()


def test_both_ends_of_the_grid_without_wrap_around():
    ends = craft([(-4096, 0, 0), (4095, 0, 0), (4095, 4095, 4095), (-4096, -4096, -4096)], seed=13)
    inside = [(-2048, 0, 0), (2047, 0, 0), (2047, 2047, 2047), (-2048, -2048, -2048)]
    outside = [(2048, 0, 0), (-2049, 0, 0), (4095, 4095, 4095)]
    assert cr.candidates(ends[0]).tolist() == sorted(([list(b) for b in inside]), key=lambda b: (b[2], b[1], b[0]))
    want, want_cnt = cr.coarsen_blocks(ends, inside + outside)
    assert (want_cnt[:4] > 0).all() and not want_cnt[4:].any()
    taps = cr.present_taps(ends, inside[:2])
    x = np.arange(512) & 7
    assert not taps[0][x == 0][:, 0::3].any()                   # the tap at -32769 is absent
    assert taps[1][x == 7][:, 14].any()                          # the tap at 32767 is present
    src = engine(VS, ends)
    try:
        rec, cnt = coarsen_on_device(src, inside + outside)
        assert np.array_equal(cnt, want_cnt) and np.array_equal(rec, cr.records(want))
        assert not rec[4:].any() and not cnt[4:].any()
        dst = engine(VS2)
        try:
            res, _ = cr.coarsen_map(ends)
            expect, info = fuse_ref.fuse(fuse_ref.empty_set(), res)
            check_stats(dst.fuse_map_coarsened(src), info)
            fuse_ref.assert_sets_match(fuse_ref.dump_set(dst), expect, info["colour_known"], prob_tol=0.0, what="grid ends")
        finally:
            dst.close()
    finally:
        src.close()


def test_awkward_floats():
    """+-0, subnormals, +-1, 1e30, +-inf and NaN in the tsdf words, weights up to 255"""
    rng = np.random.default_rng(17)
    positions = [(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)]
    pos, t, c, p = craft(positions, seed=19)
    pool = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x3F800000,
                     0xBF800000, 0x7149F2CA, 0x7F800000, 0xFF800000, 0x7FC00000, 0x3DCCCCCD, 0xBE4CCCCD],
                    dtype=np.uint32).view(F)
    t = np.where(rng.random(t.shape) < 0.2, pool[rng.integers(0, len(pool), t.shape)], t).astype(F)
    c["weight"] = rng.integers(0, 256, t.shape)
    src_set = (pos, t, c, p)
    offered = cr.candidates(pos)
    assert offered.tolist() == [[0, 0, 0]]
    want, want_cnt = cr.coarsen_blocks(src_set, offered)
    w_rec = cr.records(want)
    nan = np.isnan(w_rec[:, :512].view(F))
    fin = np.isfinite(w_rec[:, :512].view(F)) & (want[2]["weight"] != 0)
    assert nan.sum() > 20 and np.isinf(want[1]).sum() > 20 and fin.sum() > 100
    src = engine(VS, src_set)
    try:
        rec, cnt = coarsen_on_device(src, offered)
        assert np.array_equal(cnt, want_cnt)
        got_nan = np.isnan(rec[:, :512].view(F))
        assert np.array_equal(got_nan, nan)
        same = rec == w_rec
        same[:, :512] |= nan
        print(f"awkward floats: {int(nan.sum())} NaN, {int(np.isinf(want[1]).sum())} infinite, "
              f"{int((~same).sum())} words differ")
        assert same.all()
    finally:
        src.close()


def test_into_an_empty_destination(cluster, coarse_cluster):
    res, cnt = coarse_cluster
    want, info = fuse_ref.fuse(fuse_ref.empty_set(), res)
    assert info["voxels_copied"] == int(cnt.sum()) > 0
    src, dst = engine(VS, cluster), engine(VS2)
    try:
        before = full_snapshot(src)
        stats = dst.fuse_map_coarsened(src)
        assert full_snapshot(src) == before  # the source is only read
        check_stats(stats, info)
        assert stats["blocks_seen"] == len(res[0]) == stats["blocks_allocated"] == 10
        assert_pool_consistent(dst)
        worst = fuse_ref.assert_sets_match(fuse_ref.dump_set(dst), want, info["colour_known"], prob_tol=TOL,
                                           what="empty destination")
        print(f"{stats}; max probability difference {worst:.3e}")
    finally:
        src.close()
        dst.close()


def test_into_a_destination_that_overlaps_half_of_it(cluster, coarse_cluster):
    res, _ = coarse_cluster
    half = res[0][::2]
    there = craft(np.concatenate([half, np.array([[40, 40, 40], [-40, 2, 7]], dtype=np.int16)]), seed=23)
    want, info = fuse_ref.fuse(there, res)
    assert info["voxels_averaged"] > 0 and info["voxels_copied"] > 0 and info["blocks_allocated"] == len(res[0]) - len(half)
    src, dst = engine(VS, cluster), engine(VS2, there)
    try:
        before = full_snapshot(src)
        stats = dst.fuse_map_coarsened(src)
        assert full_snapshot(src) == before
        check_stats(stats, info)
        assert_pool_consistent(dst)
        worst = fuse_ref.assert_sets_match(fuse_ref.dump_set(dst), want, info["colour_known"], prob_tol=TOL,
                                           what="overlapping destination")
        print(f"overlap: {stats}; max probability difference {worst:.3e}")
    finally:
        src.close()
        dst.close()


def test_shard_filter(cluster, coarse_cluster):
    res, _ = coarse_cluster
    shard = (1, 2, 1)  # (slab bits 0 would mean the default, 2)
    want, info = fuse_ref.fuse(fuse_ref.empty_set(), res, shard)
    assert 0 < info["blocks_skipped"] < len(res[0])
    src = engine(VS, cluster)
    dst = engine(VS2, shard_rank=shard[0], shard_count=shard[1], shard_slab_bits=shard[2])
    try:
        stats = dst.fuse_map_coarsened(src)
        check_stats(stats, info)
        assert stats["blocks_seen"] == len(res[0]) == stats["blocks_allocated"] + stats["blocks_skipped"]
        fuse_ref.assert_sets_match(fuse_ref.dump_set(dst), want, info["colour_known"], prob_tol=TOL, what="shard 1 of 2")
        assert fuse_ref.shard_owned(fuse_ref.dump_set(dst)[0], *shard).all()
    finally:
        src.close()
        dst.close()


def test_more_than_one_chunk():
    """2060 fine blocks, one per coarse block: two staging chunks of 2048 candidates"""
    n = 2060
    big = craft([(2 * (i % 64), 2 * (i // 64), 0) for i in range(n)], seed=41)
    cand = cr.candidates(big[0])
    assert len(cand) == n > 2048
    res, cnt = cr.coarsen_map(big)
    want, info = fuse_ref.fuse(fuse_ref.empty_set(), res)
    assert len(res[0]) > 2048
    src, dst = engine(VS, big), engine(VS2)
    try:
        stats = dst.fuse_map_coarsened(src)
        print(f"{n} candidates, {len(res[0])} non-empty: {stats}")
        check_stats(stats, info)
        assert stats["blocks_seen"] == len(res[0])
        got = fuse_ref.dump_set(dst)
        k = fuse_ref.keys(got[0])
        assert len(np.unique(k)) == len(k) and np.array_equal(np.sort(k), np.sort(fuse_ref.keys(res[0])))
        fuse_ref.assert_sets_match(got, want, info["colour_known"], prob_tol=TOL, what="two chunks")
        assert_pool_consistent(dst)
    finally:
        src.close()
        dst.close()


def test_refusals_and_empty_calls(cluster):
    import torch
    import ratsdf
    src, dst = engine(VS, cluster), engine(VS2, craft([(1, 1, 1), (3, 2, 0)], seed=5))
    same_vs = engine(VS)
    four = engine(float(F(4) * F(VS)))
    other_trunc = engine(VS2, trunc=0.05)
    empty = engine(VS)
    everyone = [src, dst, same_vs, four, other_trunc, empty]
    fn = ratsdf.library().fn["fuse_map_coarsened"]
    try:
        before = [full_snapshot(e) for e in everyone]

        def refused(call):
            with pytest.raises(ratsdf.RatsdfError) as ei:
                call()
            assert ei.value.status == 1
            assert [full_snapshot(e) for e in everyone] == before

        refused(lambda: dst.fuse_map_coarsened(dst))           # dst == src
        refused(lambda: same_vs.fuse_map_coarsened(src))       # an equal voxel size
        refused(lambda: four.fuse_map_coarsened(src))          # 4x
        refused(lambda: other_trunc.fuse_map_coarsened(src))   # 2x with another truncation
        st = np.full(1, -1, dtype=ratsdf._abi.FUSE_STATS)
        assert fn(None, src._h, st.ctypes.data) == 1           # NULL handles
        assert fn(dst._h, None, st.ctypes.data) == 1
        assert all(int(st[0][k]) == -1 for k in ratsdf._abi.FUSE_STATS.names)
        assert ratsdf.library().fn["coarsen_blocks_device"](None, 0, None, None, None) == 1
        buf = torch.zeros(1536 + 4, dtype=torch.int32, device="cuda")
        refused(lambda: src.coarsen_blocks_device(1, buf.data_ptr(), buf.data_ptr() + 4))  # misaligned records
        refused(lambda: src.coarsen_blocks_device(-1, buf.data_ptr(), buf.data_ptr()))     # n < 0
        refused(lambda: src.coarsen_blocks_device(1, 0, buf.data_ptr()))                   # a NULL pointer with n > 0
        assert [full_snapshot(e) for e in everyone] == before
        # nothing to do: OK, zero statistics, nothing changed
        src.coarsen_blocks_device(0, 0, 0)
        src.synchronize()
        assert dst.fuse_map_coarsened(empty) == dict.fromkeys(STAT_KEYS, 0)
        assert [full_snapshot(e) for e in everyone] == before
    finally:
        for e in everyone:
            e.close()


def test_a_chain_of_three_levels(tmp_path):
    """coarsened(levels=3) of a crafted map at 2^-8 m = the restatement applied three times; the read-outs run on it"""
    import ratsdf
    vs = 2.0 ** -8
    # 4 x 4 x 4 fine blocks around the origin, all voxels observed with a smooth field so that the levels stay populated
    positions = [(x, y, z) for z in range(-2, 2) for y in range(-2, 2) for x in range(-2, 2)]
    fine = craft(positions, seed=29)
    level = fine
    for _ in range(3):
        level, _ = cr.coarsen_map(level)
    assert len(level[0]) > 0 and fuse_ref.contributes(level[1], level[2]).sum() > 8
    want, info = fuse_ref.fuse(fuse_ref.empty_set(), level)
    src = engine(vs, fine)
    out = back = None
    try:
        with pytest.raises(ValueError):
            src.coarsened(levels=0)
        with pytest.raises(ValueError):
            src.coarsened(levels=9)
        out = src.coarsened(levels=3, **CFG)
        assert isinstance(out, ratsdf.TSDFGrid) and out.voxel_size == 2.0 ** -5 and out.truncation == src.truncation
        fuse_ref.assert_sets_match(fuse_ref.dump_set(out), want, info["colour_known"], prob_tol=0.0, what="three levels")
        assert_pool_consistent(out)
        # the coarse map is an engine like any other
        d = out.esdf((-8, -8, -8), (16, 16, 16))
        assert d.shape == (16, 16, 16) and np.isfinite(d).any()
        pts = out.surface_points((-8, -8, -8), (16, 16, 16))
        assert pts.dtype == ratsdf.SURFACE_DTYPE
        path = tmp_path / "coarse.map"
        out.save_map(path)
        meta = ratsdf.map_file_info(path)
        assert meta["voxel_size"] == 2.0 ** -5 and meta["n_blocks"] == len(want[0])
        back = engine(2.0 ** -5)
        back.load_map(path)
        a, b = fuse_ref.by_position(fuse_ref.dump_set(out)), fuse_ref.by_position(fuse_ref.dump_set(back))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    finally:
        for e in (src, out, back):
            if e is not None:
                e.close()


def test_real_frames():
    """four frames of the 160 x 120 / 1 cm synthetic room, coarsened: carved blocks, fresh voxels and real colours"""
    src = engine(VS)
    out = None
    try:
        fuse_ref.integrate_frames([src], (0, 1, 2, 3))
        fine = fuse_ref.dump_set(src)
        assert len(fine[0]) > 100 and (~fuse_ref.contributes(fine[1], fine[2])).any()
        res, cnt = cr.coarsen_map(fine)
        want, info = fuse_ref.fuse(fuse_ref.empty_set(), res)
        out = src.coarsened(**CFG)
        got = fuse_ref.dump_set(out)
        print(f"{len(fine[0])} fine blocks -> {len(got[0])} coarse blocks, {int(cnt.sum())} contributing voxels")
        fuse_ref.assert_sets_match(got, want, info["colour_known"], prob_tol=0.0, what="real frames")
        assert out.num_active_blocks() == len(res[0])
    finally:
        for e in (src, out):
            if e is not None:
                e.close()
