"""Transformed map fusion of the HIP engine (include/ratsdf_resample.h) against the numpy restatement of its contract
(tests/resample_ref.py, then tests/fuse_ref.py for the fusion step).  The maps are crafted with import_blocks, so every
voxel word is known; the expected values never come from the engine under test."""
import math

import numpy as np
import pytest

import fuse_ref
import resample_ref as rr
from parity import TOL, assert_pool_consistent
from ratsdf._abi import RGBW_DTYPE

pytestmark = pytest.mark.gpu

F = np.float32
TRUNC = 0.06
CFG = dict(block_bits=14, bucket_bits=16)
STAT_KEYS = ("blocks_seen", "blocks_allocated", "blocks_skipped", "voxels_copied", "voxels_averaged")
VS_LATTICE = 2.0 ** -6
_AXIS = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
# 0.3 rad about (1, 2, 3) / sqrt(14), and a translation that is no multiple of either voxel size
GENERIC = tuple(float(v) for v in (*(_AXIS * math.sin(0.15)), math.cos(0.15), 0.1234, -0.0567, 0.0891))
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
CLUSTER = ([(x, y, z) for z in (-1, 0, 1) for y in (1, 2, 3) for x in (2, 3, 4)]  # 3 x 3 x 3
           + [(9, -6, 5)]                                                         # one isolated block
           + [(-7, -3, -8)])                                                      # one at negative coordinates


def craft(positions, seed):
    """blocks with random tsdf in [-1, 1], weights 0 .. 40 (zeros and fresh voxels among them), random colour / prob"""
    rng = np.random.default_rng(seed)
    n = len(positions)
    t = rng.uniform(-1, 1, (n, 512)).astype(F)
    c = np.zeros((n, 512), dtype=RGBW_DTYPE)
    for ch in ("r", "g", "b"):
        c[ch] = rng.integers(0, 256, (n, 512))
    c["weight"] = rng.integers(0, 41, (n, 512))
    fresh = rng.random((n, 512)) < 0.08
    t[fresh], c["weight"][fresh] = F(-1), 1
    p = rng.uniform(0.02, 0.98, (n, 512)).astype(F)
    return np.array(positions, dtype=np.int16).reshape(-1, 3), t, c, p


def engine(vs, block_set=None, **kw):
    import ratsdf
    e = ratsdf.TSDFGrid(vs, TRUNC, **{**CFG, **kw})
    if block_set is not None:
        for lo in range(0, len(block_set[0]), 1024):
            e.import_blocks(*(a[lo:lo + 1024] for a in block_set))
    return e


def snapshot(e):
    ei, blocks = e.dump_directory()
    nf, heap = e.dump_heap()
    return ei.tobytes(), blocks.tobytes(), nf, heap[:nf].tobytes()


def check_stats(stats, info):
    for k in STAT_KEYS:
        assert stats[k] == info[k], (k, stats, {q: info[q] for q in STAT_KEYS})


def resample_on_device(src, pose, positions):
    """ratsdf_resample_blocks_device over `positions`: (records [n, 1536] uint32, counts int32[n])"""
    import torch
    from ratsdf import multi
    n = len(positions)
    pos = multi._pos_tensor(positions, "cuda")
    rec = torch.full((n, 1536), -1, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    src.resample_blocks_device(pose, n, pos.data_ptr(), rec.data_ptr(), cnt.data_ptr())
    src.synchronize()
    return rec.cpu().numpy().view(np.uint32), cnt.cpu().numpy()


@pytest.fixture(scope="module")
def cluster():
    return craft(CLUSTER, seed=11)


@pytest.fixture(scope="module")
def resampled(cluster):
    """the restatement's resampled cluster under GENERIC, per voxel size: (block set, counts)"""
    return {vs: rr.blocks_with_contribution(GENERIC, vs, cluster) for vs in (0.01, VS_LATTICE)}


@pytest.mark.parametrize("vs", [0.01, VS_LATTICE])
def test_records_equal_the_restatement_byte_for_byte(cluster, vs):
    cand = rr.padded_blocks(GENERIC, vs, cluster[0])
    want, want_cnt = rr.resample_blocks(GENERIC, vs, cand, rr.set_lookup(cluster))
    assert 0 < int((want_cnt > 0).sum()) < len(cand) and 0 < int(want_cnt.sum()) < 512 * len(cand)
    src = engine(vs, cluster)
    try:
        before = snapshot(src)
        rec, cnt = resample_on_device(src, GENERIC, cand)
        print(f"vs {vs}: {len(cand)} candidate blocks, {int((want_cnt > 0).sum())} non-empty, "
              f"{int(want_cnt.sum())} contributing voxels; records differ in {int((rec != rr.records(want)).sum())} words")
        assert np.array_equal(cnt, want_cnt)
        assert np.array_equal(rec, rr.records(want))
        assert snapshot(src) == before
        # without counts
        import torch
        from ratsdf import multi
        out = torch.zeros((2, 1536), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        src.resample_blocks_device(GENERIC, 2, multi._pos_tensor(cand[:2], "cuda").data_ptr(), out.data_ptr())
        src.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), rr.records(want)[:2])
    finally:
        src.close()


@pytest.mark.parametrize("vs", [0.01, VS_LATTICE])
def test_into_an_empty_destination(cluster, resampled, vs):
    res, cnt = resampled[vs]
    want, info = fuse_ref.fuse(fuse_ref.empty_set(), res)
    assert info["voxels_copied"] > 0
    src, dst = engine(vs, cluster), engine(vs)
    try:
        before = snapshot(src)
        stats = dst.fuse_map_transformed(src, GENERIC)
        assert snapshot(src) == before  # the source is only read
        check_stats(stats, info)
        assert stats["blocks_seen"] == len(res[0]) == stats["blocks_allocated"]
        assert_pool_consistent(dst)
        worst = fuse_ref.assert_sets_match(fuse_ref.dump_set(dst), want, info["colour_known"], prob_tol=TOL,
                                           what="empty destination")  # (the block set: no block more, none less)
        print(f"vs {vs}: {stats}; max probability difference {worst:.3e}")
    finally:
        src.close()
        dst.close()


def test_into_a_destination_that_overlaps_half_of_it(cluster, resampled):
    vs = 0.01
    res, _ = resampled[vs]
    half = res[0][::2]
    there = craft(np.concatenate([half, np.array([[40, 40, 40], [-40, 2, 7]], dtype=np.int16)]), seed=23)
    want, info = fuse_ref.fuse(there, res)
    assert info["voxels_averaged"] > 0 and info["voxels_copied"] > 0 and info["blocks_allocated"] == len(res[0]) - len(half)
    src, dst = engine(vs, cluster), engine(vs, there)
    try:
        stats = dst.fuse_map_transformed(src, GENERIC)
        check_stats(stats, info)
        assert_pool_consistent(dst)
        worst = fuse_ref.assert_sets_match(fuse_ref.dump_set(dst), want, info["colour_known"], prob_tol=TOL,
                                           what="overlapping destination")
        print(f"overlap: {stats}; max probability difference {worst:.3e}")
    finally:
        src.close()
        dst.close()


def _moved_words_match(dst_set, src_set, mapping):
    """every contributing source voxel s sits at mapping(s) of the destination with its three words"""
    pos, t, c, p = src_set
    live = fuse_ref.contributes(t, c).reshape(-1)
    s = rr.block_voxels(pos)[live]
    found, gt, gc, gp = rr.set_lookup(dst_set)(mapping(s))
    assert found.all()
    assert np.array_equal(gt.view(np.uint32), t.reshape(-1)[live].view(np.uint32))
    assert np.array_equal(gc, c.reshape(-1)[live]) and np.array_equal(gp.view(np.uint32), p.reshape(-1)[live].view(np.uint32))
    return int(live.sum())


def test_lattice_cases(cluster):
    vs = VS_LATTICE
    assert fuse_ref.contributes(cluster[1], cluster[2]).any(axis=1).all()  # every source block holds a live voxel
    src = engine(vs, cluster)
    made = [src]

    def fused(pose):
        dst = engine(vs)
        made.append(dst)
        return dst, dst.fuse_map_transformed(src, pose)
    try:
        # identity == plain fusion on a twin destination, every word, by position
        a, sa = fused(IDENTITY)
        b = engine(vs)
        made.append(b)
        sb = b.fuse_map(src)
        assert sa == sb, (sa, sb)
        ga, gb = fuse_ref.by_position(fuse_ref.dump_set(a)), fuse_ref.by_position(fuse_ref.dump_set(b))
        for i in (0, 1, 3):
            assert ga[i].tobytes() == gb[i].tobytes()
        # (the colour of a voxel nobody wrote is whatever its pool block held: two pools, two histories)
        wrote = fuse_ref.contributes(gb[1], gb[2])
        assert np.array_equal(ga[2]["weight"], gb[2]["weight"]) and np.array_equal(ga[2][wrote], gb[2][wrote])
        n_live = int(fuse_ref.contributes(cluster[1], cluster[2]).sum())
        # a shift by whole blocks moves the blocks
        d, st = fused((0, 0, 0, 1, 8 * vs, -16 * vs, 24 * vs))
        moved = (cluster[0] + np.array([1, -2, 3], dtype=np.int16),) + cluster[1:]
        want, info = fuse_ref.fuse(fuse_ref.empty_set(), moved)
        check_stats(st, info)
        fuse_ref.assert_sets_match(fuse_ref.dump_set(d), want, info["colour_known"], prob_tol=0.0, what="block shift")
        # a shift by (3, 0, -5) voxels moves voxels across block faces, exactly
        d, st = fused((0, 0, 0, 1, 3 * vs, 0, -5 * vs))
        assert st["voxels_copied"] == n_live and st["voxels_averaged"] == 0
        assert _moved_words_match(fuse_ref.dump_set(d), cluster, lambda s: s + np.array([3, 0, -5])) == n_live
        want, info = rr.fuse_transformed(fuse_ref.empty_set(), cluster, (0, 0, 0, 1, 3 * vs, 0, -5 * vs), vs)
        check_stats(st, info)
        fuse_ref.assert_sets_match(fuse_ref.dump_set(d), want, info["colour_known"], prob_tol=0.0, what="voxel shift")
        # half a turn about z mirrors the indices
        d, st = fused((0, 0, 1, 0, 0, 0, 0))
        assert st["voxels_copied"] == n_live
        assert _moved_words_match(fuse_ref.dump_set(d), cluster, lambda s: s * np.array([-1, -1, 1])) == n_live
        want, info = rr.fuse_transformed(fuse_ref.empty_set(), cluster, (0, 0, 1, 0, 0, 0, 0), vs)
        check_stats(st, info)
        fuse_ref.assert_sets_match(fuse_ref.dump_set(d), want, info["colour_known"], prob_tol=0.0, what="half turn")
    finally:
        for e in made:
            e.close()


def test_no_wrap_around():
    """a source block at block coordinate 4095 pushed past the int16 range: those voxels vanish, nothing appears at -4096"""
    vs = VS_LATTICE
    edge = craft([(4095, 0, 0), (4095, 1, -1)], seed=31)
    pose = (0, 0, 0, 1, 4 * vs, 0, 0)
    want, info = rr.fuse_transformed(fuse_ref.empty_set(), edge, pose, vs)
    live = fuse_ref.contributes(edge[1], edge[2])
    assert 0 < info["voxels_copied"] < int(live.sum())
    src, dst = engine(vs, edge), engine(vs)
    try:
        check_stats(dst.fuse_map_transformed(src, pose), info)
        got = fuse_ref.dump_set(dst)
        assert (got[0][:, 0] == 4095).all() and len(got[0]) == 2
        fuse_ref.assert_sets_match(got, want, info["colour_known"], prob_tol=0.0, what="edge of the grid")
        # ... and asked for the blocks at -4096 directly, the kernel finds nothing there
        rec, cnt = resample_on_device(src, pose, [(-4096, 0, 0), (-4096, 1, -1)])
        assert not cnt.any() and not rec.any()
        # a translation that leaves the grid altogether: OK, nothing offered
        far = engine(vs)
        assert far.fuse_map_transformed(src, (0, 0, 0, 1, 700.0, 0, 0)) == dict.fromkeys(STAT_KEYS, 0)
        assert far.num_active_blocks() == 0
        far.close()
    finally:
        src.close()
        dst.close()


def test_more_than_one_chunk():
    """13 x 13 x 13 source blocks under the generic pose: more candidates than one staging chunk of 2048 holds"""
    vs = 0.01
    big = craft([(x, y, z) for z in range(-6, 7) for y in range(-4, 9) for x in range(-8, 5)], seed=41)
    cand = rr.padded_blocks(GENERIC, vs, big[0])
    assert len(cand) > 2048
    res, cnt = rr.blocks_with_contribution(GENERIC, vs, big)  # (every voxel of every candidate: a few seconds)
    assert len(res[0]) > 2048
    want, info = fuse_ref.fuse(fuse_ref.empty_set(), res)
    src, dst = engine(vs, big), engine(vs)
    try:
        stats = dst.fuse_map_transformed(src, GENERIC)
        print(f"13^3: {len(cand)} brute-force candidates, {stats}")
        check_stats(stats, info)
        got = fuse_ref.dump_set(dst)
        assert np.array_equal(np.sort(fuse_ref.keys(got[0])), np.sort(fuse_ref.keys(res[0])))  # the full block set
        fuse_ref.assert_sets_match(got, want, info["colour_known"], prob_tol=TOL, what="13^3")
        assert_pool_consistent(dst)
    finally:
        src.close()
        dst.close()


def test_refusals_and_empty_calls(cluster):
    import torch
    import ratsdf
    vs = 0.01
    src, dst = engine(vs, cluster), engine(vs, craft([(1, 1, 1), (3, 2, 0)], seed=5))
    other_trunc = ratsdf.TSDFGrid(vs, 0.05, **CFG)
    other_vs = ratsdf.TSDFGrid(0.008, TRUNC, **CFG)
    empty = engine(vs)
    everyone = [src, dst, other_trunc, other_vs, empty]
    fn = ratsdf.library().fn["fuse_map_transformed"]
    try:
        before = [snapshot(e) for e in everyone]

        def refused(call):
            with pytest.raises(ratsdf.RatsdfError) as ei:
                call()
            assert ei.value.status == 1
            assert [snapshot(e) for e in everyone] == before

        refused(lambda: dst.fuse_map_transformed(dst, GENERIC))            # dst == src
        refused(lambda: dst.fuse_map_transformed(other_trunc, GENERIC))    # unequal truncation
        refused(lambda: other_vs.fuse_map_transformed(src, GENERIC))       # unequal voxel size
        for bad in ((0, 0, 0, 1, float("nan"), 0, 0), (0, 0, 0, 1, 0, float("inf"), 0), (float("nan"), 0, 0, 1, 0, 0, 0),
                    (0, 0, 0, 1.01, 0, 0, 0), (0, 0, 0, 0.99, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0)):
            refused(lambda: dst.fuse_map_transformed(src, bad))            # non-finite, or not a unit quaternion
            refused(lambda: src.resample_blocks_device(bad, 0, 0, 0))
        pose = ratsdf._abi._as_pose(GENERIC)
        import ctypes as C
        st = np.full(1, -1, dtype=ratsdf._abi.FUSE_STATS)
        assert fn(dst._h, src._h, None, st.ctypes.data) == 1               # NULL pose
        assert fn(None, src._h, C.byref(pose), st.ctypes.data) == 1        # NULL handles
        assert fn(dst._h, None, C.byref(pose), st.ctypes.data) == 1
        assert [snapshot(e) for e in everyone] == before
        if torch.cuda.device_count() > 1:                                  # engines on two devices
            away = ratsdf.TSDFGrid(vs, TRUNC, device=1, **CFG)
            refused(lambda: away.fuse_map_transformed(src, GENERIC))
            away.close()
        buf = torch.zeros(1536 + 4, dtype=torch.int32, device="cuda")
        refused(lambda: src.resample_blocks_device(GENERIC, -1, buf.data_ptr(), buf.data_ptr()))
        refused(lambda: src.resample_blocks_device(GENERIC, 1, 0, buf.data_ptr()))
        refused(lambda: src.resample_blocks_device(GENERIC, 1, buf.data_ptr(), buf.data_ptr() + 4))  # misaligned records
        # nothing to do: OK, zero statistics, nothing changed
        assert dst.fuse_map_transformed(empty, GENERIC) == dict.fromkeys(STAT_KEYS, 0)
        src.resample_blocks_device(GENERIC, 0, 0, 0)
        src.synchronize()
        assert [snapshot(e) for e in everyone] == before
    finally:
        for e in everyone:
            e.close()


def test_shard_filter(cluster, resampled):
    vs = 0.01
    res, _ = resampled[vs]
    shard = (1, 2, 1)
    want, info = fuse_ref.fuse(fuse_ref.empty_set(), res, shard)
    assert 0 < info["blocks_skipped"] < len(res[0])
    src = engine(vs, cluster)
    dst = engine(vs, shard_rank=shard[0], shard_count=shard[1], shard_slab_bits=shard[2])
    try:
        stats = dst.fuse_map_transformed(src, GENERIC)
        check_stats(stats, info)
        assert stats["blocks_seen"] == len(res[0]) == stats["blocks_allocated"] + stats["blocks_skipped"]
        fuse_ref.assert_sets_match(fuse_ref.dump_set(dst), want, info["colour_known"], prob_tol=TOL, what="shard 1 of 2")
        assert fuse_ref.shard_owned(fuse_ref.dump_set(dst)[0], *shard).all()
    finally:
        src.close()
        dst.close()


def test_the_map_is_consistent_afterwards_and_goes_on(cluster):
    """directory, pool and free list after a transformed fusion; then two frames through integrate_device_batch equal
    the same frames on a twin that was GIVEN the fused blocks (compared by position: the directories were filled in
    different orders)"""
    import torch
    from ratsdf import synthetic
    vs = 0.01
    frames = [synthetic.frame("room", i, scale=0.25, noise=True, holes=True) for i in (0, 2)]
    seen = engine(vs)
    fuse_ref.integrate_frames([seen], (0,))
    room = fuse_ref.dump_set(seen)[0].astype(np.int64)
    seen.close()
    # the source is laid where the frames look: the cluster moved to the middle of what frame 0 allocates
    centre = np.sort(room, axis=0)[len(room) // 2]
    pose = GENERIC[:4] + tuple(float(GENERIC[4 + a] + 8 * vs * centre[a]) for a in range(3))
    src, dst = engine(vs, cluster), engine(vs)
    twin = None
    try:
        stats = dst.fuse_map_transformed(src, pose)
        assert stats["blocks_allocated"] > 0
        assert_pool_consistent(dst)
        _, blocks = dst.dump_directory()
        assert dst.num_active_blocks() == len(blocks) == stats["blocks_allocated"]
        nf, _ = dst.dump_heap()
        assert nf == (1 << CFG["block_bits"]) - len(blocks)
        fused = fuse_ref.dump_set(dst)
        assert np.isin(fuse_ref.keys(fused[0]), fuse_ref.keys(room)).any()  # the frames will touch fused blocks
        twin = engine(vs, fused)
        dev = [{k: torch.from_numpy(f[k]).cuda() for k in ("rgb", "depth", "ht", "lt")} for f in frames]
        H, W = frames[0]["depth"].shape
        torch.cuda.synchronize()
        for e in (dst, twin):
            batch = e.make_batch(*([d[k].data_ptr() for d in dev] for k in ("rgb", "depth", "ht", "lt")), H, W, 4.0,
                                 [f["intrinsics"] for f in frames], [f["pose"] for f in frames])
            e.integrate_device_batch(batch)
            e.synchronize()
        assert_pool_consistent(dst)
        g, t = fuse_ref.by_position(fuse_ref.dump_set(dst)), fuse_ref.by_position(fuse_ref.dump_set(twin))
        assert np.array_equal(g[0], t[0]) and len(g[0]) > len(fused[0])
        touched = fuse_ref.contributes(t[1], t[2])
        assert np.array_equal(g[1].view(np.uint32), t[1].view(np.uint32))
        assert np.array_equal(g[2]["weight"], t[2]["weight"]) and np.array_equal(g[2][touched], t[2][touched])
        assert np.array_equal(g[3].view(np.uint32), t[3].view(np.uint32))
    finally:
        for e in (src, dst, twin):
            if e is not None:
                e.close()
