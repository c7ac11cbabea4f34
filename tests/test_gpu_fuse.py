"""Map fusion of the HIP engine (include/ratsdf_fuse.h) against the numpy restatement of its contract
(tests/fuse_ref.py) applied to the CPU ORACLE's maps -- never to the engine's own output.

Maps A and B are two partly overlapping views of the synthetic room (fuse_ref.FRAMES_A / FRAMES_B, 30 degrees apart),
integrated by the HIP engine and by the oracle; assert_maps_equal first, so what is fused is the oracle's input.

Observed on an MI355X (printed by the tests): see DESIGN.md 4 "Map fusion".
"""
import numpy as np
import pytest

import fuse_ref
from fuse_ref import FRAMES_A, FRAMES_AFTER, FRAMES_B, TRUNCATION as TRUNC, VOXEL_SIZE as VS
from parity import TOL, assert_maps_equal, assert_pool_consistent
from test_fuse_ref import assert_pair_qualifies

pytestmark = pytest.mark.gpu

CFG = dict(block_bits=14, bucket_bits=16)
STAT_KEYS = ("blocks_seen", "blocks_allocated", "blocks_skipped", "voxels_copied", "voxels_averaged")


def _snapshot(e):
    ei, blocks = e.dump_directory()
    nf, heap = e.dump_heap()
    t, c, p = e.dump_voxels(blocks["idx"])
    return ei, blocks, nf, heap[:nf].copy(), t, c, p


def _same_snapshot(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y


def _hip(frames=(), **kw):
    import ratsdf
    e = ratsdf.TSDFGrid(VS, TRUNC, **{**CFG, **kw})
    fuse_ref.integrate_frames([e], frames)
    return e


@pytest.fixture(scope="module")
def world():
    """HIP engines holding A and B, the oracle's block sets of both, and the expected fusion A <- B"""
    from oracle_binding import load_oracle
    from ratsdf._abi import Engine
    made, sets = [], []
    for ids in (FRAMES_A, FRAMES_B):
        gpu = _hip()
        cpu = Engine(load_oracle(), VS, TRUNC, threads=8, **CFG)
        fuse_ref.integrate_frames([gpu, cpu], ids)
        assert_maps_equal(gpu, cpu)
        sets.append(fuse_ref.dump_set(cpu))
        cpu.close()
        made.append(gpu)
    A, B = sets
    assert_pair_qualifies(A, B)
    want, info = fuse_ref.fuse(A, B)
    yield dict(gpu_a=made[0], gpu_b=made[1], A=A, B=B, want=want, info=info)
    for e in made:
        e.close()


def _check_stats(stats, info):
    for k in STAT_KEYS:
        assert stats[k] == info[k], (k, stats, {q: info[q] for q in STAT_KEYS})


def _b_records(world):
    """B's blocks as device tensors: positions and 1536-word records, written by the HIP engine that holds B"""
    from ratsdf import multi
    pos = [tuple(int(v) for v in p) for p in world["B"][0]]
    return pos, multi._pos_tensor(pos, "cuda"), multi.export_blocks_device(world["gpu_b"], pos, len(pos), "cuda")


@pytest.mark.parametrize("form", ["map", "blocks", "blocks_device", "file"])
def test_every_form_equals_the_restatement(world, form, tmp_path):
    dst = _hip(FRAMES_A)
    try:
        before = _snapshot(world["gpu_b"])
        if form == "map":
            stats = dst.fuse_map(world["gpu_b"])
        elif form == "blocks":
            stats = dst.fuse_blocks(*world["B"])  # the oracle's arrays
        elif form == "blocks_device":
            pos, pos_t, rec = _b_records(world)
            stats = dst.fuse_blocks_device(len(pos), pos_t.data_ptr(), rec.data_ptr())
        else:
            world["gpu_b"].save_map(tmp_path / "b.map")
            stats = dst.fuse_map_file(tmp_path / "b.map")
        _same_snapshot(before, _snapshot(world["gpu_b"]))  # the source is only read
        _check_stats(stats, world["info"])
        assert_pool_consistent(dst)
        worst = fuse_ref.assert_sets_match(fuse_ref.dump_set(dst), world["want"], world["info"]["colour_known"],
                                           prob_tol=TOL, what=form)
        print(f"fuse[{form}]: max probability difference to the restatement {worst:.3e}; stats {stats}")
    finally:
        dst.close()


def test_fusing_into_an_empty_engine_is_a_copy(world):
    dst = _hip()
    try:
        stats = dst.fuse_map(world["gpu_b"])
        B = world["B"]
        live = fuse_ref.contributes(B[1], B[2])
        assert stats["blocks_allocated"] == len(B[0]) and stats["voxels_copied"] == int(live.sum())
        assert stats["voxels_averaged"] == 0 and stats["blocks_skipped"] == 0
        got = fuse_ref.by_position(fuse_ref.dump_set(dst))
        exp = fuse_ref.by_position(B)
        live = fuse_ref.contributes(exp[1], exp[2])
        assert np.array_equal(got[0], exp[0])
        assert np.array_equal(got[1].view(np.uint32), exp[1].view(np.uint32))
        assert np.array_equal(got[2]["weight"], exp[2]["weight"])
        assert np.array_equal(got[2][live], exp[2][live])  # (colour of fresh voxels: whatever the pool block held)
        worst = float(np.max(np.abs(got[3] - exp[3])))
        assert worst <= TOL
        assert np.array_equal(got[3][~live].view(np.uint32), exp[3][~live].view(np.uint32))
    finally:
        dst.close()


def _home_buckets(pos, bucket_bits):
    p = np.asarray(pos).astype(np.int64).astype(np.uint32)  # two's complement, as the engine's (uint32_t)x
    h = (p[:, 0] * np.uint32(73856093)) ^ (p[:, 1] * np.uint32(19349669)) ^ (p[:, 2] * np.uint32(83492791))
    return h & np.uint32((1 << bucket_bits) - 1)


def test_a_small_directory_needs_several_passes_and_fuses_once(world):
    """2 048 buckets (4 096 entries) for ~1 180 blocks: many of B's blocks share a home bucket, an allocation pass places one block
    per bucket, so one call needs several passes -- a block fused by every pass that finds it would show here"""
    import ratsdf
    new = world["B"][0][~np.isin(fuse_ref.keys(world["B"][0]), fuse_ref.keys(world["A"][0]))]
    with np.errstate(over="ignore"):
        _, per_bucket = np.unique(_home_buckets(world["B"][0], 11), return_counts=True)
        _, new_per_bucket = np.unique(_home_buckets(new, 11), return_counts=True)
    assert per_bucket.max() >= 3, per_bucket.max()
    # ... and of the blocks A lacks (the ones that need a place) some bucket is the home of at least two: one pass
    # places one block per bucket, so a second pass is certain
    assert new_per_bucket.max() >= 2, new_per_bucket.max()
    passes = ratsdf.library().dll.ratsdf_debug_fuse_passes
    passes.restype = __import__("ctypes").c_longlong
    for form in ("map", "blocks_device"):
        # (frames integrated into so small a directory lose insertions to bucket collisions, as in the reference, and
        # the map lags behind A: the destination takes the oracle's A through import_blocks instead)
        dst = _hip(bucket_bits=11)
        try:
            dst.import_blocks(*world["A"])
            assert sorted(fuse_ref.keys(fuse_ref.dump_set(dst)[0])) == sorted(fuse_ref.keys(world["A"][0]))
            if form == "map":
                before = passes()
                stats = dst.fuse_map(world["gpu_b"])
            else:
                pos, pos_t, rec = _b_records(world)
                before = passes()
                stats = dst.fuse_blocks_device(len(pos), pos_t.data_ptr(), rec.data_ptr())
            made = passes() - before
            print(f"small directory, {form}: {made} allocation passes")
            assert made >= 2, made  # (one chunk: the call itself needed more than one pass)
            _check_stats(stats, world["info"])
            assert_pool_consistent(dst)
            fuse_ref.assert_sets_match(fuse_ref.dump_set(dst), world["want"], world["info"]["colour_known"],
                                       prob_tol=TOL, what=f"small directory, {form}")
        finally:
            dst.close()


def test_fusion_is_deterministic_and_checkpoints_continue(world, tmp_path):
    snaps, engines = [], []
    try:
        for _ in range(2):
            a, b = _hip(FRAMES_A), _hip(FRAMES_B)
            engines += [a, b]
            a.fuse_map(b)
            snaps.append(_snapshot(a))
        _same_snapshot(snaps[0], snaps[1])
        fused = engines[0]
        fused.save_map(tmp_path / "fused.map")
        again = _hip()
        engines.append(again)
        again.load_map(tmp_path / "fused.map")
        _same_snapshot(snaps[0], _snapshot(again))
        fuse_ref.integrate_frames([fused, again], FRAMES_AFTER)
        _same_snapshot(_snapshot(fused), _snapshot(again))
    finally:
        for e in engines:
            e.close()


def test_integrating_after_a_fusion_follows_the_oracle(world):
    """frames 54 .. 60 into the fused HIP map == the same frames into an oracle engine that was given the HIP engine's
    fused blocks (the oracle implements import); compared by position: the two directories were filled in different
    orders"""
    from oracle_binding import load_oracle
    from ratsdf._abi import Engine
    gpu = _hip(FRAMES_A)
    cpu = Engine(load_oracle(), VS, TRUNC, threads=8, **CFG)
    try:
        gpu.fuse_map(world["gpu_b"])
        fused = fuse_ref.dump_set(gpu)
        for lo in range(0, len(fused[0]), 1024):
            cpu.import_blocks(*(v[lo:lo + 1024] for v in fused))
        fuse_ref.integrate_frames([gpu, cpu], FRAMES_AFTER)
        g, c = fuse_ref.by_position(fuse_ref.dump_set(gpu)), fuse_ref.by_position(fuse_ref.dump_set(cpu))
        assert np.array_equal(g[0], c[0])
        assert len(g[0]) > len(fused[0])  # the new frames added blocks
        # a voxel nobody has written keeps the colour of its pool block, which differs between the two pools
        touched = fuse_ref.contributes(c[1], c[2])
        assert np.array_equal(g[2]["weight"], c[2]["weight"])
        assert np.array_equal(g[2][touched], c[2][touched])
        dt, dp = float(np.max(np.abs(g[1] - c[1]))), float(np.nanmax(np.abs(g[3] - c[3])))
        print(f"integrate after fusing: tsdf differs by {dt:.3e}, probability by {dp:.3e}")
        assert np.array_equal(np.isnan(g[3]), np.isnan(c[3]))
        assert dt <= TOL and dp <= TOL
    finally:
        gpu.close()
        cpu.close()


def test_shard_engines_get_their_shards_of_the_fused_map(world):
    want = world["want"]
    total = dict.fromkeys(STAT_KEYS, 0)
    seen_blocks = 0
    for r in range(3):
        shard = (r, 3, 2)
        # (a shard engine that integrates A's frames itself does not end with the shard of the whole map A -- on the
        # oracle as well: 2 297 voxels of shard 0 differ, the update of a block depends on which neighbours exist -- so
        # each shard engine is GIVEN its shard of the oracle's A)
        e = _hip(shard_rank=r, shard_count=3, shard_slab_bits=2)
        try:
            mine_a = fuse_ref.shard_owned(world["A"][0], *shard)
            e.import_blocks(*(v[mine_a] for v in world["A"]))
            assert sorted(fuse_ref.keys(fuse_ref.dump_set(e)[0])) == sorted(fuse_ref.keys(world["A"][0][mine_a]))
            existing = int(np.isin(fuse_ref.keys(world["B"][0]), fuse_ref.keys(world["A"][0][mine_a])).sum())
            stats = e.fuse_map(world["gpu_b"])
            assert stats["blocks_seen"] == len(world["B"][0])
            assert stats["blocks_seen"] == stats["blocks_allocated"] + existing + stats["blocks_skipped"]
            assert 0 < stats["blocks_skipped"] < stats["blocks_seen"]
            own = fuse_ref.shard_owned(want[0], *shard)
            part = tuple(v[own] for v in want)
            fuse_ref.assert_sets_match(fuse_ref.dump_set(e), part, world["info"]["colour_known"][own], prob_tol=TOL,
                                       what=f"shard {r}")
            seen_blocks += int(own.sum())
            for k in STAT_KEYS:
                total[k] += stats[k]
        finally:
            e.close()
    assert seen_blocks == len(want[0])
    for k in ("blocks_allocated", "voxels_copied", "voxels_averaged"):
        assert total[k] == world["info"][k], (k, total)
    assert total["blocks_skipped"] == 2 * len(world["B"][0])


def test_errors(world, tmp_path):
    import ratsdf
    dst = _hip(FRAMES_A)
    other = ratsdf.TSDFGrid(VS, 0.05, **CFG)
    tiny = _hip(block_bits=8)  # 256 pool blocks for B's ~970
    try:
        before = _snapshot(dst)

        def refused(call):
            with pytest.raises(ratsdf.RatsdfError) as ei:
                call()
            assert ei.value.status == 1
            _same_snapshot(before, _snapshot(dst))

        refused(lambda: dst.fuse_map(other))           # unequal truncation
        refused(lambda: other.fuse_map(dst))
        refused(lambda: dst.fuse_map(dst))             # dst == src
        B = world["B"]
        dup = tuple(np.concatenate([v[:5], v[2:3]]) for v in B)
        refused(lambda: dst.fuse_blocks(*dup))         # a position listed twice (host form)
        fuse_ref.integrate_frames([other], FRAMES_B[:1])
        other.save_map(tmp_path / "other.map")
        refused(lambda: dst.fuse_map_file(tmp_path / "other.map"))   # a file with another truncation
        finer = ratsdf.TSDFGrid(0.008, TRUNC, **CFG)   # ... and one with another voxel size
        fuse_ref.integrate_frames([finer], FRAMES_B[:1])
        finer.save_map(tmp_path / "finer.map")
        refused(lambda: dst.fuse_map(finer))
        finer.close()
        refused(lambda: dst.fuse_map_file(tmp_path / "finer.map"))
        refused(lambda: dst.fuse_map_file(tmp_path / "missing.map"))
        good = tmp_path / "b.map"
        world["gpu_b"].save_map(good)
        (tmp_path / "short.map").write_bytes(good.read_bytes()[:-4096])
        refused(lambda: dst.fuse_map_file(tmp_path / "short.map"))
        # nothing to do: OK, zero statistics
        empty = _hip()
        assert dst.fuse_map(empty) == dict.fromkeys(STAT_KEYS, 0)
        assert dst.fuse_blocks_device(0, 0, 0) == dict.fromkeys(STAT_KEYS, 0)
        assert dst.fuse_blocks(*fuse_ref.empty_set()) == dict.fromkeys(STAT_KEYS, 0)
        empty.close()
        _same_snapshot(before, _snapshot(dst))
        # pool exhaustion: the status allocation uses, sticky, and the statistics say how far the call got
        with pytest.raises(ratsdf.RatsdfError) as ei:
            tiny.fuse_map(world["gpu_b"])
        assert ei.value.status == 3
        assert 0 < ei.value.fuse_stats["blocks_allocated"] <= 256
        with pytest.raises(ratsdf.RatsdfError) as ei:
            tiny.synchronize()
        assert ei.value.status == 3
    finally:
        for e in (dst, other, tiny):
            e.close()


def test_fuse_group(world):
    """four members of a Group stepped together, then fused into the first: equal to the chain of restatements over the
    oracle's maps of the four streams"""
    import torch
    import ratsdf
    from oracle_binding import load_oracle
    from ratsdf import multi, synthetic
    from ratsdf._abi import Engine
    S, n = 4, 6
    members = [_hip() for _ in range(S)]
    oracles = [Engine(load_oracle(), VS, TRUNC, threads=8, **CFG) for _ in range(S)]
    group = ratsdf.Group(members)
    try:
        frames = [[synthetic.frame("room", 16 * s + 2 * f, scale=0.25, noise=True, holes=True) for s in range(S)]
                  for f in range(n)]
        dev = [[{k: torch.from_numpy(frames[f][s][k]).cuda() for k in ("rgb", "depth", "ht", "lt")} for s in range(S)]
               for f in range(n)]
        H, W = frames[0][0]["depth"].shape

        def batch(lo, hi):
            rows = lambda key: [[dev[f][s][key].data_ptr() for s in range(S)] for f in range(lo, hi)]
            return group.make_batch(rows("rgb"), rows("depth"), rows("ht"), rows("lt"), H, W, 4.0,
                                    [[frames[f][s]["intrinsics"] for s in range(S)] for f in range(lo, hi)],
                                    [[frames[f][s]["pose"] for s in range(S)] for f in range(lo, hi)])

        n_first = n - 2
        torch.cuda.synchronize()
        group.integrate_device_batch(batch(0, n_first))
        group.synchronize()
        for s in range(S):
            for f in range(n_first):
                x = frames[f][s]
                oracles[s].integrate(x["rgb"], x["depth"], x["ht"], x["lt"], 4.0, x["intrinsics"], x["pose"])
            assert_maps_equal(members[s], oracles[s])
        sets = [fuse_ref.dump_set(o) for o in oracles]
        want, known = sets[0], np.ones(sets[0][1].shape, dtype=bool)
        total = dict.fromkeys(STAT_KEYS, 0)
        for s in range(1, S):
            n_before = len(want[0])
            want, info = fuse_ref.fuse(want, sets[s])
            known = np.concatenate([known, np.zeros((len(want[0]) - n_before, 512), dtype=bool)]) | info["colour_known"]
            for k in STAT_KEYS:
                total[k] += info[k]
        stats = multi.fuse_group(members)
        _check_stats(stats, total)
        fuse_ref.assert_sets_match(fuse_ref.dump_set(members[0]), want, known, prob_tol=TOL, what="fuse_group")
        # the group stays usable: one more batch; members 1 .. 3 (only read by the fusion) still follow their oracles
        group.integrate_device_batch(batch(n_first, n))
        group.synchronize()
        for s in range(1, S):
            for f in range(n_first, n):
                x = frames[f][s]
                oracles[s].integrate(x["rgb"], x["depth"], x["ht"], x["lt"], 4.0, x["intrinsics"], x["pose"])
            assert_maps_equal(members[s], oracles[s])
        assert_pool_consistent(members[0])
    finally:
        group.close()
        for e in members + oracles:
            e.close()
