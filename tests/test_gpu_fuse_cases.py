"""Plain map fusion of the HIP engine (include/ratsdf_fuse.h) on the crafted cases of tests/fuse_cases.py.  Both maps of
a case go in with import_blocks, so every voxel word is known; what is expected is tests/fuse_ref.py applied to the
crafted inputs, never the engine's own output.  tests/test_fuse_cases.py shows without a GPU that the cases hold what
they are for and that planted mistakes fail them.

Observed on an MI355X (printed by the tests): see DESIGN.md 2 and 4 "Map fusion".
"""
import ctypes

import numpy as np
import pytest

import fuse_cases as fc
import fuse_ref
import resample_ref as rr
from fuse_ref import F
from parity import TOL, assert_pool_consistent

pytestmark = pytest.mark.gpu

CFG = dict(block_bits=14, bucket_bits=16)
BIG = dict(block_bits=15, bucket_bits=16)
STAT_KEYS = ("blocks_seen", "blocks_allocated", "blocks_skipped", "voxels_copied", "voxels_averaged")


def engine(block_set=None, **kw):
    import ratsdf
    e = ratsdf.TSDFGrid(fc.VS, fc.TRUNC, **{**CFG, **kw})
    if block_set is not None:
        for lo in range(0, len(block_set[0]), 1024):
            e.import_blocks(*(a[lo:lo + 1024] for a in block_set))
    return e


def words(s):
    """the block set by position as bytes: positions and all three voxel words"""
    return tuple(np.ascontiguousarray(v).tobytes() for v in fuse_ref.by_position(s))


def assert_holds(e, block_set, what):
    """the engine's map is the block set, every word (import_blocks wrote what it was given)"""
    assert words(fuse_ref.dump_set(e)) == words(block_set), f"{what}: the imported map is not the crafted one"


def passes():
    import ratsdf
    fn = ratsdf.library().dll.ratsdf_debug_fuse_passes
    fn.restype = ctypes.c_longlong
    return fn()


def fuse(dst, form, src_set, tmp_path, cfg=None):
    """src_set fused into dst through one of the four forms; for `map` and `file` a source engine is built (cfg) and
    shown to hold the crafted words before and after.  Returns the statistics (or raises what the call raises)."""
    if form == "blocks":
        return dst.fuse_blocks(*src_set)
    if form == "blocks_device":
        import torch
        from ratsdf import multi
        pos = multi._pos_tensor(src_set[0], "cuda")
        rec = torch.from_numpy(rr.records(src_set).view(np.int32)).cuda()
        torch.cuda.synchronize()
        try:
            return dst.fuse_blocks_device(len(src_set[0]), pos.data_ptr(), rec.data_ptr())
        finally:
            assert np.array_equal(rec.cpu().numpy().view(np.uint32), rr.records(src_set))  # the records are only read
    src = engine(src_set, **(cfg or {}))
    try:
        assert_holds(src, src_set, form)
        if form == "map":
            try:
                return dst.fuse_map(src)
            finally:
                assert_holds(src, src_set, "the source after fuse_map")  # the source is only read
        path = tmp_path / "source.map"
        src.save_map(path)
        return dst.fuse_map_file(path)
    finally:
        src.close()


def check_stats(stats, info):
    for k in STAT_KEYS:
        assert stats[k] == info[k], (k, stats, {q: info[q] for q in STAT_KEYS})


def check(dst, want, info, what, **kw):
    assert_pool_consistent(dst)
    return fuse_ref.assert_sets_match(fuse_ref.dump_set(dst), want, info["colour_known"], prob_tol=TOL, what=what, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# voxel cases
_expected = {}


def expected(name):
    """(destination set, source set, restatement's result, info, branch masks by block), once per module"""
    if name not in _expected:
        dst, src = fc.as_block_sets(fc.voxel_case(name))
        want, info = fuse_ref.fuse(dst, src)
        _, _, _, copied, averaged = fuse_ref.fuse_voxels(*dst[1:], *src[1:])
        _expected[name] = (dst, src, want, info, copied, averaged)
    return _expected[name]


def run_voxel_case(name, form, tmp_path):
    dst_set, src_set, want, info, copied, averaged = expected(name)
    assert info["blocks_allocated"] == 0 and info["colour_known"].all()
    dst = engine(dst_set)
    try:
        assert_holds(dst, dst_set, name)
        stats = fuse(dst, form, src_set, tmp_path)
        check_stats(stats, info)  # voxels_copied / voxels_averaged exactly
        # tsdf bit for bit (any NaN where NaN is expected), colour and weight exactly, probability within parity.TOL
        worst = check(dst, want, info, f"{name}[{form}]", tsdf_nan_payload=False)
        got, exp = fuse_ref.by_position(fuse_ref.dump_set(dst)), fuse_ref.by_position(want)
        order = np.argsort(fuse_ref.keys(want[0]), kind="stable")
        # unchanged: all three words as they were; copied: all three words of the source -- probability bits too
        same = ~averaged[order]
        assert np.array_equal(got[3].view(np.uint32)[same], exp[3].view(np.uint32)[same]), f"{name}[{form}]: probability words"
        assert np.array_equal(got[1].view(np.uint32)[same], exp[1].view(np.uint32)[same])
        # the special values: 0 and 1 exact where the restatement has them exact (infinite log-odds; on the grid a 1.0
        # of the restatement is a rounded result, and the bar is parity.TOL)
        for v in (0.0, 1.0) if name == "prob_special" else ():
            at = exp[3] == F(v)
            assert at.any() and np.array_equal(got[3][at], exp[3][at]), f"{name}[{form}]: probability {v} not exact"
        print(f"fuse case {name}[{form}]: {len(dst_set[0])} blocks, {stats['voxels_copied']} copied, "
              f"{stats['voxels_averaged']} averaged; max probability difference to the restatement {worst:.3e}")
        return worst
    finally:
        dst.close()


@pytest.mark.parametrize("form", fc.FORMS)
@pytest.mark.parametrize("name", [n for n in fc.VOXEL_CASES if n != "prob_subnormal"])
def test_voxel_cases(name, form, tmp_path):
    run_voxel_case(name, form, tmp_path)


@pytest.mark.parametrize("form", fc.FORMS)
def test_subnormal_probabilities(form, tmp_path):
    """probabilities below FLT_MIN follow the header's line like any other: the logarithm of subnormal odds is taken
    after scaling them into the normal range (the hardware's log2 reads a subnormal input as zero: unscaled, 1e-40 at
    weight 1 against 0.5 at weight 39 gave 0 instead of 0.0909, and against 1.0 NaN instead of 1)"""
    run_voxel_case("prob_subnormal", form, tmp_path)


# ---------------------------------------------------------------------------------------------------------------------
# block lists
@pytest.fixture(scope="module")
def long_list():
    c = fc.long_list()
    st = c.extra["staged"]
    return dict(full=(c, fuse_ref.fuse(c.dst, c.src)), staged=(st, fuse_ref.fuse(st.dst, st.src)))


@pytest.mark.parametrize("form", fc.FORMS)
def test_long_list(long_list, form, tmp_path):
    """18 469 blocks through the device forms (waves stride, a second chunk of 2 085), the first 4 133 through the
    staged forms (two staging chunks of 2 048 and a short third)"""
    c, (want, info) = long_list["full" if form in ("map", "blocks_device") else "staged"]
    assert info["voxels_copied"] > 0 and info["voxels_averaged"] > 0 and info["blocks_allocated"] > 0
    dst = engine(c.dst, **BIG)
    try:
        before = passes()
        stats = fuse(dst, form, c.src, tmp_path, cfg=BIG)
        made = passes() - before
        check_stats(stats, info)
        worst = check(dst, want, info, f"long list[{form}]")
        print(f"long list[{form}]: {stats}; {made} allocation passes; max probability difference {worst:.3e}")
    finally:
        dst.close()


@pytest.mark.parametrize("form", ["blocks", "blocks_device"])
@pytest.mark.parametrize("n", fc.SHORT_LISTS)
def test_short_lists_with_refused_blocks_between(n, form, tmp_path):
    c = fc.short_lists()[n]
    want, info = fuse_ref.fuse(c.dst, c.src, fc.SHORT_SHARD)
    r, count, slab = fc.SHORT_SHARD
    dst = engine(c.dst, bucket_bits=9, shard_rank=r, shard_count=count, shard_slab_bits=slab)
    try:
        before = passes()
        stats = fuse(dst, form, c.src, tmp_path)
        made = passes() - before
        print(f"short list of {n}[{form}]: {stats}; {made} allocation passes")
        if n >= 31:
            assert made >= 2, made  # (so the done bits of the first pass mattered)
        check_stats(stats, info)   # a refused block is counted once, whatever the number of passes
        check(dst, want, info, f"short list of {n}[{form}]")
    finally:
        dst.close()


@pytest.mark.parametrize("form", ["map", "blocks_device"])
def test_passes_run_out(form, tmp_path):
    """11 new blocks in one home bucket of a 512-bucket directory: 8 passes place 8 of them.  RATSDF_ERR_CAPACITY, the
    statistics say how far the call got, what has a place is fused exactly once, the engine stays usable."""
    import ratsdf
    c = fc.passes_run_out()
    col, others = c.extra["colliders"], c.extra["others"]
    dst = engine(c.dst, bucket_bits=9)
    try:
        assert_holds(dst, c.dst, "destination")
        before = passes()
        with pytest.raises(ratsdf.RatsdfError) as ei:
            fuse(dst, form, c.src, tmp_path)
        assert ei.value.status == 4
        assert passes() - before == fc.PASSES
        stats = ei.value.fuse_stats
        got = fuse_ref.dump_set(dst)
        placed = np.isin(fuse_ref.keys(c.src[0]), fuse_ref.keys(got[0]))
        n_col = int(np.isin(fuse_ref.keys(col), fuse_ref.keys(got[0])).sum())
        print(f"passes run out[{form}]: {n_col} of {len(col)} colliders placed in {fc.PASSES} passes; {stats}")
        assert 1 <= n_col <= fc.PASSES
        assert np.isin(fuse_ref.keys(others), fuse_ref.keys(got[0])).all()
        assert stats["blocks_allocated"] == n_col + len(others) == len(got[0]) - len(c.dst[0])
        want, info = fuse_ref.fuse(c.dst, fc.subset(c.src, placed))
        assert stats["blocks_seen"] == len(c.src[0]) and stats["blocks_skipped"] == 0
        assert stats["voxels_copied"] == info["voxels_copied"] and stats["voxels_averaged"] == info["voxels_averaged"]
        check(dst, want, info, f"passes run out[{form}]")  # every block with a place fused once, none twice
        # the status is the call's own, not a sticky engine error (ratsdf_fuse.h): the engine reports nothing and the
        # blocks that found no place can be offered again
        dst.synchronize()
        rest = fc.subset(c.src, ~placed)
        stats2 = dst.fuse_blocks(*rest)
        assert stats2["blocks_allocated"] == len(rest[0]) == len(col) - n_col
        whole, winfo = fuse_ref.fuse(c.dst, c.src)
        check(dst, whole, winfo, f"passes run out[{form}], the rest offered again")
    finally:
        dst.close()


def test_chained_directories_on_both_sides(tmp_path):
    c = fc.chained()
    want, info = fuse_ref.fuse(c.dst, c.src)
    small = dict(bucket_bits=9)
    dst = engine(c.dst, **small)
    try:
        assert_holds(dst, c.dst, "destination")
        before = passes()
        stats = fuse(dst, "map", c.src, tmp_path, cfg=small)  # (the source engine has 512 buckets too)
        made = passes() - before
        print(f"chained directories: {made} allocation passes; {stats}")
        assert made >= 2, made
        check_stats(stats, info)
        check(dst, want, info, "chained directories")
    finally:
        dst.close()


@pytest.mark.parametrize("form", ["map", "blocks"])
@pytest.mark.parametrize("slab_bits", [0, 1, 2])
def test_positions_and_shards(slab_bits, form, tmp_path):
    """(slab_bits 0 is the engine's default, slabs of 4 blocks like 2: ratsdf.h)"""
    c = fc.positions_and_shards()
    skipped = blocks = 0
    for r in range(3):
        shard = fc.effective_shard((r, 3, slab_bits))
        mine = fc.subset(c.dst, fuse_ref.shard_owned(c.dst[0], *shard))
        want, info = fuse_ref.fuse(mine, c.src, shard)
        dst = engine(mine, shard_rank=r, shard_count=3, shard_slab_bits=slab_bits)
        try:
            stats = fuse(dst, form, c.src, tmp_path)
            check_stats(stats, info)
            check(dst, want, info, f"shard {shard}[{form}]")
            got = fuse_ref.dump_set(dst)[0]
            assert fuse_ref.shard_owned(got, *shard).all()
            assert sorted(fuse_ref.keys(got).tolist()) == sorted(
                fuse_ref.keys(c.src[0][fuse_ref.shard_owned(c.src[0], *shard)]).tolist())  # dst is a subset of src
            skipped += stats["blocks_skipped"]
            blocks += len(got)
        finally:
            dst.close()
    assert skipped == 2 * len(c.src[0]) and blocks == len(c.src[0])


# ---------------------------------------------------------------------------------------------------------------------
# the two promises of the header's "All forms" paragraph
@pytest.mark.parametrize("form", ["map", "file"])
@pytest.mark.parametrize("kw", [dict(), dict(bucket_bits=9)], ids=["65536 buckets", "512 buckets"])
def test_the_directory_delta_record_stays_right(kw, form, tmp_path):
    """a replica kept from the engine's own delta log is the directory after a fusion that allocates and averages,
    every field, chain links included"""
    import torch
    from ratsdf import multi
    c = fc.chained()
    want, info = fuse_ref.fuse(c.dst, c.src)
    assert info["blocks_allocated"] > 0 and info["voxels_averaged"] > 0
    dst = engine(c.dst, **kw)
    by_pos = lambda b: b[np.lexsort((b["z"], b["y"], b["x"]))]
    try:
        dx = multi.DirectoryDeltaExchange(engine=dst, device=torch.device("cuda", 0), delta_capacity=4096)
        dx.fill_from_engine(dst)   # the whole directory, and the engine forgets its changes so far
        dx.all_gather()
        assert np.array_equal(by_pos(dx.result()[0]), by_pos(dst.dump_directory()[1]))
        stats = fuse(dst, form, c.src, tmp_path)
        check_stats(stats, info)
        dx.fill_from_engine(dst)   # the delta log alone
        dx.all_gather()
        _, blocks = dst.dump_directory()
        got = dx.result()[0]
        assert len(got) == len(blocks) == len(want[0])
        assert np.array_equal(by_pos(got), by_pos(blocks))
        assert stats["blocks_allocated"] <= dx.last_sent[0] <= len(blocks) and dx.last_sent[1] == 0, dx.last_sent
        if not kw:
            assert dx.last_sent[0] < len(blocks)  # (a delta, not the whole directory again)
        dst.synchronize()
    finally:
        dst.close()


def test_fusion_marks_the_map_as_carrying_probabilities():
    """a map that has only seen TSDF-only frames neither loads nor stores probabilities; after a fusion it must.
    Crafted blocks with p = 0.8 go into blocks the frames look at, more TSDF-only frames follow, and the result is an
    oracle engine's that was given the fused map and the same frames."""
    from oracle_binding import load_oracle
    from ratsdf import synthetic
    from ratsdf._abi import Engine, RGBW_DTYPE

    def tsdf_only(engines, ids):
        for i in ids:
            f = synthetic.frame("room", i, scale=0.25, noise=True, holes=True)
            for e in engines:
                e.integrate(f["rgb"], f["depth"], None, None, fuse_ref.MAX_DEPTH, f["intrinsics"], f["pose"])

    gpu = engine()
    cpu = Engine(load_oracle(), fc.VS, fc.TRUNC, threads=8, **CFG)
    try:
        tsdf_only([gpu], fuse_ref.FRAMES_A[:4])
        seen = fuse_ref.dump_set(gpu)
        assert (seen[3] == F(0.5)).all()
        pos = seen[0][::3]  # the destination's own blocks: the next frames look at them again
        n = len(pos)
        assert n >= 100
        c = np.zeros((n, 512), dtype=RGBW_DTYPE)
        c["r"], c["weight"] = 9, 3
        stats = gpu.fuse_blocks(pos, np.full((n, 512), 0.1, dtype=F), c, np.full((n, 512), 0.8, dtype=F))
        assert stats["blocks_allocated"] == 0 and stats["voxels_copied"] > 0 and stats["voxels_averaged"] > 0
        fused = fuse_ref.dump_set(gpu)
        for lo in range(0, len(fused[0]), 1024):
            cpu.import_blocks(*(v[lo:lo + 1024] for v in fused))
        tsdf_only([gpu, cpu], fuse_ref.FRAMES_A[4:8])
        g, o = fuse_ref.by_position(fuse_ref.dump_set(gpu)), fuse_ref.by_position(fuse_ref.dump_set(cpu))
        assert np.array_equal(g[0], o[0])
        touched = fuse_ref.contributes(o[1], o[2])
        assert np.array_equal(g[2]["weight"], o[2]["weight"])
        assert np.array_equal(g[2][touched], o[2][touched])
        dt, dp = float(np.max(np.abs(g[1] - o[1]))), float(np.nanmax(np.abs(g[3] - o[3])))
        print(f"TSDF-only frames after a fusion: tsdf differs by {dt:.3e}, probability by {dp:.3e}")
        assert np.array_equal(np.isnan(g[3]), np.isnan(o[3]))
        assert dt <= TOL and dp <= TOL
        # the fused voxels the new frames updated have left 0.8 (pooled with the frames' 0.5)
        f = fuse_ref.by_position(fused)
        at = np.isin(fuse_ref.keys(g[0]), fuse_ref.keys(f[0]))
        was = f[3] == F(0.8)
        updated = was & (g[1][at].view(np.uint32) != f[1].view(np.uint32))
        print(f"{int(was.sum())} voxels held 0.8 after the fusion, the frames updated {int(updated.sum())} of them")
        assert updated.sum() >= 100
        assert (g[3][at][updated] < F(0.8)).all() and (g[3][at][updated] > F(0.5)).all()
    finally:
        gpu.close()
        cpu.close()
