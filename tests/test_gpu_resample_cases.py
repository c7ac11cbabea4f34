"""Transformed map fusion of the HIP engine (include/ratsdf_resample.h) on the crafted cases of tests/resample_cases.py:
worst-row and scaled poses over dense sources at the origin and at the ends of the grid (the 27-block table), lattice
and near-lattice poses over sparse sources (needed corners, ties of roundf, the fraction that rounds to one), awkward
floats, a chained source directory, and a pose whose translation overflows in voxel units.  The sources go in with
import_blocks, so every voxel word is known; what is expected is tests/resample_ref.py (then tests/fuse_ref.py)
applied to the crafted inputs, never an engine's output.  tests/test_resample_cases.py shows without a GPU that the
cases hold what they are for and that planted mistakes fail them.

Records are compared word for word; where the restatement's tsdf is NaN any NaN will do.  The fusion step keeps the
bars of tests/test_gpu_resample.py: statistics and block set exact, tsdf / weight / colour bit for bit, probability
within parity.TOL where voxels are averaged and equal where they are only copied."""
import numpy as np
import pytest

import fuse_ref
import resample_cases as rc
import resample_ref as rr
from fuse_ref import F
from parity import TOL, assert_pool_consistent
from test_gpu_resample import STAT_KEYS, check_stats, engine, resample_on_device, snapshot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sources():
    """get(key, vs) -> (source engine holding rc.source(key), its snapshot); one engine per source and voxel size"""
    made = {}

    def get(key, vs):
        if (key, vs) not in made:
            if key[0] == "chained":  # the fillers first: the dense blocks hang behind them on the chains
                e = engine(vs, bucket_bits=9)
                for part in rc.chained_imports():
                    e.import_blocks(*part)
            else:
                e = engine(vs, rc.source(key))
            want = fuse_ref.by_position(rc.source(key))
            got = fuse_ref.by_position(fuse_ref.dump_set(e))
            assert all(np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes() for g, w in zip(got, want)), \
                f"{key}: the imported map is not the crafted one"
            made[(key, vs)] = (e, snapshot(e))
        return made[(key, vs)]
    yield get
    for e, _ in made.values():
        e.close()


def run_records(sources, c, cand, want, want_cnt, what=None):
    """the device's records over `cand` against the restatement's; prints the case's line; returns (records, counts)"""
    src, before = sources(c.key, c.vs)
    rec, cnt = resample_on_device(src, c.pose, cand)
    bad = rc.record_differences(rec, want)
    nan = int(np.isnan(want[1]).sum())
    print(f"{what or c.name}: {len(cand)} candidate blocks, {int((want_cnt > 0).sum())} non-empty "
          f"({int((want_cnt == 512).sum())} full), {int(want_cnt.sum())} contributing voxels"
          + (f", {nan} NaN" if nan else "") + f"; records differ in {int(bad.sum())} words, counts in "
          f"{int((cnt != want_cnt).sum())} blocks")
    assert np.array_equal(cnt, want_cnt), f"{c.name}: counts differ at blocks {np.asarray(cand)[cnt != want_cnt][:4].tolist()}"
    assert not bad.any(), f"{c.name}: first differing (block, word) {np.argwhere(bad)[0].tolist()}"
    if not nan:
        assert np.array_equal(rec, rr.records(want))  # word for word
    assert snapshot(src) == before, f"{c.name}: the source changed"
    return rec, cnt


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: records and the footprint
@pytest.mark.parametrize("name", [c.name for c in rc.RECORD_CASES])
def test_records_of_dense_sources(sources, name):
    c = rc.BY_NAME[name]
    cand, want, want_cnt = rc.expected(name)
    assert 0 < len(cand) <= rc.CANDIDATE_LIMIT and (want_cnt == 512).sum() >= 2
    rec, cnt = run_records(sources, c, cand, want, want_cnt)
    # the footprint: a block the restatement fills is full on the device (a corner that missed the 27-block table
    # would read as absent and zero its voxel)
    assert (cnt[want_cnt == 512] == 512).all()


@pytest.mark.parametrize("key, pose_name", [(rc.ORIGIN, "worst_y_fwd_up")] + [(("dense", e), rc.END_POSES[e][0])
                                                                           for e in rc.ENDS])
def test_block_lists_at_the_corners_of_the_grid_and_a_block_twice(sources, key, pose_name):
    c = rc.case(key, pose_name)
    cand, _, cnt = rc.expected(c.name)
    some = cand[cnt > 0]
    full, part = (tuple(int(v) for v in b) for b in (cand[np.argmax(cnt)], some[np.argmin(cnt[cnt > 0])]))
    src = rc.source(key)
    for blocks in ([(-4096,) * 3], [(4095,) * 3], [full, part, full],
                   [(-4096,) * 3, part, (4095,) * 3, part, full]):
        want, want_cnt = rr.resample_blocks(c.pose, c.vs, blocks, rr.set_lookup(src))
        run_records(sources, c, np.array(blocks, dtype=np.int16), want, want_cnt, what=f"{c.name} {blocks}")


def test_records_behind_a_chained_directory(sources):
    """the 27 probes walk chains: the dense source behind 600 fillers in 512 buckets, its own destination blocks"""
    c = rc.WHOLE_CASES[2]
    assert c.key == ("chained",)
    src = rc.source(c.key)
    cand = rr.padded_blocks(c.pose, c.vs, rc.dense()[0])
    assert 0 < len(cand) <= rc.CANDIDATE_LIMIT
    want, want_cnt = rr.resample_blocks(c.pose, c.vs, cand, rr.set_lookup(src))
    assert (want_cnt == 512).sum() >= 2
    run_records(sources, c, cand, want, want_cnt)


# ---------------------------------------------------------------------------------------------------------------------
# 3: corners and ties
def _live(key):
    s = rc.source(key)
    return int(fuse_ref.contributes(s[1], s[2]).sum())


@pytest.mark.parametrize("name", [c.name for c in rc.TIE_CASES])
def test_corners_and_ties(sources, name):
    c = rc.BY_NAME[name]
    cand, want, want_cnt = rc.expected(name)
    rec, cnt = run_records(sources, c, cand, want, want_cnt)
    lattice = rc.POSES[c.pose_name].family == "lattice"
    if lattice and c.pose_name.split("+")[1] in ("whole", "eps", "none"):
        # one needed corner per voxel: nothing is eaten away next to unallocated space, not even where the fraction
        # of g = -1e-9 rounds to one
        assert int(want_cnt.sum()) == _live(c.key) == int(cnt.sum())
    # through the whole call into an empty destination
    keep = want_cnt > 0
    res = tuple(a[keep] for a in want)
    exp, info = fuse_ref.fuse(fuse_ref.empty_set(), res)
    src, before = sources(c.key, c.vs)
    dst = engine(c.vs)
    try:
        stats = dst.fuse_map_transformed(src, c.pose)
        check_stats(stats, info)
        assert stats["voxels_averaged"] == 0 and stats["voxels_copied"] == int(want_cnt.sum())
        assert_pool_consistent(dst)
        fuse_ref.assert_sets_match(fuse_ref.dump_set(dst), exp, info["colour_known"], prob_tol=0.0, what=name)
        assert snapshot(src) == before
    finally:
        dst.close()


def test_half_voxel_ties_take_the_voxel_roundf_names(sources):
    """the device's records against the rule worked by hand (resample_cases.half_z_half_x_by_hand): the floor where
    g < 0, floor + 1 where g > 0 -- colour, probability, the smaller weight and the mean of the two tsdf values"""
    c = rc.BY_NAME["sparse_straddle|half_z+half_x"]
    by_hand, n_neg, n_pos = rc.half_z_half_x_by_hand(rc.source(c.key))
    assert n_neg > 300 and n_pos > 300
    cand = rc.expected(c.name)[0]
    src, _ = sources(c.key, c.vs)
    rec, cnt = resample_on_device(src, c.pose, cand)
    assert int(cnt.sum()) == len(by_hand)
    xyz = rr.block_voxels(cand)
    flat = np.concatenate([rec[:, :512].reshape(-1, 1), rec[:, 512:1024].reshape(-1, 1), rec[:, 1024:].reshape(-1, 1)], axis=1)
    at = {tuple(v): i for i, v in enumerate(xyz.tolist())}
    for d, (t, col, p) in by_hand.items():
        row = flat[at[d]]
        assert row[0] == t.view(np.uint32) and row[1] == np.array([col]).view(np.uint32)[0] and row[2] == p.view(np.uint32), d
    print(f"half-voxel ties on the device: {n_neg} voxels at g < 0 take the floor, {n_pos} at g > 0 take floor + 1")


# ---------------------------------------------------------------------------------------------------------------------
# 4: values
@pytest.mark.parametrize("name", [c.name for c in rc.VALUE_CASES])
def test_awkward_values(sources, name):
    c = rc.BY_NAME[name]
    cand, want, want_cnt = rc.expected(name)
    assert np.isnan(want[1]).any()
    rec, cnt = run_records(sources, c, cand, want, want_cnt)
    # (run_records: every word but a NaN tsdf bit for bit.)  Colour, weight and probability words also where the tsdf is NaN
    assert np.array_equal(rec[:, 512:], rr.records(want)[:, 512:])
    assert np.array_equal(np.isnan(rec[:, :512].view(F)), np.isnan(want[1]))


# ---------------------------------------------------------------------------------------------------------------------
# 5: the whole call
_whole = {}


def whole_expected(c):
    """the restatement's resampled map of a whole-call case, once per module"""
    if c.name not in _whole:
        _whole[c.name] = rr.blocks_with_contribution(c.pose, c.vs, rc.source(c.key))
    return _whole[c.name]


@pytest.mark.parametrize("into", ["empty", "crafted"])
@pytest.mark.parametrize("name", [c.name for c in rc.WHOLE_CASES])
def test_the_whole_call(sources, name, into):
    c = next(w for w in rc.WHOLE_CASES if w.name == name)
    res, res_cnt = whole_expected(c)
    assert len(res[0]) >= 40
    there = fuse_ref.empty_set() if into == "empty" else rc.crafted_destination(res[0], seed=97)
    exp, info = fuse_ref.fuse(there, res)
    if into == "crafted":
        assert info["voxels_averaged"] > 0 and info["voxels_copied"] > 0
        assert info["blocks_allocated"] == len(res[0]) - len(res[0][::2])
    src, before = sources(c.key, c.vs)
    dst = engine(c.vs, there if into == "crafted" else None)
    try:
        stats = dst.fuse_map_transformed(src, c.pose)
        print(f"{name} into {into}: {len(res[0])} non-empty blocks, {int(res_cnt.sum())} contributing voxels; {stats}")
        check_stats(stats, info)
        got = fuse_ref.dump_set(dst)
        gk, wk = set(fuse_ref.keys(got[0]).tolist()), set(fuse_ref.keys(exp[0]).tolist())
        assert not (wk - gk), f"{len(wk - gk)} blocks missing: the host's candidate list"
        assert not (gk - wk), f"{len(gk - wk)} blocks too many: an empty candidate was allocated"
        worst = fuse_ref.assert_sets_match(got, exp, info["colour_known"], prob_tol=TOL if into == "crafted" else 0.0,
                                           what=f"{name} into {into}")
        print(f"{name} into {into}: max probability difference {worst:.3e}")
        assert_pool_consistent(dst)
        assert snapshot(src) == before
    finally:
        dst.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6: a pose whose translation overflows in voxel units
def test_overflowing_pose(sources):
    import fuse_cases as fc
    vs = rc.VS
    assert rr.pose_ok(rc.OVERFLOWING) and not np.isfinite(rr.transform(rc.OVERFLOWING, vs)[1][0])
    src, before = sources(rc.ORIGIN, vs)
    cand = np.concatenate([rc.expected("dense[0,0,0]|worst_x_inv")[0], np.array([(-4096,) * 3, (4095,) * 3], dtype=np.int16)])
    rec, cnt = resample_on_device(src, rc.OVERFLOWING, cand)
    print(f"overflowing pose: {len(cand)} blocks, {int(np.count_nonzero(rec))} non-zero words, {int(np.count_nonzero(cnt))} non-zero counts")
    assert not rec.any() and not cnt.any()
    assert snapshot(src) == before
    for there in (None, fc.craft([(0, 0, 0), (1, 1, 1), (-4096, 4095, 0)], seed=5)):
        dst = engine(vs, there)
        try:
            held, words = snapshot(dst), [np.ascontiguousarray(v).tobytes() for v in fuse_ref.dump_set(dst)]
            assert dst.fuse_map_transformed(src, rc.OVERFLOWING) == dict.fromkeys(STAT_KEYS, 0)
            assert snapshot(dst) == held and snapshot(src) == before
            assert [np.ascontiguousarray(v).tobytes() for v in fuse_ref.dump_set(dst)] == words
            assert dst.num_active_blocks() == (0 if there is None else 3)
        finally:
            dst.close()
