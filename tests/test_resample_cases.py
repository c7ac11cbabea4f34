"""The crafted cases of transformed fusion (tests/resample_cases.py) without a GPU: the brute force of the restatement
follows the map the contract defines, every case holds what it was written for (conditions on the restatement's own
inner values, not measurements of an engine), single mistakes planted in a copy of the restatement fail at least one
named case -- so a kernel that makes one of them fails tests/test_gpu_resample_cases.py -- and one answer per family is
worked by hand."""
import numpy as np
import pytest

import fuse_cases as fc
import fuse_ref
import resample_cases as rc
import resample_ref as rr
from fuse_ref import F
from test_resample_ref import assert_is_shuffle, voxel_table


# ---------------------------------------------------------------------------------------------------------------------
# the brute force
def padded_blocks_normalised(pose, vs, src_pos, pad=2.0):
    """WRONG (what resample_ref.padded_blocks was): the forward transform from the NORMALISED quaternion"""
    p = np.array([F(v) for v in pose], dtype=np.float64)
    x, y, z, w = p[:4] / np.linalg.norm(p[:4])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    t = p[4:] / float(F(vs))
    found = set()
    corner = np.array([[(k >> a) & 1 for a in range(3)] for k in range(8)], dtype=np.float64)
    for b in np.asarray(src_pos, dtype=np.int64).reshape(-1, 3):
        d = (8.0 * b[None, :] - 1.0 + 9.0 * corner) @ R.T + t
        lo = np.maximum(np.ceil(d.min(axis=0) - pad), -32768).astype(np.int64) >> 3
        hi = np.minimum(np.floor(d.max(axis=0) + pad), 32767).astype(np.int64) >> 3
        if np.any(lo > hi):
            continue
        found |= {(bx, by, bz) for bz in range(lo[2], hi[2] + 1) for by in range(lo[1], hi[1] + 1)
                  for bx in range(lo[0], hi[0] + 1)}
    return np.array(sorted(found), dtype=np.int16).reshape(-1, 3)


def non_empty(pose, vs, src, cand):
    if len(cand) == 0:
        return set()
    _, cnt = rr.resample_blocks(pose, vs, cand, rr.set_lookup(src))
    return {tuple(b) for b in np.asarray(cand)[cnt > 0].tolist()}


@pytest.mark.parametrize("scaled", ["down", "up"])  # |q|^2 = 0.9991 and 1.0009
@pytest.mark.parametrize("origin", rc.ENDS[:2])
def test_the_brute_force_follows_the_map_of_the_contract(origin, scaled):
    """a dense source at a corner of the grid turned about its own centre with |q|^2 off 1: the non-empty blocks found
    with 2 voxels of padding are those found with 80, and the search from the normalised pose misses most of them"""
    c = rc.case(("dense", origin), f"worst_x_inv_{scaled}")
    n2 = float(np.sum(np.array([F(v) for v in c.pose[:4]], dtype=np.float64) ** 2))
    assert rr.pose_ok(c.pose) and 8e-4 < abs(n2 - 1) <= 1e-3
    src = rc.source(c.key)
    narrow = non_empty(c.pose, c.vs, src, rr.padded_blocks(c.pose, c.vs, src[0]))
    wide = non_empty(c.pose, c.vs, src, rr.padded_blocks(c.pose, c.vs, src[0], pad=80.0))
    old = non_empty(c.pose, c.vs, src, padded_blocks_normalised(c.pose, c.vs, src[0]))
    print(f"{c.name}: {len(narrow)} non-empty blocks at pad 2, {len(wide)} at pad 80, {len(old)} from the normalised pose")
    assert narrow == wide and len(wide) >= 40
    assert len(old & wide) < len(wide) // 2


def test_the_brute_force_of_a_pose_that_overflows_is_empty():
    assert rr.pose_ok(rc.OVERFLOWING)
    G = rr.transform(rc.OVERFLOWING, rc.VS)
    assert not np.isfinite(G[1][0])
    assert len(rr.padded_blocks(rc.OVERFLOWING, rc.VS, rc.dense()[0])) == 0
    _, cnt = rr.resample_blocks(rc.OVERFLOWING, rc.VS, [(0, 0, 0), (-4096, 5, 4095)], rr.set_lookup(rc.dense()))
    assert cnt.tolist() == [0, 0]
    res, _ = rr.blocks_with_contribution(rc.OVERFLOWING, rc.VS, rc.dense())
    assert len(res[0]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# coverage conditions
def summarise(c):
    cand, want, cnt = rc.expected(c.name)
    got, gcnt, inn = rc.resample_with(c.pose, c.vs, cand, rr.set_lookup(rc.source(c.key)))
    # the copy without a switch IS the restatement
    assert np.array_equal(gcnt, cnt) and np.array_equal(rr.records(got), rr.records(want)), c.name
    ok, con, g, f = inn["ok"], inn["contrib"], inn["g"], inn["f"]
    in_grid = ok.reshape(-1, 512).sum(axis=1)
    t = inn["tsdf"][con]
    return dict(
        name=c.name, candidates=len(cand), non_empty=int((cnt > 0).sum()), full=int((cnt == 512).sum()),
        contributing=int(cnt.sum()),
        reach=int(inn["reach"][inn["any_ok"]].max()) if inn["any_ok"].any() else -1,
        need=np.bincount(inn["need_n"][con], minlength=9), kn=set(np.unique(inn["kn"][ok]).tolist()),
        tie_neg=[bool(((f[:, a] == F(0.5)) & (g[:, a] < 0) & ok).any()) for a in range(3)],
        tie_pos=[bool(((f[:, a] == F(0.5)) & (g[:, a] > 0) & ok).any()) for a in range(3)],
        f_one=bool(((f == F(1)) & ok[:, None]).any()), f_values=np.unique(f[ok]),
        partial=int(((in_grid > 0) & (in_grid < 512)).sum()),
        base_min=int(inn["base"][inn["any_ok"]].min()) if inn["any_ok"].any() else None,
        column_max=int(inn["base"][inn["any_ok"]].max()) + 2 if inn["any_ok"].any() else None,
        wmin=set(np.unique(inn["wmin"][con]).tolist()), nan=int(np.isnan(t).sum()),
        subnormal=int(((np.abs(t) > 0) & (np.abs(t) < F(fc.FLT_MIN))).sum()), inf=int(np.isinf(t).sum()))


@pytest.fixture(scope="module")
def summaries():
    out = {c.name: summarise(c) for c in rc.ALL_CASES}
    for s in out.values():
        print(f"{s['name']}: {s['candidates']} candidates, {s['non_empty']} non-empty blocks ({s['full']} full), "
              f"{s['contributing']} contributing voxels, reach {s['reach']}, needed corners 1/2/4/8 "
              f"{s['need'][[1, 2, 4, 8]].tolist()}")
    return out


def test_pose_list():
    assert len(rc.names("worst")) == 6 and len(rc.names("scaled")) == 12
    for n in rc.names("worst", "scaled", "lattice", "quarter", "diagonal", "overflowing"):
        pose = rc.pose_of(n, (11.5, 11.5, 11.5))
        assert rr.pose_ok(pose), n
        n2 = float(np.sum(np.array([F(v) for v in pose[:4]], dtype=np.float64) ** 2))
        if n.endswith("_up"):
            assert 1.0008 < n2 <= 1.001
        elif n.endswith("_down"):
            assert 0.999 <= n2 < 0.9992
        else:
            assert abs(n2 - 1) < 1e-6
    # the worst rows: e_a goes to (1, 1, 1) / sqrt(3), so a row of the inverse's A has the 1-norm sqrt(3)
    for a, ax in enumerate("xyz"):
        M = rc.linear(rc.POSES[f"worst_{ax}_fwd"].q)
        assert np.allclose(M[:, a], rc.N111, atol=1e-6) and abs(np.abs(M[:, a]).sum() - np.sqrt(3)) < 1e-6
        assert np.allclose(rc.linear(rc.POSES[f"worst_{ax}_inv"].q), M.T, atol=1e-6)
    # the centre of the source stays where it is under the contract's own map, scaled or not
    for n in ("worst_x_inv_up", "worst_y_fwd_down", "diag_xy"):
        centre = np.array(rc.centre(("dense", rc.ENDS[1])))
        Ai, c = rr.forward_map(rc.pose_of(n, centre), rc.VS)
        assert np.abs(Ai @ (centre - c) - centre).max() < 1.5  # (the small offset of 1.2 voxels, float32 at 327 m)


def test_every_case_stays_small(summaries):
    for s in summaries.values():
        assert 0 < s["candidates"] <= rc.CANDIDATE_LIMIT, s["name"]
        assert s["non_empty"] > 0 and 0 < s["contributing"] < 512 * s["candidates"], s["name"]


def test_the_table_is_reached_to_its_last_column_and_never_beyond(summaries):
    reach = {n: s["reach"] for n, s in summaries.items()}
    assert max(reach.values()) == 21
    at = [n for n, r in reach.items() if r == 21]
    print(f"reach 21 in {len(at)} cases: {at}")
    assert all("worst" in n for n in at)
    # ... in a dense case at the origin and in one at an end of the grid
    assert any(n.startswith("dense[0,0,0]") for n in at) and any(not n.startswith("dense[0,0,0]") for n in at)


def test_needed_corners_and_nearest_voxels(summaries):
    need = sum(s["need"] for s in summaries.values())
    print(f"contributing voxels by needed corners: {need.tolist()}")
    assert all(need[k] >= 1000 for k in (1, 2, 4, 8)) and need[[0, 3, 5, 6, 7]].sum() == 0
    assert set().union(*(s["kn"] for s in summaries.values())) == set(range(8))
    for a in range(3):
        assert any(s["tie_neg"][a] for s in summaries.values()) and any(s["tie_pos"][a] for s in summaries.values())
    assert any(s["f_one"] for s in summaries.values())


def test_fractions_of_the_lattice_poses_are_what_they_are_for(summaries):
    for c in rc.DENSE_CASES + rc.TIE_CASES:
        p, fv = rc.POSES[c.pose_name], summaries[c.name]["f_values"]
        shift = c.pose_name.split("+")[-1]
        if p.family == "lattice":  # exact
            want = {"whole": {0.0}, "none": {0.0}, "eps": {0.0, 1.0}, "half_xyz": {0.5}}.get(shift, {0.0, 0.5})
            assert set(fv.tolist()) == want, (c.name, fv)
        elif p.family == "quarter":  # sqrt(1/2) is no float32: next to the lattice, not on it
            off = np.minimum(np.minimum(fv, np.abs(fv - F(0.5))), F(1) - fv)
            assert off.max() <= 2e-5 and (off > 0).any(), (c.name, fv)
    s = summaries["sparse_straddle|third_111+eps"]
    assert s["f_one"] and s["need"][1] == s["contributing"]
    # next to the lattice a voxel leans on corners whose factor is 1e-7: two and four of them where a lattice pose needs one
    s = summaries["dense[0,0,0]|quarter_z+whole"]
    assert s["need"][2] > 1000 and s["need"][4] > 1000


def test_grid_ends(summaries):
    ends = [c for c in rc.END_CASES]
    for c in ends:
        assert summaries[c.name]["partial"] >= 1, c.name   # blocks with some lanes in the grid, not all
    assert any(summaries[c.name]["base_min"] == -4096 for c in ends)
    assert any(summaries[c.name]["column_max"] > 4095 for c in ends)
    # float32 at |g| near 32 768 has 1 / 512 of a voxel: the fractions are multiples of it
    fv = summaries["dense[4093,4093,4093]|worst_y_fwd"]["f_values"]
    assert np.array_equal(fv * 512, np.round(fv * 512))


def test_dense_cases_have_full_blocks(summaries):
    for c in rc.RECORD_CASES:
        assert summaries[c.name]["full"] >= 2, c.name
    for c in rc.RECORD_CASES:  # every source voxel is live, so every in-range voxel that leans on allocated space counts
        src = rc.source(c.key)
        assert fuse_ref.contributes(src[1], src[2]).all()


def test_values_case(summaries):
    src = rc.values()
    t, w = src[1].reshape(-1), src[2]["weight"].reshape(-1)
    bits = t.view(np.uint32)
    for tv in rc.VALUE_TSDF:
        for wt in rc.VALUE_WEIGHTS:
            at = np.isnan(t) if tv != tv else bits == (np.uint32(tv) if isinstance(tv, int) else F(tv).view(np.uint32))
            assert (at & (w == wt)).any(), (tv, wt)
    p = src[3].reshape(-1)
    assert np.isnan(p).any() and (p < 0).any() and (np.abs(p) > 1).any()  # probability words are bit patterns
    total = nan = 0
    for c in rc.VALUE_CASES:
        s = summaries[c.name]
        total, nan = total + s["contributing"], nan + s["nan"]
        assert 0 < s["nan"] < 0.05 * s["contributing"], (c.name, s["nan"], s["contributing"])
        assert s["subnormal"] > 0 and s["inf"] > 0, c.name
    print(f"values: {nan} NaN results among {total} contributing voxels")
    wmin = set().union(*(summaries[c.name]["wmin"] for c in rc.VALUE_CASES))
    assert {1, 2, 254, 255} <= wmin
    generic = summaries["values|diag_xy"]
    assert {1, 255} <= generic["wmin"]  # ... also where all eight corners are needed


def test_chained_source():
    filler, d, seed = rc.chained()
    every = rc.source(("chained",))
    assert len(filler[0]) == 600 and len(every[0]) == 627 and len(np.unique(fuse_ref.keys(every[0]))) == 627
    home = fc.home_buckets(every[0], 9)
    assert np.unique(home, return_counts=True)[1].max() <= fc.PASSES
    behind = np.isin(fc.home_buckets(d[0], 9), fc.home_buckets(filler[0], 9))
    print(f"chained (seed {seed}): {int(behind.sum())} of 27 dense blocks share their home bucket with a filler")
    assert behind.sum() >= 14
    # room in the directory: a block is the first or second of its home bucket, or takes the first entry of a bucket
    # nobody calls home
    per = np.bincount(home.astype(np.int64), minlength=512)
    assert (np.maximum(per - 2, 0)).sum() <= 0.8 * (per == 0).sum()
    parts = rc.chained_imports()
    assert np.array_equal(np.concatenate([q[0] for q in parts]), every[0])  # the whole source, fillers first
    assert [len(q[0]) for q in parts] == [100] * 6 + [1] * 27


# ---------------------------------------------------------------------------------------------------------------------
# planted mistakes
@pytest.mark.parametrize("mistake", list(rc.MISTAKES))
def test_planted_mistakes_fail_a_named_case(mistake):
    assert rc.MISTAKES[mistake][1]
    caught = rc.failing_cases(mistake)
    print(f"{mistake}: fails {caught}")
    assert caught, mistake


def test_the_reach_mistake_zeroes_voxels_inside_full_blocks():
    """what a table one column short does: voxels in the middle of blocks that are full in the restatement"""
    c = rc.BY_NAME["dense[0,0,0]|worst_y_fwd"]
    cand, want, cnt = rc.expected(c.name)
    _, wrong_cnt, _ = rc.resample_with(c.pose, c.vs, cand, rr.set_lookup(rc.source(c.key)), reach_limit=20)
    lost = cnt - wrong_cnt
    assert (lost >= 0).all() and lost.sum() > 0
    _, same_cnt, _ = rc.resample_with(c.pose, c.vs, cand, rr.set_lookup(rc.source(c.key)), reach_limit=21)
    assert np.array_equal(same_cnt, cnt)


# ---------------------------------------------------------------------------------------------------------------------
# hand-worked answers
def test_a_third_of_a_turn_about_111_permutes_the_axes():
    """q = (1/2, 1/2, 1/2, 1/2): e_x -> e_y -> e_z -> e_x, so source voxel (x, y, z) lands on (z, x, y), all three words"""
    src = rc.source(("sparse_straddle",))
    assert rc.VS_LATTICE == 2.0 ** -6  # (the voxel size of test_resample_ref.assert_is_shuffle)
    assert_is_shuffle(rc.pose_of("third_111+none"), src, lambda k: (k[2], k[0], k[1]))
    # with the source-frame shift s: d = R (g + s)
    assert_is_shuffle(rc.pose_of("third_111+whole"), src, lambda k: (k[2] + 8, k[0] + 3, k[1] - 5))
    assert_is_shuffle(rc.pose_of("half_y+whole"), src, lambda k: (-(k[0] + 3), k[1] - 5, -(k[2] + 8)))
    assert_is_shuffle(rc.pose_of("half_x+eps"), src, lambda k: (k[0], -k[1], -k[2]))


def test_a_quarter_turn_about_z_by_hand():
    """q = (0, 0, s, s): (x, y, z) -> (-y, x, z).  s = sqrt(1/2) is no float32, so g is within 1e-5 of the source voxel
    but not on it: colour and probability are that voxel's words exactly (the nearest), the weight is the smallest among
    it and the neighbours the tiny factors lean on, and the tsdf moves by at most 3 * 1e-5 * 2 (three axes, factor
    below 1e-5, values in [-1, 1])"""
    c = rc.BY_NAME["dense[0,0,0]|quarter_z+whole"]
    src = rc.source(c.key)
    tab = voxel_table(src)
    cand, want, cnt = rc.expected(c.name)
    got = voxel_table(want)
    sx, sy, sz = rc.SHIFTS["whole"]
    n = exact = 0
    for (x, y, z), (t, col, p) in tab.items():
        d = (-(y + int(sy)), x + int(sx), z + int(sz))
        if not (1 <= x <= 22 and 1 <= y <= 22 and 1 <= z <= 22):
            continue  # (at the source's faces a tiny factor may lean on unallocated space)
        gt, gc, gp = got[d]
        near = [tab[(x + i, y + j, z + k)][1]["weight"] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]
        assert gp.tobytes() == p.tobytes() and all(gc[ch] == col[ch] for ch in ("r", "g", "b")), d
        assert min(near) <= gc["weight"] <= col["weight"], d
        assert abs(float(gt) - float(t)) <= 6e-5, d
        n, exact = n + 1, exact + (gt.tobytes() == t.tobytes())
    print(f"quarter turn about z: {n} interior voxels, tsdf bit-equal in {exact}")
    assert n == 22 ** 3 and 0 < exact < n


def test_half_voxel_ties_at_negative_coordinates_by_hand():
    """the restatement against resample_cases.half_z_half_x_by_hand (the rule is worked there): the nearest voxel is the
    floor where g < 0 and floor + 1 where g > 0, every contributing voxel with all three words, and no voxel more"""
    c = rc.BY_NAME["sparse_straddle|half_z+half_x"]
    want, n_neg, n_pos = rc.half_z_half_x_by_hand(rc.source(c.key))
    got = voxel_table(rc.expected(c.name)[1])
    assert set(got) == set(want)
    for d, (t, col, p) in want.items():
        assert got[d][0] == t and got[d][1] == col and got[d][2].tobytes() == p.tobytes(), d
    print(f"half-voxel ties by hand: {n_neg} at g < 0, {n_pos} at g > 0")
    assert n_neg > 300 and n_pos > 300
