"""The crafted fusion cases (tests/fuse_cases.py) without a GPU: each case holds what it was written for, the
restatement's answers on them are sound where that can be shown independently, and single mistakes planted in a copy of
the restatement fail at least one named case -- so a kernel that makes one of them fails tests/test_gpu_fuse_cases.py."""
import numpy as np
import pytest

import fuse_cases as fc
import fuse_ref
from fuse_ref import F


def _expected(name):
    c = fc.voxel_case(name)
    return c, fuse_ref.fuse_voxels(*c.a, *c.b)


def test_colours_cover_every_quotient_and_round_as_exact_rationals():
    c, (_, oc, _, copied, averaged) = _expected("colours")
    assert averaged.all() and not copied.any()
    num, wc = fc.colour_quotients(c.a, c.b)
    have = set((num * 1024 + wc[:, None]).reshape(-1).tolist())
    f, t = fc.colour_pairs_from_frames(), fc.colour_ties()
    assert len(f[0]) == 786290                       # every (num, wc) two maps built from frames can produce
    assert 54825 <= len(t[0]) <= 164475 and int(t[6].sum()) == 215 * 255  # every tie is realisable; most neighbours
    want = set((f[0] * 1024 + f[1]).tolist()) | set((t[0] * 1024 + t[1]).tolist())
    assert have == want
    print(f"colours: {len(f[0])} pairs from frame weights, {len(t[0])} ties and neighbours at sums 82 .. 510, "
          f"{len(c.a.t)} voxels in {-(-len(c.a.t) // 512)} blocks")
    # independently of any float: round half up of the exact rational.  (A non-tie is at least 1 / wc >= 1 / 510 from a
    # half, far above one ulp at 255, so fp32 division followed by roundf must agree.)
    exact = (2 * num + wc[:, None]) // (2 * wc[:, None])
    got = np.stack([oc[ch] for ch in ("r", "g", "b")], axis=1).astype(np.int64)
    assert np.array_equal(got, exact)
    assert np.array_equal(oc["weight"], np.minimum(wc, 40))
    assert {41, 510, 2, 80} <= set(wc.tolist())
    # both sides carry the larger weight somewhere, and ties exist below and above the frame weights
    assert (c.a.c["weight"] > c.b.c["weight"]).any() and (c.a.c["weight"] < c.b.c["weight"]).any()
    ties = (2 * num) % (2 * wc[:, None]) == wc[:, None]
    assert int(ties.sum()) >= 215 * 255


def test_tsdf_case_holds_the_awkward_values():
    c, (ot, _, _, copied, averaged) = _expected("tsdf")
    bits = ot.view(np.uint32)
    av = ot[averaged]
    assert np.isnan(av).sum() >= 100 and np.isinf(av).sum() >= 100     # NaN in, inf - inf, overflow of the sum
    sub = (np.abs(av) > 0) & (np.abs(av) < fc.FLT_MIN)
    assert sub.sum() >= 20                                            # subnormal results
    assert (bits[averaged] == 0x80000000).any() and (bits[averaged] == 0).any()  # both zeros
    assert (np.abs(av[np.isfinite(av)]) > 1).any()
    assert copied.any()                                               # (-1.0 at weight 1 is a fresh voxel)
    wc = c.a.c["weight"].astype(int) + c.b.c["weight"].astype(int)
    assert {2, 41, 80, 510} <= set(wc.tolist())
    # overflow: FLT_MAX on both sides with the same sign gives inf, with opposite signs NaN (inf - inf)
    big = (np.abs(c.a.t) == fc.FLT_MAX) & (np.abs(c.b.t) == fc.FLT_MAX) & (c.a.c["weight"] > 1) & (c.b.c["weight"] > 1)
    assert np.isinf(ot[big & (c.a.t == c.b.t)]).all() and np.isnan(ot[big & (c.a.t != c.b.t)]).all() and big.sum() >= 50


def test_edges_case_takes_every_branch_and_keeps_or_copies_all_three_words():
    from test_fuse_ref import CASES
    c, (ot, oc, op, copied, averaged) = _expected("edges")
    unchanged = ~copied & ~averaged
    assert min(unchanged.sum(), copied.sum(), averaged.sum()) >= 20
    for got, a, b in ((ot.view(np.uint32), c.a.t.view(np.uint32), c.b.t.view(np.uint32)), (oc, c.a.c, c.b.c),
                      (op.view(np.uint32), c.a.p.view(np.uint32), c.b.p.view(np.uint32))):
        assert np.array_equal(got[unchanged], a[unchanged])   # colour included
        assert np.array_equal(got[copied], b[copied])
    assert (c.a.c[unchanged] != c.b.c[unchanged]).all() and (c.a.c[copied] != c.b.c[copied]).all()  # (it would show)
    # the hand-worked rows sit at the end with their branches
    branch = np.array([k[3] for k in CASES])
    assert np.array_equal(copied[-len(CASES):], branch == 1) and np.array_equal(averaged[-len(CASES):], branch == 2)
    # weight 1 at -1.0 is fresh; its two neighbouring bit patterns, and -1.0 at weights 2 and 255, are not
    live = fuse_ref.contributes(*fc.rows(fc.edge_rows((0, 0, 0), 0.5))[:2])
    assert live.tolist() == [False, False, False, True, True, True, True, True, True, True]


def test_patterns_case_counts():
    c, (_, _, _, copied, averaged) = _expected("patterns")
    cp, av = copied.reshape(5, 512), averaged.reshape(5, 512)
    assert cp[0].all() and av[1].all() and not (cp[2] | av[2]).any()
    lanes = (cp[3] | av[3]).reshape(64, 8)
    assert lanes.all(axis=1).sum() == 1 and lanes.any(axis=1).sum() == 1 and lanes[37].all()
    lanes = (cp[4] | av[4]).reshape(64, 8)
    assert (lanes.sum(axis=1) == 1).all() and len(set(lanes.argmax(axis=1).tolist())) == 8
    assert cp[4].sum() == 32 and av[4].sum() == 32   # the tally's two halves both move


def test_prob_grid_is_sound_in_float32():
    """the float32 restatement against a float64 evaluation of the header's line on the grid: 2.2e-7 measured"""
    c, (_, _, op, _, averaged) = _expected("prob_grid")
    assert averaged.all() and len(op) == (len(fc.PROB_GRID) * len(fc.PROB_WEIGHTS)) ** 2
    worst = float(np.max(np.abs(op.astype(np.float64) - fc.prob_float64(c.a, c.b))))
    print(f"prob_grid: float32 restatement within {worst:.3e} of float64")
    assert not np.isnan(op).any() and worst <= 2.5e-7
    assert op.min() < 1e-30 and op.max() > 0.999999


def test_prob_special_and_subnormal_cases():
    c, (_, _, op, _, averaged) = _expected("prob_special")
    assert averaged.all()
    nan = np.isnan(op)
    assert 0 < nan.sum() < len(op)
    assert (op[~nan] == 0).any() and (op[~nan] == 1).any()           # 0 and 1 come out exact
    zero_one = ((c.a.p == 0) & (c.b.p == 1)) | ((c.a.p == 1) & (c.b.p == 0))
    assert zero_one.any() and nan[zero_one].all()
    for v in fc.PROB_SPECIAL:
        for side in (c.a.p, c.b.p):
            assert (np.isnan(side) if v != v else (side.view(np.uint32) == F(v).view(np.uint32))).any(), v
    c, (_, _, op, _, averaged) = _expected("prob_subnormal")
    assert averaged.all() and not np.isnan(op).any()
    sub = lambda p: (p > 0) & (p < fc.FLT_MIN)
    assert (sub(c.a.p) & ~sub(c.b.p)).any() and (~sub(c.a.p) & sub(c.b.p)).any() and (sub(c.a.p) & sub(c.b.p)).any()
    # the two rows that told the raw hardware logarithm from the header's line: (1e-40, 1) with (0.5, 39) and (1.0, 1)
    row = lambda pa, wa, pb, wb: (c.a.p == F(pa)) & (c.a.c["weight"] == wa) & (c.b.p == F(pb)) & (c.b.c["weight"] == wb)
    assert abs(float(op[row(1e-40, 1, 0.5, 39)][0]) - 0.0909) < 1e-4 and float(op[row(1e-40, 1, 1.0, 1)][0]) == 1.0
    worst = float(np.max(np.abs(op.astype(np.float64) - fc.prob_float64(c.a, c.b))))
    print(f"prob_subnormal: float32 restatement within {worst:.3e} of float64")
    assert worst <= 2.5e-7


def test_block_sets_of_a_voxel_case():
    dst, src = fc.as_block_sets(fc.voxel_case("edges"))
    assert np.array_equal(dst[0], src[0]) and len(np.unique(fuse_ref.keys(dst[0]))) == len(dst[0])
    out, info = fuse_ref.fuse(dst, src)
    c, want = _expected("edges")
    n = len(c.a.t)
    assert np.array_equal(out[1].reshape(-1)[:n].view(np.uint32), want[0].view(np.uint32))
    assert info["voxels_copied"] == int(want[3].sum()) and info["voxels_averaged"] == int(want[4].sum())  # the padding adds none
    assert info["blocks_allocated"] == 0 and (dst[0] < 0).any() and (dst[0] > 0).any()


def test_list_cases_hold_what_they_are_for():
    long = fc.long_list()
    n = len(long.src[0])
    assert n == fc.N_LONG == 18469 and n > fc.CHUNK_FUSE > fc.WAVES and len(np.unique(fuse_ref.keys(long.src[0]))) == n
    shared = np.isin(fuse_ref.keys(long.src[0]), fuse_ref.keys(long.dst[0]))
    assert shared[:fc.CHUNK_FUSE].any() and shared[fc.CHUNK_FUSE:].any() and (~shared[fc.CHUNK_FUSE:]).any()
    assert shared[fc.WAVES:fc.CHUNK_FUSE].any() and (~shared[fc.WAVES:fc.CHUNK_FUSE]).any()
    assert (~np.isin(fuse_ref.keys(long.dst[0]), fuse_ref.keys(long.src[0]))).sum() == 5
    live = fuse_ref.contributes(long.src[1], long.src[2])
    assert (long.src[2]["weight"] == 0).any() and (~live & (long.src[2]["weight"] == 1)).any()
    st = long.extra["staged"]
    assert len(st.src[0]) == fc.N_STAGED == 4133 > 2 * fc.CHUNK_STAGE
    sh = np.isin(fuse_ref.keys(st.src[0]), fuse_ref.keys(st.dst[0]))
    for lo, hi in ((0, 2048), (2048, 4096), (4096, 4133)):
        assert sh[lo:hi].any() and (~sh[lo:hi]).any()

    for n, c in fc.short_lists().items():
        assert len(c.src[0]) == n
        own = fuse_ref.shard_owned(c.src[0], *fc.SHORT_SHARD)
        assert own[0] and (n == 1 or (0 < (~own).sum() < n))
        _, info = fuse_ref.fuse(c.dst, c.src, fc.SHORT_SHARD)
        assert info["blocks_allocated"] + info["blocks_skipped"] < n and info["voxels_averaged"] > 0
        if n >= 31:  # two new owned blocks in one home bucket: a second pass is certain
            new = c.src[0][own & ~np.isin(fuse_ref.keys(c.src[0]), fuse_ref.keys(c.dst[0]))]
            assert np.unique(fc.home_buckets(new, 9), return_counts=True)[1].max() >= 2

    run = fc.passes_run_out()
    col, others, held = run.extra["colliders"], run.extra["others"], run.extra["held"]
    assert len(set(fc.home_buckets(col, 9).tolist())) == 1 and len(col) - fc.PASSES >= 1
    rest = fc.home_buckets(np.concatenate([others, held]), 9)
    assert len(set(rest.tolist())) == len(rest) and run.extra["bucket"] not in set(rest.tolist())
    assert len(others) >= 24 and len(held) >= 12
    assert not np.isin(fuse_ref.keys(np.concatenate([col, others])), fuse_ref.keys(run.dst[0])).any()
    assert np.isin(fuse_ref.keys(held), fuse_ref.keys(run.dst[0])).all()
    # (the source engine of the map form has 2^16 buckets: there the colliders spread out)
    assert np.unique(fc.home_buckets(run.src[0], 16), return_counts=True)[1].max() <= fc.PASSES

    ch = fc.chained()
    per = np.unique(fc.home_buckets(ch.src[0], 9), return_counts=True)[1]
    assert len(ch.src[0]) == 700 and 3 <= per.max() <= fc.PASSES
    new = ch.src[0][~np.isin(fuse_ref.keys(ch.src[0]), fuse_ref.keys(ch.dst[0]))]
    assert len(new) == 350 and np.unique(fc.home_buckets(new, 9), return_counts=True)[1].max() >= 2
    print(f"chained: at most {per.max()} blocks per home bucket; passes_run_out: {len(col)} colliders")

    ps = fc.positions_and_shards()
    x = ps.src[0][:, 0].astype(int)
    assert {-4096, 4095} <= set(x.tolist()) and {-4096, 4095} <= set(ps.src[0][:, 1].tolist()) \
        and {-4096, 4095} <= set(ps.src[0][:, 2].tolist())
    assert ((ps.src[0].min(axis=1) < 0) & (ps.src[0].max(axis=1) > 0)).any()
    assert fc.effective_shard((1, 3, 0)) == (1, 3, 2) and fc.effective_shard((1, 3, 1)) == (1, 3, 1)
    for shard in fc.SHARD_SETTINGS:
        own = fuse_ref.shard_owned(ps.src[0], *fc.effective_shard(shard))
        assert (own & (x < 0)).any() and (own & (x >= 0)).any() and (~own & (x < 0)).any()
    owners = sum(fuse_ref.shard_owned(ps.src[0], r, 3, 2).astype(int) for r in range(3))
    assert (owners == 1).all()


@pytest.mark.parametrize("mistake", fc.MISTAKES)
def test_planted_mistakes_fail_a_named_case(mistake):
    caught = fc.failing_cases(mistake)
    print(f"{mistake}: fails {caught}")
    assert caught, mistake


def test_the_unchanged_restatement_fails_none():
    for name in fc.VOXEL_CASES:
        c = fc.voxel_case(name)
        assert fc.same_voxels(fc._fuse_voxels_with(*c.a, *c.b), fuse_ref.fuse_voxels(*c.a, *c.b)), name


def test_nan_payload_keyword():
    pos = np.zeros((1, 3), np.int16)
    c = np.zeros((1, 512), dtype=fc.RGBW_DTYPE)
    t = np.zeros((1, 512), F)
    t[0, 3] = np.nan
    other = t.copy()
    other.view(np.uint32)[0, 3] ^= 1  # another payload
    p = np.full((1, 512), 0.5, F)
    with pytest.raises(AssertionError):
        fuse_ref.assert_sets_match((pos, other, c, p), (pos, t, c, p))
    fuse_ref.assert_sets_match((pos, other, c, p), (pos, t, c, p), tsdf_nan_payload=False)
    other[0, 3] = 1.0
    with pytest.raises(AssertionError):
        fuse_ref.assert_sets_match((pos, other, c, p), (pos, t, c, p), tsdf_nan_payload=False)
    other[0, 3], other[0, 4] = np.nan, np.nan
    with pytest.raises(AssertionError):
        fuse_ref.assert_sets_match((pos, other, c, p), (pos, t, c, p), tsdf_nan_payload=False)
