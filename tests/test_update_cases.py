"""The crafted update cases of tests/update_cases.py on the CPU oracle alone (no GPU): the cases hold what they are for,
the numpy restatement of the update predicate counts the oracle's updated voxels, a voxel that does not update keeps its
three words, the carve verdicts are the reference's rule, and the oracle's tsdf and weight are the reference's expression
(voxel_tsdf.cu:228, 236, 238) evaluated in float64 -- which pins the oracle to the formula and not only to itself.
tests/test_gpu_update_cases.py then holds the HIP engine against the oracle on the same cases."""
import numpy as np
import pytest

import update_cases as uc
from update_cases import F


def run_oracle(pool, lib):
    """[(before, after, stats)] per frame: the oracle's map as a block set around each of the case's frames"""
    from fuse_ref import dump_set
    from ratsdf._abi import Engine
    cs = uc.case(pool)
    e = Engine(lib, uc.VS, uc.TRUNC, threads=4, **uc.CFG)
    try:
        e.import_blocks(*cs.blocks)
        out = []
        for fr in cs.frames:
            before = dump_set(e)
            e.integrate(*fr.args())
            out.append((before, dump_set(e), e.last_frame_stats()))
        return out
    finally:
        e.close()


@pytest.fixture(scope="module")
def runs(oracle_lib):
    made = {}

    def get(pool):
        if pool not in made:
            made[pool] = run_oracle(pool, oracle_lib)
        return made[pool]
    return get


def with_fresh(before, after):
    """`before` and, as fresh blocks (-1, weight 1, 0.5), the blocks that only `after` holds"""
    from ratsdf._abi import RGBW_DTYPE
    new = ~uc.align(before, after)[1] if len(before[0]) else np.ones(len(after[0]), bool)
    n = int(new.sum())
    c = np.zeros((n, 512), dtype=RGBW_DTYPE)
    c["weight"] = 1
    return (np.concatenate([before[0], after[0][new]]), np.concatenate([before[1], np.full((n, 512), -1, F)]),
            np.concatenate([before[2], c]), np.concatenate([before[3], np.full((n, 512), 0.5, F)]))


@pytest.mark.parametrize("pool", uc.POOLS)
def test_every_entry_meets_every_situation(pool):
    """the guards against a vacuous pass: per entry of the pool's table at least 8 voxels that update, 8 that do not,
    8 beside an updating partner, 8 in a pair of which exactly one updates, and both x parities; several hundred pairs
    with exactly one updating voxel; no carve block is ever updated"""
    cs = uc.case(pool)
    occ = uc.occurrences(cs)
    names = ("updated", "untouched", "partner updates", "one of a pair", "even x", "odd x")
    for j, row in enumerate(occ):
        for k in range(4):
            assert row[k] >= 8, f"{pool}: entry {j} {uc.ENTRIES[pool][j]} has {row[k]} voxels '{names[k]}'"
        assert row[4] >= 8 and row[5] >= 8, (pool, j, row)
    upd = uc.predict(cs.blocks[0][:cs.n_pool], cs.frames[0]).upd
    pairs = uc.one_of_a_pair(upd)
    print(f"{pool}: {len(occ)} entries, least counts {occ.min(axis=0).tolist()} {names}; frame 0 updates "
          f"{int(upd.sum())} pool voxels, {pairs} lane pairs with exactly one updating voxel")
    assert pairs >= (1000 if pool == "holes" else 300), pairs
    for fr in cs.frames:
        assert not uc.predict(cs.blocks[0][cs.n_pool:], fr).upd.any()
    if pool in ("weights", "wnew"):  # w_new = 0 and ~2.4e-7 over weights 0 and 255
        wn_at = [uc.predict(cs.blocks[0][:cs.n_pool], fr) for fr in (cs.frames if pool == "weights" else cs.frames[:1])]
        w = cs.blocks[2]["weight"][:cs.n_pool]
        for wo in (0, 255):
            for wn in (F(0), ((F(1) - F(uc.MD_PRED) / F(uc.MD)) * F(4))):
                n = sum(int((p.upd & (w == wo) & (p.wn == wn)).sum()) for p in wn_at)
                assert n >= 8, (pool, wo, float(wn), n)
                assert 0 <= wn < 3e-7


def test_the_carve_verdicts_are_the_rule():
    names, pos, t, w, verdict = uc.carve_blocks()
    assert len(names) == 14 and len(np.unique(uc.keys(pos))) == 14
    want = dict(zip(names, verdict.tolist()))
    assert want == {"NaN only": False, "NaN with one 0.95": True, "0.9f": True, "0.9f with one predecessor": False,
                    "-0.9f": True, "+inf": True, "inf mixed with NaN": True, "the fresh word": True,
                    **{f"1.0 with 0.5 at voxel {at}": False for at in uc.SINGLE_LOW_AT}}
    # the four waves of a block at two voxels per lane: voxel 2 (64 w + l) + j
    assert sorted({at // 128 for at in uc.SINGLE_LOW_AT}) == [0, 1, 2, 3] and {at & 1 for at in uc.SINGLE_LOW_AT} == {0, 1}


@pytest.mark.parametrize("pool", uc.POOLS)
def test_oracle_counts_carves_and_keeps(pool, runs):
    """updated_voxels is the restated mask's sum, the carve blocks go by the rule, deleted_blocks counts what left, and
    what a frame does not update keeps its words"""
    cs = uc.case(pool)
    _, cpos, _, _, verdict = uc.carve_blocks()
    for i, (before, after, stats) in enumerate(runs(pool)):
        fr = cs.frames[i]
        if i == 0:
            assert uc.words(uc.by_position(before)).tobytes() == uc.words(uc.by_position(cs.blocks)).tobytes()
        known = with_fresh(before, after)
        n_upd = int(uc.predict(known[0], fr).upd.sum())
        gone = ~np.isin(uc.keys(before[0]), uc.keys(after[0]))
        print(f"{pool} frame {i}: {stats}; restated updates {n_upd}, {int(gone.sum())} known blocks left the map")
        if i == 0 and pool not in ("wnew", "far"):
            # every visible block is an imported one: the restated mask is the whole count
            assert stats["allocated_blocks"] == 0
            assert stats["updated_voxels"] == n_upd
            assert stats["deleted_blocks"] == int(gone.sum())
        else:
            # blocks allocated and carved within the frame (fresh blocks wholly behind the surface, or updated at
            # w_new ~ 0) are in neither dump: their updates and deletions come on top
            assert stats["updated_voxels"] >= n_upd > 0
            assert stats["deleted_blocks"] >= int(gone.sum())
            if i == 1:
                assert stats["allocated_blocks"] > 0
        if i == 0 and pool == "far":  # the numerator -0 is met: prior -0, w_new 0, ts < 0
            pr = uc.predict(cs.blocks[0][:cs.n_pool], fr)
            t0, w0 = cs.blocks[1][:cs.n_pool], cs.blocks[2]["weight"][:cs.n_pool]
            at = pr.upd & (uc.bits(t0) == 0x80000000) & (w0 > 0) & (pr.wn == 0) & (pr.ts < 0)
            assert at.sum() >= 16, int(at.sum())
            a, held = uc.align(after, cs.blocks)
            assert held[:cs.n_pool].all() and (uc.bits(after[1][a[:cs.n_pool]])[at] == 0x80000000).all()
        if i == 0:
            left = np.isin(uc.keys(cpos), uc.keys(before[0][gone]))
            assert np.array_equal(left, verdict), (left, verdict)
        else:  # the survivors are judged again, with the same outcome
            assert np.isin(uc.keys(cpos[~verdict]), uc.keys(after[0])).all()
        assert uc.untouched_unchanged(before, after, fr) >= 1000


@pytest.mark.parametrize("pool", uc.POOLS)
def test_oracle_follows_the_formula(pool, runs):
    """updated voxels with finite results: tsdf within the four float32 roundings of (t wo + ts wn) / wc evaluated in
    float64, weight min(round(wc), 40) exactly"""
    cs = uc.case(pool)
    worst, n = 0.0, 0
    for i, (before, after, stats) in enumerate(runs(pool)):
        known = with_fresh(before, after)
        at, held = uc.align(known, after)
        assert held.all()
        prior = tuple(a[at] for a in known)
        upd, q, bound, w = uc.formula_float64(prior, cs.frames[i])
        got_t, got_w = after[1].astype(np.float64), after[2]["weight"]
        # finite in float32: the numerator does not overflow (bound * wc is sum |products| * 2^-22) and wc is not 0
        with np.errstate(all="ignore"):
            fin = upd & np.isfinite(q) & (bound * (prior[2]["weight"].astype(F) + uc.predict(prior[0], cs.frames[i]).wn)
                                          <= uc.FLT_MAX * 2.0 ** -22)
        assert np.isfinite(got_t[fin]).all(), f"{pool} frame {i}: a finite quotient came out not finite"
        with np.errstate(invalid="ignore"):
            err = np.abs(got_t - q)
        # (below FLT_MIN a rounding is half a subnormal step, not 2^-24 of the value)
        ok = err <= bound + np.where(np.abs(q) < uc.FLT_MIN, 2.0 ** -149, 0.0)
        assert ok[fin].all(), (f"{pool} frame {i}: {int((~ok & fin).sum())} voxels off the formula, worst "
                               f"{float((err - bound)[fin].max()):.3e} over its bound")
        wfin = upd & np.isfinite(w)
        assert np.array_equal(got_w[wfin], w[wfin].astype(np.uint8)), f"{pool} frame {i}: weights"
        rel = err[fin & (bound > 0)] / bound[fin & (bound > 0)]
        worst, n = max(worst, float(rel.max()) if rel.size else 0.0), n + int(fin.sum())
    print(f"{pool}: {n} updated voxels with finite results, worst tsdf error {worst:.3f} of its bound")
    assert n >= (10000 if pool != "far" else 1000)
