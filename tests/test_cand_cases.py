"""The crafted candidate-pass cases of tests/cand_cases.py without a GPU: every case reaches what it is named for, shown
on the numpy restatement of the sample chain or on the CPU oracle (never on the engine under test), and the restatement
is pinned to the oracle: on an empty map a frame allocates exactly the distinct owned blocks of the restated samples
that pass the full-frustum test, one per directory bucket.  tests/test_gpu_cand_cases.py then holds the HIP engine
against the oracle on the same cases."""
import numpy as np
import pytest

import cand_cases as cc
from cand_cases import F


def oracle_stats(lib, case, frames=None, fresh=False):
    """the oracle's frame statistics for the frames of the case (fresh: every frame on an empty map)"""
    from ratsdf._abi import Engine
    out, e = [], None
    try:
        for fr in case.frames if frames is None else frames:
            if e is None or fresh:
                if e is not None:
                    e.close()
                e = Engine(lib, case.vs, case.trunc, threads=4, **case.engine_kw())
            e.integrate(*fr.args())
            out.append(e.last_frame_stats())
    finally:
        if e is not None:
            e.close()
    return out


def chains(case):
    return [cc.chain(fr.depth, fr.md, fr.intr, fr.pose, case.vs, case.trunc) for fr in case.frames]


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against the oracle
PINNED = ([cc.ragged(W, H) for W, H in ((17, 5), (250, 157), (353, 97))] + [cc.steps_case(t) for t in cc.STEP_TRUNCS] +
          [cc.far_case(n) for n in cc.FAR] + [cc.shard_case(3, 1, 1), cc.shard_case(7, 3, 0), cc.shard_case(7, 3, 5)])


@pytest.mark.parametrize("case", PINNED, ids=lambda c: c.name)
def test_restated_samples_allocate_what_the_oracle_allocates(case, oracle_lib):
    """every frame of the case on an EMPTY oracle map: allocated_blocks is the restatement's count"""
    got = oracle_stats(oracle_lib, case, fresh=True)
    for i, fr in enumerate(case.frames):
        want, distinct = cc.first_frame_allocations(case, fr)
        print(f"{case.name} frame {i}: {distinct} distinct visible owned blocks in {want} buckets; the oracle allocated "
              f"{got[i]['allocated_blocks']}")
        assert got[i]["allocated_blocks"] == want, (case.name, i)


def test_restated_samples_allocate_what_the_oracle_allocates_at_hd(oracle_lib):
    case = cc.ragged(1000, 600)
    got = oracle_stats(oracle_lib, case, frames=case.frames[:1])
    want, _ = cc.first_frame_allocations(case, case.frames[0])
    assert got[0]["allocated_blocks"] == want and want > 2000, (got[0], want)


# ---------------------------------------------------------------------------------------------------------------------
# ragged sizes
def test_ragged_sizes_are_the_share_forms_they_are_named_for():
    """premises on plain arithmetic: the super-tile counts, and where the shipped split (10 % below 600 000 pixels, all
    of it from there on) puts the first tile of share C"""
    sup = {f"{W}x{H}": cc.supers_of(W, H) for W, H in cc.RAGGED_SMALL + cc.RAGGED_HD}
    assert sup["250x157"] == 160 and sup["353x97"] == 161
    assert sup["999x600"] == sup["1000x600"] == 2394 and sup["1001x601"] == 2394 and 2394 % 16 == 10
    assert 999 * 600 < 600000 <= 1000 * 600
    share_a = lambda s: s * 10 // 100 // 16 * 16  # super-tiles of A at the shipped split
    assert share_a(159) == 0 and share_a(160) == 16   # 250x157: the smallest with a non-empty A
    assert (161 - share_a(161)) % 16 == 1              # 353x97: C ends in a partial group of workgroups
    assert (sup["17x5"], sup["1x300"], sup["300x1"]) == (2, 19, 19)
    for W, H in cc.RAGGED_HD:
        assert len(cc.tail_supers(W, H)) == 10


@pytest.mark.parametrize("size", cc.RAGGED_SMALL + cc.RAGGED_HD, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_super_tile_asks_for_its_own_blocks_in_every_frame(size):
    """premise on the restatement: the planes differ from super-tile to super-tile and from frame to frame (nine in ten
    super-tiles, at the least, ask for a block that no other super-tile of the frame asks for), and noise makes every
    frame's texels its own"""
    case = cc.ragged(*size)
    assert 3 <= len(case.frames) <= 4
    s = cc.super_index(case.W, case.H).reshape(-1)
    for i, (fr, ch) in enumerate(zip(case.frames, chains(case))):
        for a, b in zip(case.frames[:i], case.frames[i + 1:]):
            assert not np.array_equal(a.depth, b.depth) and not np.array_equal(a.rgb, b.rgb)
        if not ch.valid.any():
            continue
        keys = cc.block_key(ch.block)
        sup = s[ch.pixel]
        lit = np.unique(sup)
        # super-tiles with a block nobody else asks for (a few, one pixel wide at a ragged edge, have none)
        order = np.argsort(keys, kind="stable")
        k_sorted, s_sorted = keys[order], sup[order]
        starts = np.flatnonzero(np.r_[True, k_sorted[1:] != k_sorted[:-1]])
        ends = np.r_[starts[1:], len(k_sorted)]
        own = [s_sorted[a] for a, b in zip(starts, ends) if (s_sorted[a:b] == s_sorted[a]).all()]
        frac = len(np.unique(own)) / len(lit)
        print(f"{case.name} frame {i}: {len(lit)} super-tiles with depth, {frac:.0%} of them ask for a block of their own")
        assert frac >= 0.9 or len(lit) < 8, (case.name, i, frac)


@pytest.mark.parametrize("size", cc.RAGGED_HD, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_last_super_tiles_ask_for_blocks_nothing_else_asks_for(size):
    """premise on the restatement: in every frame after the first, the pixels of the last supers % 16 super-tiles request
    blocks that no other pixel of the frame and no earlier frame requests, and some of them pass the frustum test (they
    are allocated); the last frame has depth only there"""
    case = cc.ragged(*size)
    s = cc.super_index(case.W, case.H)
    tail = np.isin(s, cc.tail_supers(case.W, case.H))
    assert (case.frames[-1].depth[~tail] == 0).all() and (case.frames[-1].depth[tail] > 0).all()
    got = cc.tail_requests(case)
    print(f"{case.name}: (blocks only the tail requests, of them fully visible) per frame after the first: {got}")
    assert len(got) == len(case.frames) - 1
    for own, visible in got:
        assert own >= 1 and visible >= 1, got


def test_the_last_super_tiles_allocate_on_the_oracle(oracle_lib):
    """premise on the oracle: the last frame of an HD case, whose depth lies in the tail super-tiles only, allocates"""
    for W, H in cc.RAGGED_HD:
        st = oracle_stats(oracle_lib, cc.ragged(W, H))
        print(f"{W}x{H}: allocated per frame {[s['allocated_blocks'] for s in st]}, updated voxels "
              f"{[s['updated_voxels'] for s in st]}")
        assert all(s["allocated_blocks"] > 0 and s["updated_voxels"] > 0 for s in st)


# ---------------------------------------------------------------------------------------------------------------------
# ray sampling
def test_steps_take_every_value_up_to_seven_and_some_above_eight():
    seen = set()
    for t in cc.STEP_TRUNCS:
        case = cc.steps_case(t)
        S = cc.max_samples(case)
        for ch in chains(case):
            st = ch.steps[ch.valid]
            assert st.min() >= 1 and st.max() < S, (t, int(st.max()), S)  # steps < S everywhere
            seen |= set(np.unique(st).tolist())
        print(f"truncation {t} voxels: S = {S}, steps seen so far {sorted(seen)}")
    assert set(range(1, 8)) <= seen, sorted(seen)
    above = {s for s in seen if s > 8}
    assert above, sorted(seen)
    assert 8 in seen and any(s & (s - 1) for s in above)  # the exact-reciprocal and the division branch above 2
    assert any(s > 2 and s & (s - 1) == 0 for s in seen) and any(s > 2 and s & (s - 1) for s in seen)


# ---------------------------------------------------------------------------------------------------------------------
# far and wrapped coordinates
def test_far_cases_reach_the_forms_they_are_named_for(oracle_lib):
    """premises on the restatement (which rounding / division form the samples call for) and on the oracle (blocks are
    allocated through the wrapped samples)"""
    for name in cc.FAR:
        case = cc.far_case(name)
        st = oracle_stats(oracle_lib, case)
        ch = chains(case)[0]
        v = ch.valid
        with np.errstate(all="ignore"):
            reach = np.max([np.abs(ch.sg[a]) + np.abs(ch.rg[a]) for a in range(3)], axis=0)
            start = np.max([np.abs(ch.sw[a]) for a in range(3)], axis=0)
        wraps = (ch.unwrapped != ch.voxel).any(axis=1)
        print(f"{name}: allocated on the oracle {[s['allocated_blocks'] for s in st]}, deleted "
              f"{[s['deleted_blocks'] for s in st]}; samples reach {reach[v].min():.3g} .. {reach[v].max():.3g} voxels, "
              f"{int(wraps.sum())} of {len(wraps)} wrap")
        assert all(s["allocated_blocks"] > 0 for s in st), (name, st)
        if name.startswith("wrap"):
            assert wraps.all() and (reach[v] < F(1e9)).all()          # the short rounding form, wrapped
            assert (np.abs(ch.unwrapped[:, 0 if "x" in name else 2]) > 65000).all()
        elif name == "at1e9":  # pixels on both sides of the long form's threshold; nothing saturates
            assert (reach[v] >= F(1e9)).sum() >= 1000 and (reach[v] < F(1e9)).sum() >= 1000
            assert (np.abs(ch.unwrapped) < 2147483647).all()
            assert (start[v] < F(1e18)).all()
        elif name == "beyond1e9":
            assert (reach[v] >= F(1e9)).all() and (np.abs(ch.unwrapped) < 2147483647).all() and (start[v] < F(1e18)).all()
        elif name == "saturated":
            assert (reach[v] >= F(1e9)).all() and (np.abs(ch.unwrapped[:, 2]) >= 2147483647).all()
        elif name == "beyond1e18":
            assert (start[v] >= F(1e18)).all()                                                # IEEE division
        else:  # waves of both kinds in one pass: left half near, right half far, in every 16-pixel tile row
            left = np.zeros(v.shape, bool)
            left[:, :case.W // 2] = True
            assert (reach[v & left] < F(1e9)).all() and (reach[v & ~left] >= F(1e9)).all()
            assert v[:, :case.W // 2].any() and v[:, case.W // 2:].any()


# ---------------------------------------------------------------------------------------------------------------------
# shards
@pytest.mark.parametrize("count,bits", cc.SHARDS)
def test_shard_scenes_straddle_slab_borders(count, bits, oracle_lib):
    """premises: the scene spans negative and positive x; pixels whose skip interval holds a slab border exist, and
    pixels that a rank skips, for every rank; every rank's oracle allocates; the ranks' allocations add up to the
    unsharded map's (restatement: ownership partitions the blocks)"""
    total = 0
    for rank in range(count):
        case = cc.shard_case(count, bits, rank)
        fr = case.frames[0]
        ch = chains(case)[0]
        assert ch.block[:, 0].min() < -8 and ch.block[:, 0].max() > 8
        valid, inside, straddles = cc.shard_skip_clause(case, fr)
        assert inside[valid].all() and straddles[valid].sum() >= 100
        mine = cc.owned(ch.block, **case.shard)
        pix_mine = np.zeros(case.W * case.H, bool)
        pix_mine[ch.pixel[mine]] = True
        assert pix_mine.sum() >= 50 and (~pix_mine & valid.reshape(-1)).sum() >= 50, (rank, int(pix_mine.sum()))
        st = oracle_stats(oracle_lib, case, frames=case.frames[:1])
        assert st[0]["allocated_blocks"] > 0, (count, bits, rank)
        total += cc.first_frame_allocations(case, fr)[1]
    whole = cc.Case("whole", "shards", case.W, case.H, case.vs, case.trunc, case.cfg, {}, case.frames)
    assert total == cc.first_frame_allocations(whole, case.frames[0])[1]


def test_sharded_wrap_cases_allocate_and_the_sideways_one_never_skips(oracle_lib):
    """the 1 cm int16-wrap cases split three ways: every rank's oracle allocates through the wrapped samples; with the
    camera 65 536 voxels down the world's x axis every pixel's x interval lies outside the shorts' range (the skip's clause "never
    skip"), while the restated blocks' wrapped x belongs to every rank in turn"""
    for name in ("wrap1cm", "wrapx1cm"):
        for rank in range(3):
            case = cc.far_case(name, cc.sharded3(rank))
            valid, inside, _ = cc.shard_skip_clause(case, case.frames[0])
            assert valid.all()
            if name == "wrapx1cm":
                assert not inside.any()
                ch = chains(case)[0]
                mine = cc.owned(ch.block, **case.shard)
                assert mine.sum() >= 100 and (~mine).sum() >= 100
            st = oracle_stats(oracle_lib, case)
            print(f"{name} rank {rank} of 3: allocated on the oracle {[s['allocated_blocks'] for s in st]}")
            assert all(s["allocated_blocks"] > 0 for s in st)
