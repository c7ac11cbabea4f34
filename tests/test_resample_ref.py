"""The numpy restatement of the resampling contract (tests/resample_ref.py) against hand-worked cases -- no GPU, no
engine: cases whose answer is an index shuffle of the source voxels, or a sum one can do on paper."""
import numpy as np

import fuse_ref
import resample_ref as rr
from ratsdf._abi import RGBW_DTYPE

F = np.float32
VS = 2.0 ** -6  # a power of two: Ti.t / vs is exact for whole-voxel translations
IDENTITY = (0, 0, 0, 1, 0, 0, 0)


def one_block(seed=3, pos=(0, 0, 0)):
    """a source of one block: random tsdf / colour / prob, weights 0 .. 40 with zeros and fresh voxels among them"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1, 1, (1, 512)).astype(F)
    c = np.zeros((1, 512), dtype=RGBW_DTYPE)
    for ch in ("r", "g", "b"):
        c[ch] = rng.integers(0, 256, (1, 512))
    c["weight"] = rng.integers(0, 41, (1, 512))
    fresh = rng.random((1, 512)) < 0.1
    t[fresh], c["weight"][fresh] = F(-1), 1
    p = rng.uniform(0.05, 0.95, (1, 512)).astype(F)
    return np.array([pos], dtype=np.int16), t, c, p


def voxel_table(block_set):
    """{(x, y, z): (tsdf, rgbw, prob)} of the contributing voxels"""
    pos, t, c, p = block_set
    live = fuse_ref.contributes(t, c)
    out = {}
    for b in range(len(pos)):
        for v in np.flatnonzero(live[b]):
            key = (int(pos[b][0]) * 8 + (v & 7), int(pos[b][1]) * 8 + ((v >> 3) & 7), int(pos[b][2]) * 8 + (v >> 6))
            out[key] = (t[b, v], c[b, v], p[b, v])
    return out


def assert_is_shuffle(pose, src, mapping):
    """under `pose` the resampled map holds exactly source voxel s at destination mapping(s), all three words"""
    res, cnt = rr.blocks_with_contribution(pose, VS, src)
    want = {mapping(k): v for k, v in voxel_table(src).items()}
    got = voxel_table(res)
    assert int(cnt.sum()) == len(want) and set(got) == set(want)
    for k, (t, c, p) in want.items():
        assert got[k][0].tobytes() == t.tobytes() and got[k][1] == c and got[k][2].tobytes() == p.tobytes(), k
    # a voxel that does not contribute is three zero words
    live = fuse_ref.contributes(res[1], res[2])
    assert int(live.sum()) == len(want)
    assert not rr.records(res)[np.tile(~live, (1, 3))].any()
    return res


def test_pose_arithmetic_is_exact_where_it_must_be():
    q, t = rr.transform(IDENTITY, VS)
    assert q == (0, 0, 0, 1) and t == (0, 0, 0)
    q, t = rr.transform((0, 0, 0, 1, 3 * VS, 0, -5 * VS), VS)
    assert tuple(float(v) for v in t) == (-3.0, 0.0, 5.0)
    v = (F(3), F(-4), F(5))
    assert rr.quat_rotate((F(0), F(0), F(1), F(0)), v) == (F(-3), F(4), F(5))
    assert rr.pose_ok(IDENTITY) and not rr.pose_ok((0, 0, 0, 1.01, 0, 0, 0)) and not rr.pose_ok((0, 0, 0, 1, np.nan, 0, 0))
    assert rr.pose_ok((0, 0, 0, 1.0004, 0, 0, 0)) and not rr.pose_ok((0, 0, 0, 0, 0, 0, 0))


def test_identity_is_a_copy_of_the_contributing_voxels():
    src = one_block()
    res = assert_is_shuffle(IDENTITY, src, lambda k: k)
    # a lone block next to unallocated space loses nothing: one needed corner per voxel
    assert np.array_equal(res[0], src[0])
    live = fuse_ref.contributes(src[1], src[2])
    assert np.array_equal(rr.records(res)[np.tile(live, (1, 3))], rr.records(src)[np.tile(live, (1, 3))])


def test_a_shift_by_whole_voxels_moves_voxels_across_block_faces():
    src = one_block()
    res = assert_is_shuffle((0, 0, 0, 1, 3 * VS, 0, -5 * VS), src, lambda k: (k[0] + 3, k[1], k[2] - 5))
    assert sorted(map(tuple, res[0].tolist())) == [(0, 0, -1), (0, 0, 0), (1, 0, -1), (1, 0, 0)]


def test_half_a_turn_about_z_mirrors_the_indices():
    src = one_block(pos=(1, -2, 3))
    res = assert_is_shuffle((0, 0, 1, 0, 0, 0, 0), src, lambda k: (-k[0], -k[1], k[2]))
    # source x in 8 .. 15 lands on -15 .. -8 (blocks -2 and, for x = 8 alone, -1), y in -16 .. -9 on 9 .. 16
    assert {tuple(b) for b in res[0].tolist()} == {(-2, 1, 3), (-2, 2, 3), (-1, 1, 3), (-1, 2, 3)}


def test_a_fraction_that_rounds_to_one_needs_only_the_upper_corner():
    """t = 1e-9 voxels: g = d - 1e-9 is d for every d but 0, where g = -1e-9, l = -1 and f = g - l rounds to 1.0f: the
    lower corner (in the unallocated block -1) has the factor u = 0 and is not needed"""
    pose = (0, 0, 0, 1, 1e-9 * VS, 1e-9 * VS, 1e-9 * VS)
    G = rr.transform(pose, VS)
    g = rr.se3_apply(G, (F(0), F(0), F(0)))
    assert all(v < 0 and np.floor(v) == -1 and v - np.floor(v) == F(1) for v in g)
    src = one_block()
    assert_is_shuffle(pose, src, lambda k: k)


def test_half_a_voxel_along_x_by_hand():
    src = one_block(seed=5)
    tab = voxel_table(src)
    res, _ = rr.blocks_with_contribution((0, 0, 0, 1, 0.5 * VS, 0, 0), VS, src)
    got = voxel_table(res)
    n_checked = 0
    for (x, y, z) in [(k[0] + 1, k[1], k[2]) for k in tab] + [(0, 0, 0), (8, 3, 3)]:
        lo, hi = tab.get((x - 1, y, z)), tab.get((x, y, z))  # g.x = x - 0.5: l = x - 1, f = u = 0.5
        if lo is None or hi is None:
            assert (x, y, z) not in got  # (x = 0 leans on block -1, x = 8 on block 1: unallocated)
            continue
        t = lo[0] * F(0.5) + hi[0] * F(0.5)
        near = hi  # roundf(x - 0.5) = x for x >= 1: half away from zero
        c = near[1].copy()
        c["weight"] = min(lo[1]["weight"], hi[1]["weight"])
        assert got[(x, y, z)][0] == F(t) and got[(x, y, z)][1] == c and got[(x, y, z)][2] == near[2]
        n_checked += 1
    assert n_checked > 100


def test_out_of_range_voxels_vanish():
    """a source block at block coordinate 4095 pushed past the int16 range: nothing wraps around to -4096"""
    src = one_block(pos=(4095, 0, 0))
    res, cnt = rr.blocks_with_contribution((0, 0, 0, 1, 4 * VS, 0, 0), VS, src)
    tab, got = voxel_table(src), voxel_table(res)
    want = {(k[0] + 4, k[1], k[2]): v for k, v in tab.items() if k[0] + 4 <= 32767}  # (the lattice ends at 32767)
    assert set(got) == set(want) and len(want) < len(tab)
    assert all(b[0] == 4095 for b in res[0].tolist())
    # ... and the restatement itself, asked for the block at -4096, finds nothing there
    _, cnt = rr.resample_blocks((0, 0, 0, 1, 4 * VS, 0, 0), VS, [(-4096, 0, 0)], rr.set_lookup(src))
    assert cnt.tolist() == [0]
    # the range rule is on l: under the identity the voxels at x = 32767 (l = 32767 > 32766) do not contribute
    got = voxel_table(rr.blocks_with_contribution(IDENTITY, VS, src)[0])
    assert set(got) == {k for k in tab if k[0] <= 32766} and len(got) < len(tab)
