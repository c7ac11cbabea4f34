"""The numpy restatement of the coarsening contract (tests/coarsen_ref.py) checked against itself and against what the
contract promises, without a GPU: the GPU tests compare the engine with it, so it has to be right first."""
import numpy as np

import coarsen_ref as cr
import fuse_ref
from ratsdf._abi import RGBW_DTYPE
from test_gpu_resample import craft

F = np.float32


def _fine_grid(block_pos):
    """integer grid indices of the voxels of fine blocks [n, 3], record order: (n, 512, 3)"""
    b = np.asarray(block_pos, dtype=np.int64).reshape(-1, 3)
    v = np.arange(512)
    local = np.stack([v & 7, (v >> 3) & 7, v >> 6], axis=1)
    return b[:, None, :] * 8 + local[None, :, :]


def test_a_linear_field_is_reproduced_at_the_centre():
    """t = n.x - d with all taps present and equal weights: full weighting of a linear field is the centre's value.
    Bound 4e-6: 27 products and 26 additions each round at 2^-24 of a partial sum no larger than den (the values are in
    [-1, 1]): 54 * 2^-24 = 3.2e-6, and the division adds 6e-8."""
    rng = np.random.default_rng(3)
    # fine blocks 1 .. 4 per axis: coarse block (1, 1, 1) has every tap (its region is fine blocks 1 .. 3)
    pos = np.array([(x, y, z) for z in range(1, 5) for y in range(1, 5) for x in range(1, 5)], dtype=np.int16)
    g = _fine_grid(pos).astype(np.float64)
    worst = 0.0
    for trial in range(20):
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        field = g @ nrm
        field = (field - field.mean()) / np.abs(field - field.mean()).max()  # in [-1, 1]
        t = field.astype(F)
        c = np.zeros(t.shape, dtype=RGBW_DTYPE)
        c["weight"] = int(rng.integers(2, 256))  # (weight 1 on a tsdf of -1 would be the fresh voxel)
        p = np.full(t.shape, 0.5, dtype=F)
        (_, ct, cc, _), cnt = cr.coarsen_blocks((pos, t, c, p), [(1, 1, 1)])
        assert cnt[0] == 512
        # the centre of coarse voxel D = 8 + local is fine voxel 2D = 16 + 2 * local: block 2 + (local >> 2)
        D = 8 + np.stack([np.arange(512) & 7, (np.arange(512) >> 3) & 7, np.arange(512) >> 6], axis=1)
        lookup = {tuple(int(v) for v in pos[i]): i for i in range(len(pos))}
        centre = np.array([t[lookup[tuple((2 * d) >> 3)], ((2 * d[0]) & 7) + 8 * ((2 * d[1]) & 7) + 64 * ((2 * d[2]) & 7)]
                           for d in D], dtype=F)
        worst = max(worst, float(np.abs(ct[0].astype(np.float64) - centre.astype(np.float64)).max()))
        assert np.array_equal(cc[0]["weight"], np.full(512, c["weight"][0, 0]))
    print(f"linear fields: largest |coarse - centre| = {worst:.3e}")
    assert worst <= 4e-6


def test_branch_free_form_equals_the_form_that_skips_absent_taps():
    """every word, on a map with missing blocks, weight-0 voxels and fresh voxels; also a check of the block slicing of
    coarsen_blocks against the contract read one voxel at a time"""
    src = craft([(2, 1, -1), (3, 1, -1), (2, 2, 0), (-7, -3, -8), (-8, -3, -8), (5, 5, 5)], seed=7)
    assert (src[2]["weight"] == 0).any() and (~fuse_ref.contributes(src[1], src[2]) & (src[2]["weight"] == 1)).any()
    offered = np.array([(1, 0, -1), (1, 1, 0), (-4, -2, -4), (2, 2, 2), (3, 2, 2), (0, 0, 0)], dtype=np.int16)
    (_, t, c, p), cnt = cr.coarsen_blocks(src, offered)
    blocks = cr.block_dict(src)
    n_contrib = n_partial = 0
    for bi, B in enumerate(offered.astype(np.int64)):
        for v in range(512):
            D = (8 * B[0] + (v & 7), 8 * B[1] + ((v >> 3) & 7), 8 * B[2] + (v >> 6))
            got = cr.coarsen_voxel_skipping(blocks, D)
            if got is None:
                assert t[bi, v].view(np.uint32) == 0 and c[bi, v].tobytes() == bytes(4) and p[bi, v].view(np.uint32) == 0
                continue
            n_contrib += 1
            assert got[0].view(np.uint32) == t[bi, v].view(np.uint32), (B, v, got[0], t[bi, v])
            assert got[1].tobytes() == c[bi, v].tobytes() and got[2].view(np.uint32) == p[bi, v].view(np.uint32)
    taps = cr.present_taps(src, offered)
    n_partial = int((taps[:, :, 13] & (taps.sum(axis=2) < 27)).sum())
    assert n_contrib == int(cnt.sum()) and n_contrib > 300 and n_partial > 100
    assert cnt[-1] == 0  # (0, 0, 0): no source block near it


def test_an_absent_centre_gives_three_zero_words():
    """whatever the neighbours hold: weight 0, the fresh voxel, or a centre in a block the map does not have"""
    src = craft([(2, 2, 2), (3, 2, 2)], seed=9)
    pos, t, c, p = (a.copy() for a in src)
    c["weight"][:] = np.maximum(c["weight"], 2)        # everything contributes ...
    t[:] = np.where(t == F(-1), F(-0.5), t)
    # ... except three centres of coarse block (1, 1, 1): fine voxel (16 + 2x, 16 + 2y, 16 + 2z)
    c["weight"][0, 0] = 0                               # coarse local (0, 0, 0): weight 0
    c["weight"][0, 2], t[0, 2] = 1, F(-1)               # coarse local (1, 0, 0): the fresh voxel
    (_, ct, cc, cp), cnt = cr.coarsen_blocks((pos, t, c, p), [(1, 1, 1), (1, 2, 1)])
    rec = cr.records((None, ct, cc, cp))
    for v in (0, 1):
        assert not rec[0, [v, 512 + v, 1024 + v]].any()
    # coarse block (1, 2, 1): its centres lie in fine blocks (2..3, 4..5, 2..3), none allocated; the halo plane
    # y = 31 of fine block (2, 3, 2) is not there either, and (2, 2, 2)'s voxels end at y = 23
    assert cnt[1] == 0 and not rec[1].any()
    # the centres of local y = 4 .. 7 (z likewise) of (1, 1, 1) lie in fine block (2, 3, 2): absent, although y = 23
    # is a tap
    ys, zs = (np.arange(512) >> 3) & 7, np.arange(512) >> 6
    assert not rec[0].reshape(3, 512)[:, (ys >= 4) | (zs >= 4)].any() and cnt[0] == 128 - 2
    assert cr.present_taps((pos, t, c, p), [(1, 1, 1)])[0][ys == 4].any()


def test_candidates_are_the_halved_positions_once():
    pos = np.array([(2, 1, -1), (3, 1, -1), (3, 0, -2), (-7, -3, -8), (-8, -3, -7), (4095, 4095, 4095),
                    (-4096, -4096, -4096), (-1, -1, -1), (0, 0, 0), (1, 1, 1)], dtype=np.int16)
    got = cr.candidates(pos)
    want = sorted({(x >> 1, y >> 1, z >> 1) for x, y, z in pos.astype(int).tolist()}, key=lambda b: (b[2], b[1], b[0]))
    assert got.dtype == np.int16 and got.tolist() == [list(b) for b in want]
    assert (-4, -2, -4) in want and (-1, -1, -1) in want and (2047, 2047, 2047) in want and (-2048, -2048, -2048) in want
    assert len(got) == 6
    assert cr.candidates(np.zeros((0, 3), dtype=np.int16)).shape == (0, 3)


def test_a_coarse_voxel_outside_the_fine_grid_never_contributes():
    """D outside [-16384, 16383]: its centre 2D is outside the int16 voxel range, and is never wrapped onto a block"""
    ends = [(-4096, 0, 0), (4095, 0, 0), (4095, 4095, 4095), (-4096, -4096, -4096)]
    pos, t, c, p = craft(ends, seed=13)
    c["weight"][:] = np.maximum(c["weight"], 2)
    src = (pos, np.where(t == F(-1), F(-0.5), t), c, p)
    offered = [(-2048, 0, 0), (2047, 0, 0), (2047, 2047, 2047), (-2048, -2048, -2048),   # D inside
               (2048, 0, 0), (-2049, 0, 0), (4095, 4095, 4095), (-2049, -2049, -2049), (2048, 2048, 2048)]
    (_, ct, cc, cp), cnt = cr.coarsen_blocks(src, offered)
    # inside: per axis the centres of local 0 .. 3 (block 0 or -4096) / 4 .. 7 (block 4095) fall into the allocated block
    assert cnt[:4].tolist() == [64, 64, 64, 64]
    assert not cnt[4:].any() and not cr.records((None, ct[4:], cc[4:], cp[4:])).any()
    taps = cr.present_taps(src, offered[:2])
    x, low = np.arange(512) & 7, (((np.arange(512) >> 3) & 7) < 4) & ((np.arange(512) >> 6) < 4)
    # coarse x = -16384: the tap at fine x = -32769 is absent, its centre -32768 present
    assert not taps[0][x == 0][:, 0::3].any() and taps[0][(x == 0) & low][:, 13].all()
    # coarse x = 16383: centre 32766, the tap at 32767 present
    assert taps[1][(x == 7) & low][:, 13].all() and taps[1][(x == 7) & low][:, 14].all()
