"""The numpy restatement of the fusion contract (tests/fuse_ref.py) without a GPU: known answers worked out by hand,
and its algebra on two maps of the CPU oracle -- the pair of views tests/test_gpu_fuse.py fuses, with the conditions
that keep those tests from passing vacuously."""
import numpy as np
import pytest

import fuse_ref
from fuse_ref import F
from ratsdf._abi import RGBW_DTYPE


def _vox(rows):
    """rows of (tsdf, (r, g, b, weight), prob) -> the three arrays"""
    t = np.array([r[0] for r in rows], dtype=F)
    c = np.array([r[1] for r in rows], dtype=RGBW_DTYPE)
    p = np.array([r[2] for r in rows], dtype=F)
    return t, c, p


NEAR_FRESH = float(np.nextafter(F(-1), F(0)))

# (a, b, expected a, branch)  branch: 0 unchanged, 1 copied, 2 averaged
CASES = [
    # b is a fresh voxel / has no weight: a stays, colour included
    ((0.5, (10, 20, 30, 5), 0.7), (-1.0, (9, 9, 9, 1), 0.5), (0.5, (10, 20, 30, 5), 0.7), 0),
    ((0.5, (10, 20, 30, 5), 0.7), (0.3, (9, 9, 9, 0), 0.9), (0.5, (10, 20, 30, 5), 0.7), 0),
    # a is fresh / has no weight: all three words of b
    ((-1.0, (4, 5, 6, 1), 0.5), (0.25, (1, 2, 3, 7), 0.9), (0.25, (1, 2, 3, 7), 0.9), 1),
    ((0.75, (4, 5, 6, 0), 0.2), (0.25, (1, 2, 3, 7), 0.9), (0.25, (1, 2, 3, 7), 0.9), 1),
    # the plain average: (0.5*1 - 0.5*3) / 4, (10 + 150) / 4, (20 + 180) / 4, (30 + 210) / 4
    ((0.5, (10, 20, 30, 1), 0.5), (-0.5, (50, 60, 70, 3), 0.5), (-0.25, (40, 50, 60, 4), 0.5), 2),
    # the cap: 30 + 25 = 55 -> 40
    ((1.0, (100, 100, 100, 30), 0.5), (1.0, (100, 100, 100, 25), 0.5), (1.0, (100, 100, 100, 40), 0.5), 2),
    # roundf ties go away from zero: 1.5 -> 2, 2.5 -> 3 (not the even 2), 0.5 -> 1
    ((0.0, (1, 2, 0, 1), 0.5), (0.0, (2, 3, 1, 1), 0.5), (0.0, (2, 3, 1, 2), 0.5), 2),
    # tsdf -1 with weight 2 is not fresh; weight 1 with tsdf one ulp above -1 is not fresh
    ((-1.0, (0, 0, 0, 2), 0.5), (1.0, (0, 0, 0, 2), 0.5), (0.0, (0, 0, 0, 4), 0.5), 2),
    ((NEAR_FRESH, (0, 0, 0, 1), 0.5), (0.5, (0, 0, 0, 1), 0.5),
     (float((F(NEAR_FRESH) * F(1) + F(0.5) * F(1)) / F(2)), (0, 0, 0, 2), 0.5), 2),
    # probabilities: p = 0 / p = 1 win against 0.5; against each other NaN
    ((0.0, (0, 0, 0, 2), 0.0), (0.0, (0, 0, 0, 2), 0.5), (0.0, (0, 0, 0, 4), 0.0), 2),
    ((0.0, (0, 0, 0, 2), 1.0), (0.0, (0, 0, 0, 2), 0.5), (0.0, (0, 0, 0, 4), 1.0), 2),
    ((0.0, (0, 0, 0, 2), 0.0), (0.0, (0, 0, 0, 2), 1.0), (0.0, (0, 0, 0, 4), float("nan")), 2),
    # log-odds pooling: L = (1 * ln 4 + 3 * 0) / 4, p = 1 / (1 + 4^-0.25) = 0.5857864
    ((0.0, (0, 0, 0, 1), 0.8), (0.0, (0, 0, 0, 3), 0.5), (0.0, (0, 0, 0, 4), 0.5857864), 2),
]


def test_known_answers():
    at, ac, ap = _vox([c[0] for c in CASES])
    bt, bc, bp = _vox([c[1] for c in CASES])
    wt, wc, wp = _vox([c[2] for c in CASES])
    ot, oc, op, copied, averaged = fuse_ref.fuse_voxels(at, ac, ap, bt, bc, bp)
    branch = np.array([c[3] for c in CASES])
    assert np.array_equal(copied, branch == 1)
    assert np.array_equal(averaged, branch == 2)
    assert np.array_equal(ot.view(np.uint32), wt.view(np.uint32))
    assert np.array_equal(oc, wc)
    assert np.array_equal(np.isnan(op), np.isnan(wp))
    ok = ~np.isnan(wp)
    assert np.max(np.abs(op[ok] - wp[ok])) <= 2e-7
    unchanged = branch < 2
    assert np.array_equal(op[unchanged].view(np.uint32), wp[unchanged].view(np.uint32))
    assert ot.dtype == F and op.dtype == F


def test_block_level_bookkeeping():
    """new blocks start as fresh voxels, the shard filter skips whole blocks, the statistics add up"""
    rng = np.random.default_rng(5)

    def blocks(pos):
        n = len(pos)
        c = np.zeros((n, 512), dtype=RGBW_DTYPE)
        for ch in ("r", "g", "b"):
            c[ch] = rng.integers(0, 256, (n, 512))
        c["weight"] = rng.integers(0, 41, (n, 512))
        return (np.array(pos, dtype=np.int16), rng.uniform(-1, 1, (n, 512)).astype(F), c,
                rng.uniform(0.05, 0.95, (n, 512)).astype(F))

    dst = blocks([(0, 0, 0), (1, 0, 0)])
    src = blocks([(1, 0, 0), (2, 0, 0), (-5, 3, 1), (9, 9, 9)])
    out, info = fuse_ref.fuse(dst, src)
    assert [tuple(p) for p in out[0]] == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (-5, 3, 1), (9, 9, 9)]
    assert info["blocks_seen"] == 4 and info["blocks_allocated"] == 3 and info["blocks_skipped"] == 0
    assert np.array_equal(out[1][0], dst[1][0]) and np.array_equal(out[2][0], dst[2][0])  # untouched block
    live = fuse_ref.contributes(src[1][1], src[2][1])
    assert np.array_equal(out[1][2][live], src[1][1][live])  # a new block: copies where the source contributes ...
    assert np.all(out[1][2][~live] == -1) and np.all(out[2][2]["weight"][~live] == 1)  # ... fresh voxels elsewhere
    assert np.all(out[3][2][~live] == 0.5)
    assert np.array_equal(info["colour_known"][2], live) and info["colour_known"][:2].all()
    assert info["voxels_copied"] + info["voxels_averaged"] == int(
        sum(fuse_ref.contributes(src[1][i], src[2][i]).sum() for i in range(4)))
    # shard 1 of 2 with slabs of 4 blocks owns bx in [4, 8), [-4, 0), ... : of the source only (-5 >> 2 = -2: no) ...
    out1, info1 = fuse_ref.fuse(dst, src, shard=(1, 2, 2))
    owned = [(p[0] >> 2) % 2 == 1 for p in src[0].tolist()]
    assert info1["blocks_skipped"] == owned.count(False)
    assert info1["blocks_seen"] == info1["blocks_allocated"] + info1["blocks_skipped"] + (1 if owned[0] else 0)
    with pytest.raises(AssertionError):
        fuse_ref.fuse(dst, blocks([(3, 3, 3), (3, 3, 3)]))


@pytest.fixture(scope="module")
def oracle_pair(oracle_lib):
    from ratsdf._abi import Engine
    sets = []
    for ids in (fuse_ref.FRAMES_A, fuse_ref.FRAMES_B):
        e = Engine(oracle_lib, fuse_ref.VOXEL_SIZE, fuse_ref.TRUNCATION, block_bits=14, bucket_bits=16, threads=8)
        fuse_ref.integrate_frames([e], ids)
        sets.append(fuse_ref.dump_set(e))
        e.close()
    return sets


def pair_shares(A, B):
    """what the pair must offer so that a fusion test proves something (asserted here and in the GPU tests)"""
    shared = np.isin(fuse_ref.keys(B[0]), fuse_ref.keys(A[0]))
    a = fuse_ref.by_position(tuple(v[np.isin(fuse_ref.keys(A[0]), fuse_ref.keys(B[0]))] for v in A))
    b = fuse_ref.by_position(tuple(v[shared] for v in B))
    _, c, _, copied, averaged = fuse_ref.fuse_voxels(a[1], a[2], a[3], b[1], b[2], b[3])
    n = copied.size
    return dict(blocks_a=len(A[0]), blocks_b=len(B[0]), shared=float(shared.mean()),
                unchanged=float((~copied & ~averaged).sum() / n), copied=float(copied.sum() / n),
                averaged=float(averaged.sum() / n), at_cap=int((averaged & (c["weight"] == 40)).sum()))


def assert_pair_qualifies(A, B):
    s = pair_shares(A, B)
    print("fusion pair:", s)
    assert 0.25 <= s["shared"] <= 0.75, s
    assert min(s["unchanged"], s["copied"], s["averaged"]) >= 0.02, s
    assert s["at_cap"] >= 1000, s
    return s


def test_the_pair_of_views_qualifies(oracle_pair):
    assert_pair_qualifies(*oracle_pair)


def test_fusing_into_an_empty_set_is_a_copy(oracle_pair):
    _, B = oracle_pair
    out, info = fuse_ref.fuse(fuse_ref.empty_set(), B)
    assert np.array_equal(out[0], B[0])
    live = fuse_ref.contributes(B[1], B[2])
    # every voxel word of B, except that a voxel B never touched is a fresh voxel either way (colour undefined)
    assert np.array_equal(out[1].view(np.uint32), B[1].view(np.uint32))
    assert np.array_equal(out[2]["weight"], B[2]["weight"])
    assert np.array_equal(out[2][live], B[2][live])
    assert np.array_equal(out[3].view(np.uint32), B[3].view(np.uint32))
    assert np.array_equal(info["colour_known"], live)
    assert info["blocks_allocated"] == len(B[0]) and info["voxels_copied"] == int(live.sum())
    assert info["voxels_averaged"] == 0


def test_fusion_commutes(oracle_pair):
    A, B = oracle_pair
    ab, iab = fuse_ref.fuse(A, B)
    ba, iba = fuse_ref.fuse(B, A)
    x, y = fuse_ref.by_position(ab), fuse_ref.by_position(ba)
    assert np.array_equal(x[0], y[0])
    assert np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32))
    assert np.array_equal(x[2]["weight"], y[2]["weight"])
    assert np.array_equal(x[3].view(np.uint32), y[3].view(np.uint32))
    # colour: wherever either side contributes (elsewhere each keeps what its own map held)
    ka = iab["colour_known"][np.argsort(fuse_ref.keys(ab[0]), kind="stable")]
    kb = iba["colour_known"][np.argsort(fuse_ref.keys(ba[0]), kind="stable")]
    either = fuse_ref.contributes(x[1], x[2])
    assert np.array_equal(x[2][either], y[2][either])
    assert (ka | kb)[either].all()
    assert iab["voxels_averaged"] == iba["voxels_averaged"] > 0
