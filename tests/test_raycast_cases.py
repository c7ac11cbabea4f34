"""The crafted ray-cast cases (tests/raycast_cases.py) on the CPU oracle alone, no GPU: the builders' self-checks, the
conditions that keep the GPU test from being vacuous, and the closed-form shading of the oracle's own renderings."""
import re
from pathlib import Path

import numpy as np
import pytest

import raycast_cases as rc

ROOT = Path(__file__).resolve().parent.parent


def _oracle_with(make_oracle, m, **kw):
    e = make_oracle(rc.VS, rc.TRUNC, threads=4, **kw)
    e.import_blocks(*m)
    return e


def _render(e, v):
    return e.raycast(v.K, v.H, v.W, v.pose, v.max_depth)


def test_hashes_restate_the_kernel_header():
    """the constants of occ_bit / occ_bit2 / cell_bit and the filter's sizes, read from kernels_raycast.h"""
    src = (ROOT / "ra-slam_amd" / "csrc" / "kernels_raycast.h").read_text()

    def body(name):
        return src[src.index(f"inline uint32_t {name}("):].split("}\n", 1)[0]

    def consts(name):
        return [int(c, 16) for c in re.findall(r"__umul24\([xyz], 0x([0-9A-Fa-f]+)u\)", body(name))]

    assert consts("occ_bit") == [0x9E5, 0x1F35B, 0x6A7C1] and ">>" not in body("occ_bit").split("return", 1)[1]
    assert consts("occ_bit2") == [0x2C1B3, 0x5D3, 0x1B873] and ">> 3) & (kOccWords" in body("occ_bit2")
    assert consts("cell_bit") == [0x9E5, 0x1F35B, 0x6A7C1] and "& (kCellWords" in body("cell_bit")
    assert int(re.search(r"kOccWords = (\d+);", src).group(1)) * 32 == rc.OCC_BITS
    assert int(re.search(r"kCellWords = (\d+);", src).group(1)) * 32 == rc.CELL_BITS
    assert int(re.search(r"#define RATSDF_CELL_BITS (\d+)", src).group(1)) - 3 == rc.CELL_BLOCK_SHIFT
    # known answers, by hand: negative coordinates enter as their low 16 bits
    assert int(rc.occ_bit(np.array([1, 0, 0]))) == 0x9E5 and int(rc.occ_bit(np.array([0, 0, 1]))) == 0x6A7C1 & 0x1FFFF
    assert int(rc.occ_bit(np.array([-1, 0, 0]))) == (0xFFFF * 0x9E5) & 0x1FFFF
    assert int(rc.occ_bit2(np.array([0, 0, -1]))) == (((0xFFFF * 0x1B873) & 0xFFFFFFFF) >> 3) & 0x1FFFF
    assert int(rc.cell_bit(np.array([-1, -1, -1]))) == (0xFFFF * (0x9E5 + 0x1F35B + 0x6A7C1)) & 0x7FFF


def test_plane_patch_is_what_it_says():
    m = rc.patch(rc.ORIGIN)
    assert m.pos.dtype == np.int16 and m.tsdf.dtype == np.float32 and m.prob.dtype == np.float32
    assert m.tsdf.shape == m.rgbw.shape == m.prob.shape == (len(m), 512)
    assert len(np.unique(rc.block_keys(m.pos))) == len(m)
    assert m.pos.min() == -6 and m.pos.max() == 5
    # all eight sign combinations of the block coordinates, and of the super-cell coordinates
    for coords in (m.pos.astype(int), rc.cells_of(m.pos)):
        assert len({tuple(s) for s in (coords < 0)}) == 8
    # a voxel by hand: block (-1, 2, 0), local (7, 0, 3) = voxel (-1, 16, 3), slot 7 + 0 + 3 * 64
    row = int(np.flatnonzero((m.pos == (-1, 2, 0)).all(axis=1))[0])
    n = np.array(rc.PLANE_NORMAL) / np.linalg.norm(rc.PLANE_NORMAL)
    d = float((np.array([-1, 16, 3]) - 3.5) @ n)
    assert abs(d) < 6
    assert m.tsdf[row, 199] == np.float32(d * rc.VS / rc.TRUNC) and m.rgbw["weight"][row, 199] == 40
    assert tuple(m.rgbw[row, 199])[:3] == ((37 * -1) & 255, (59 * 16) & 255, (83 * 3) & 255)
    assert m.prob[row, 199] == np.float32(0.3 + 0.5 * 15 / 15)
    # clipped and unweighted beyond the truncation; probabilities on both sides of 0.5
    far = np.abs((rc.block_voxels(m.pos) - 3.5) @ n) > 6
    assert far.any() and (np.abs(m.tsdf[far]) == 1).all() and (m.rgbw["weight"][far] == 0).all()
    assert (m.rgbw["weight"][~far] == 40).all() and (m.prob < 0.5).any() and (m.prob > 0.5).any()
    # every block that holds a voxel within the truncation (+ 1 for the normal's neighbours) of the plane is kept
    cube = rc._cube((-6,) * 3, (6,) * 3)
    near = (np.abs((rc.block_voxels(cube) - 3.5) @ n) <= 7).any(axis=1)
    assert np.isin(rc.block_keys(cube[near]), rc.block_keys(m.pos)).all()


def test_maps_are_small_and_reach_the_ends_of_the_voxel_range():
    seen = {}
    for v in rc.views():
        seen[id(v.build())] = v.build()
    for m in seen.values():
        assert 100 <= len(m) <= 1500
    hi, lo = rc.patch(rc.EDGE_HI), rc.patch(rc.EDGE_LO)
    assert hi.pos[:, 0].max() == 4095 and rc.block_voxels(hi.pos)[..., 0].max() == 32767
    assert lo.pos[:, 0].min() == -4096 and rc.block_voxels(lo.pos)[..., 0].min() == -32768
    neg = rc.patch(rc.NEGATIVE)
    assert (neg.pos < 0).all()
    s = rc.sphere()
    d = np.linalg.norm(rc.block_voxels(s.pos) - np.array(rc.SPHERE_CENTRE), axis=2) - rc.SPHERE_RADIUS
    assert np.array_equal(s.tsdf, np.clip(d / 6, -1, 1).astype(np.float32))


def test_filter_decoys_cover_their_targets():
    v, plain = rc.collisions_view(), rc.octants_view()
    m, base = v.build(), plain.build()
    decoys = m.take(np.arange(len(base), len(m)))
    targets = rc.march(base, plain, full_step_only=True)["absent"]
    assert len(targets) >= 30 and len(np.unique(rc.cells_of(targets), axis=0)) >= 5
    assert not np.isin(rc.block_keys(targets), rc.block_keys(base.pos)).any()
    # (filter_decoys asserts the same before it returns)
    assert np.isin(rc.occ_bit(targets), rc.occ_bit(decoys.pos)).all()
    assert np.isin(rc.occ_bit2(targets), rc.occ_bit2(decoys.pos)).all()
    assert np.isin(rc.cell_bit(rc.cells_of(targets)), rc.cell_bit(rc.cells_of(decoys.pos))).all()
    # without the decoys the map alone would leave most targets provably absent: the case is not already covered
    own = np.isin(rc.occ_bit(targets), rc.occ_bit(base.pos)) & np.isin(rc.occ_bit2(targets), rc.occ_bit2(base.pos))
    assert own.mean() < 0.2
    # the decoys are nowhere near a view, and render nothing
    assert decoys.pos.min() >= 1000 and (decoys.rgbw["weight"] == 0).all() and (decoys.tsdf == 1).all()


def test_collisions_render_like_octants(make_oracle):
    v, plain = rc.collisions_view(), rc.octants_view()
    with_decoys, without = _render(_oracle_with(make_oracle, v.build()), v), _render(_oracle_with(make_oracle, plain.build()), plain)
    assert np.array_equal(with_decoys[0], without[0]) and np.array_equal(with_decoys[1], without[1])


@pytest.mark.parametrize("v", rc.views(), ids=lambda v: v.name)
def test_oracle_view_is_not_vacuous(v, make_oracle):
    m = v.build()
    e = _oracle_with(make_oracle, m)
    rgba, normal = _render(e, v)
    share = rc.assert_hit_share(v, rgba)
    hit = rgba[..., 3] == 255
    assert not rgba[~hit].any() and not normal[~hit].any()
    if hit.sum() >= 100:
        assert len(np.unique(rgba[hit][:, :3], axis=0)) > 10   # the colour varies from voxel to voxel
    if v.surface is not None and v.name in rc.SHADING_ORACLE:
        rc.assert_shading(m, v, normal, rgba)
        alpha = (normal[..., 0].astype(int) - normal[..., 1])[hit]
        assert (alpha == 0).any() and (alpha > 0).any()          # both branches of alpha
    # the numpy march (what the cases were designed with) sees the same pixels hit
    assert (rc.march(m, v)["hit"] == hit).mean() > 0.999
    # any row range is that part of the rendering
    for r0, r1 in rc.row_ranges(v.H):
        ra, rn = e.raycast_rows(v.K, v.H, v.W, v.pose, v.max_depth, r0, r1)
        assert np.array_equal(ra, rgba[r0:r1]) and np.array_equal(rn, normal[r0:r1]), (r0, r1)


def test_short_views_stop_one_sample_before_the_first_crossing(make_oracle):
    last = rc.short_views()[-1]
    e = _oracle_with(make_oracle, last.build())
    assert rc.hit_share(_render(e, last)[0]) == 0
    one_more = last._replace(max_depth=last.max_depth + rc.TRUNC / 2)
    assert rc.hit_share(_render(e, one_more)[0]) > 0


def test_far_views_start_beyond_the_short_rounding_form():
    far = rc.far_views()
    assert [v.name for v in far] == ["far_0", "far_1", "far_2", "far_mixed"]
    starts = [np.float32(-v.pose[4]) / np.float32(rc.VS) for v in far]
    assert starts[0] == 2.0 ** 30 and starts[1] == 2.0 ** 30 + 3 * 65536 and starts[2] >= 2.0 ** 31
    assert [rc.wrapped_voxel(s) for s in starts] == [0, 0, -1, -13888]
    for s in starts[:3]:
        assert s >= 1e9 and np.float32(s) + np.float32(3.0) == s   # `small` is false for every wave; the step is absorbed
    # far_mixed: the image's first 16x4-pixel wave has lanes on either side of the threshold
    lanes = rc.far_mixed_lanes(far[3])
    assert 0 < lanes[:4, :16].sum() < 64 and starts[3] == 999999936.0
