"""The crafted marching-cubes cases (tests/mesh_cases.py) on the CPU oracle alone, no GPU: the oracle's mesh equals the
numpy reference's on every builder, triangle for triangle and vertex for vertex, and the properties that
tests/test_gpu_mesh.py asserts of the engine's output hold of the oracle's (the same helper functions)."""
import re
from pathlib import Path

import numpy as np
import pytest

import mesh_cases as mc

ROOT = Path(__file__).resolve().parent.parent


def _oracle_with(make_oracle, m):
    e = make_oracle(mc.VS, mc.TRUNC, threads=4)
    e.import_blocks(*m)
    return e


def test_constants_restate_the_kernel_header():
    src = (ROOT / "ra-slam_amd" / "csrc" / "kernels_mesh.h").read_text()
    assert int(re.search(r"kVertVolume = (\d+);", src).group(1)) * 3 == mc.VERTS_PER_BLOCK
    assert int(re.search(r"kScanTile = (\d+);", src).group(1)) == mc.SCAN_TILE
    assert "base < ntiles; base += 1024" in src and mc.SCAN_PASS == 1024
    assert re.search(r">> 24\) > (\d+)\)", src).group(1) == str(mc.MIN_WEIGHT)


def test_reference_by_hand():
    """one block, one negative voxel: the eight cubes round it each cut a corner; the vertices by hand"""
    pos = np.array([[2, -3, 1]], np.int16)
    tsdf = np.full((1, 512), 0.5, np.float32)
    tsdf[0, 3 + 4 * 8 + 5 * 64] = -0.25
    v = mc.block_voxels(pos)
    m = mc.BlockSet(pos, tsdf, mc._colour(v, 11), mc._probability(v))
    vert, tri, p, info = mc.mesh_ref(m)
    assert len(tri) == 8 and len(vert) == 6 and mc.unreferenced(vert, tri) == 0
    at = np.array([16 + 3, -24 + 4, 8 + 5], dtype=np.float64)
    want = sorted(tuple(np.float32(np.float32(at[k] + s * (1 / 3 if k == d else 0)) * np.float32(mc.VS)) for k in range(3))
                  for d in range(3) for s in (1, -1))
    got = sorted(tuple(r) for r in vert)
    assert np.allclose(got, want, rtol=0, atol=1e-6)
    assert info["interior"].sum() == 343 and info["interior"][0] == 343 - 8
    assert sorted(np.flatnonzero(info["interior"])[1:].tolist()) == [1, 2, 4, 8, 16, 32, 64, 128]
    # at weight 10 the same block is unobserved: no mesh
    assert len(mc.mesh_ref(mc.replaced(m, rgbw=mc._colour(v, 10)))[1]) == 0


def test_noise_blocks_cover_what_they_promise():
    m = mc.noise_blocks()            # (asserts the coverage and prints the counts)
    assert len(m) == 4 * 3 * 3 - 1 and (m.pos < 0).all()
    off = np.array(mc.NOISE_OFFSET)
    assert not (m.pos == off + mc.NOISE_ABSENT).all(axis=1).any()
    under = m.rgbw["weight"][(m.pos == off + mc.NOISE_UNDERWEIGHT).all(axis=1)]
    assert under.shape == (1, 512) and (under == 10).all()
    assert (m.tsdf == 0).sum() >= 4 and np.signbit(m.tsdf[m.tsdf == 0]).sum() >= 2
    assert np.float64(np.float32(1e-3)) > 1e-3 > np.float64(np.nextafter(np.float32(1e-3), np.float32(0)))
    one = np.float32(1)
    assert one - np.nextafter(-one, np.float32(0)) == 2 and one - (-one + np.float32(2.0 ** -23)) < 2


@pytest.mark.parametrize("name", mc.CASES)
def test_oracle_matches_the_reference(name, make_oracle):
    m = mc.cases()[name]
    got = _oracle_with(make_oracle, m).gather_valid_mesh()
    want = mc.reference(name)
    print(f"mesh {name}: {len(m)} blocks")
    mc.assert_same_mesh(got, want, name)
    if name in ("empty",):
        assert len(got[0]) == 0 and len(got[1]) == 0
    else:
        assert len(got[1]) > 0
    if name == "noise":
        assert mc.unreferenced(got[0], got[1]) == mc.unreferenced(want[0], want[1]) > 0
    if name in ("noise", "sphere", "single_block"):
        between, on = mc.assert_vertex_probabilities(m, got[0], got[2])
        print(f"mesh {name}: {between} vertices between two voxels, {on} on a voxel")
        assert between > 0 and (on > 0 or name != "noise")


def test_oracle_matches_the_reference_on_the_big_map(make_oracle):
    """three passes of either scan (the counts' tile numbers are asserted by big_map()), at each of the three counts:
    the one-item last tile, the exactly full one and the generic one"""
    maps = mc.big_maps()
    assert [len(m) for m in maps] == list(mc.BIG_COUNTS) and len(mc.big_map()) == mc.BIG_COUNTS[-1] >= 3900
    for small, large in zip(maps, maps[1:]):
        assert np.array_equal(large.pos[:len(small)], small.pos)
    e, done = make_oracle(mc.VS, mc.TRUNC, threads=4), 0
    for m in maps:
        e.import_blocks(*m.take(np.arange(done, len(m))))
        done = len(m)
        mc.assert_same_mesh(e.gather_valid_mesh(), mc.reference(("big", len(m))), f"big {len(m)}")


def test_sphere_is_closed_and_on_the_sphere(make_oracle):
    m = mc.sphere_mesh_map()
    v, tri, p, info = mc.reference("sphere")
    assert info["cull_small"] == 0 and info["cull_large_observed"] == 0
    for mesh in ((v, tri, p), _oracle_with(make_oracle, m).gather_valid_mesh()):
        mc.assert_closed_sphere(mesh[0], mesh[1], mc.SPHERE_CENTRE, mc.SPHERE_RADIUS)
        mc.assert_on_sphere(mesh[0], mc.SPHERE_CENTRE, mc.SPHERE_RADIUS)


def test_edge_maps_reach_the_ends_of_the_range():
    maps = mc.edge_maps()
    hi, lo = mc.reference("edge_hi"), mc.reference("edge_lo")
    assert hi[0][:, 0].max() > np.float32(32766 * mc.VS) and lo[0][:, 0].min() == np.float32(-32768 * mc.VS)
    # the last block's lattice points at x = 32768 would come out at -32768: their cubes reach into an absent block
    # (4096) and every one of their triangles is dropped; nothing of the high end lies at negative x
    # (so edge_hi does not show the int16 wrap of the vertex base in any exported vertex; edge_wrap does)
    assert hi[0][:, 0].min() > 0 and hi[3]["dropped_at"].sum() > 0
    v = mc.reference("edge_wrap")[0]
    m = maps["edge_wrap"]
    beyond = (mc.block_voxels(m.pos)[..., 0] >= 32768) & (np.abs(m.tsdf) < 1)
    assert beyond.any()
    # block 4095 ends at x = 32767 voxels, block 4096 begins at -32768: nothing is exported beyond 32768 - 1, the far
    # side of the plane comes out at the low end of the range, and the vertices on the edges from 32767 to 32768, whose
    # base is not wrapped, lie in between
    x = v[:, 0].astype(np.float64) / mc.VS
    assert x.max() < 32768 and -32768 <= x.min() < -32767 and ((x > 32767) & (x < 32768)).any()
    assert (x < -32768 + 16.5).sum() > 100 and (x > 32768 - 16.5).sum() > 100 and not (np.abs(x) < 32768 - 16.5).any()


def test_edited_maps_split_the_sphere():
    base, more = mc.edited_maps()
    assert len(more) == mc.EDIT_EXTRA and len(base) + len(more) == len(mc.sphere_mesh_map())
    v, tri, p, _ = mc.mesh_ref(base)
    own = mc.owners(v, tri)
    assert np.isin(mc.block_keys(own), mc.block_keys(base.pos)).all()
    gone = base.take(np.arange(0, len(base), 3))
    assert np.isin(mc.block_keys(gone.pos), mc.block_keys(own)).mean() > 0.3   # the deleted blocks do hold triangles
