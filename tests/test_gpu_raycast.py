"""k_raycast / k_occupancy_build on crafted maps (tests/raycast_cases.py) against the CPU oracle: block coordinates of
every sign and at the ends of the voxel range, image sizes that are no multiple of the workgroup's tile, filter bits set
by other blocks, maps written by every path that maintains Table::active, chained directories, the long rounding form,
crossings at the map's rim -- and the shading against geometry known in closed form.

The maps are imported, not integrated: both sides hold the same voxels bit for bit, probabilities included, so the
crafted cases assert EQUAL images (the first run on an MI355X showed 0 differing bytes in every one of them).  Only the
last step of `edited`, which integrates frames, keeps the bar of test_raycast_matches_oracle.
"""
import numpy as np
import pytest

import raycast_cases as rc

pytestmark = pytest.mark.gpu

EXACT = True   # (set after the first run showed 0 differing bytes everywhere, the step with frames included)


def _pair(make_engine, make_oracle, m, **kw):
    gpu, cpu = make_engine(rc.VS, rc.TRUNC, **kw), make_oracle(rc.VS, rc.TRUNC, threads=8, **kw)
    for e in (gpu, cpu):
        e.import_blocks(*m)
    return gpu, cpu


def _render(e, v):
    return e.raycast(v.K, v.H, v.W, v.pose, v.max_depth)


def _compare(gpu, cpu, v, what=None, exact=EXACT):
    """renders the view on both; the engine's images against the oracle's.  Returns (engine's, oracle's)."""
    got, want = _render(gpu, v), _render(cpu, v)
    rc.assert_matches_oracle(got, want, what or v.name, exact=exact)
    return got, want


def _same_images(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what


@pytest.mark.parametrize("v", rc.plane_views() + rc.sphere_views(), ids=lambda v: v.name)
def test_surfaces(v, make_engine, make_oracle):
    """octants, negative, edge_hi, edge_lo, rim, sphere (from outside and from inside the shell)"""
    m = v.build()
    gpu, cpu = _pair(make_engine, make_oracle, m)
    got, want = _compare(gpu, cpu, v)
    rc.assert_hit_share(v, want[0])
    rc.assert_shading(m, v, got[1], got[0])


@pytest.mark.parametrize("v", rc.size_views(), ids=lambda v: v.name)
def test_sizes(v, make_engine, make_oracle):
    """the x >= W guard, a partial last workgroup row, row ranges, device output, null outputs"""
    import torch
    gpu, cpu = _pair(make_engine, make_oracle, v.build())
    got, want = _compare(gpu, cpu, v)
    assert rc.hit_share(want[0]) > 0.8
    for r0, r1 in rc.row_ranges(v.H):
        ra, rn = gpu.raycast_rows(v.K, v.H, v.W, v.pose, v.max_depth, r0, r1)
        assert ra.shape == (r1 - r0, v.W, 4)
        _same_images((ra, rn), (got[0][r0:r1], got[1][r0:r1]), (r0, r1))
    for with_rgba, with_normal in ((True, True), (True, False), (False, True), (False, False)):
        d_a = torch.full((v.H, v.W, 4), 7, dtype=torch.uint8, device="cuda")
        d_n = torch.full((v.H, v.W, 4), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        gpu.raycast_device(v.K, v.H, v.W, v.pose, v.max_depth, d_a.data_ptr() if with_rgba else 0,
                           d_n.data_ptr() if with_normal else 0)
        gpu.synchronize()
        for d, used, full in ((d_a, with_rgba, got[0]), (d_n, with_normal, got[1])):
            assert np.array_equal(d.cpu().numpy(), full if used else np.full_like(full, 7)), (with_rgba, with_normal)


def test_short(make_engine, make_oracle):
    """max_step 1, 2 and one sample short of the first crossing: nothing is rendered"""
    views = rc.short_views()
    gpu, cpu = _pair(make_engine, make_oracle, views[0].build())
    for v in views:
        got, want = _compare(gpu, cpu, v)
        assert rc.hit_share(want[0]) == 0 and not got[0].any() and not got[1].any()


def test_collisions(make_engine, make_oracle):
    """every empty sample between the camera and the surface finds its cell bit and both block bits set by OTHER
    blocks, and has to find the block absent in the directory"""
    v, plain = rc.collisions_view(), rc.octants_view()
    gpu, cpu = _pair(make_engine, make_oracle, v.build())
    got, want = _compare(gpu, cpu, v)
    rc.assert_hit_share(v, want[0])
    rc.assert_shading(v.build(), v, got[1], got[0])
    _, cpu_plain = _pair(make_engine, make_oracle, plain.build())
    _same_images(want, _render(cpu_plain, plain), "the oracle's image changed with the decoys")


@pytest.mark.parametrize("v", rc.far_views(), ids=lambda v: v.name)
def test_far(v, make_engine, make_oracle):
    """ray origins beyond 1e9 voxels: the long form of (short)roundf, for whole waves and for a wave that mixes lanes
    on either side of the threshold"""
    gpu, cpu = _pair(make_engine, make_oracle, v.build())
    got, want = _compare(gpu, cpu, v)
    assert rc.hit_share(want[0]) == 1.0
    if v.name == "far_mixed":
        assert 0 < rc.far_mixed_lanes(v)[:4, :16].sum() < 64


def _delete_and_reimport(gpu, cpu, m, views, what):
    """steps 1 and 2 of `edited`: every third block deleted in list order (they vanish from the picture), imported back
    in reverse order (pool slots are reused in another order), then 50 more blocks (free_low moves).  Returns the map."""
    before = {v.name: _render(cpu, v) for v in views}
    gone = m.take(np.arange(0, len(m), 3))
    for e in (gpu, cpu):
        e.test_delete(gone.pos)
    # (one call is one carve pass: a delete that finds its bucket locked by another of the pass is dropped, in both
    # implementations alike -- in the chained directory that happens)
    assert gpu.num_active_blocks() == cpu.num_active_blocks() <= len(m) - 0.9 * len(gone)
    for v in views:
        _, want = _compare(gpu, cpu, v, f"{what}: {v.name} after the deletes")
        assert not np.array_equal(want[0], before[v.name][0]), "the deletes did not change the oracle's image"
    back = gone.take(np.arange(len(gone))[::-1])
    more = rc.extension(m)
    for e in (gpu, cpu):
        e.import_blocks(*back)
        e.import_blocks(*more)
    assert gpu.num_active_blocks() == cpu.num_active_blocks() == len(m) + len(more)
    for v in views:
        _, want = _compare(gpu, cpu, v, f"{what}: {v.name} after the re-import")
        if v.name == "octants":   # (its frame lies inside the patch: the picture is the one before the deletes again)
            _same_images(want, before[v.name], "the re-import did not restore the oracle's image")
    return rc.concat(m, more)


def test_edited(make_engine, make_oracle, tmp_path):
    """Table::active / free_low / the occupancy bits after every path that writes a map"""
    import torch
    from ratsdf import multi, synthetic
    import fuse_ref
    views = [rc.octants_view(), rc.rim_view()]
    m = views[0].build()
    a, o = _pair(make_engine, make_oracle, m)
    for v in views:
        _compare(a, o, v, f"edited: {v.name} as imported")
    m = _delete_and_reimport(a, o, m, views, "edited")
    mine = {v.name: _render(a, v) for v in views}

    # 3. through a map file
    a.save_map(tmp_path / "a.map")
    b = make_engine(rc.VS, rc.TRUNC)
    b.load_map(tmp_path / "a.map")
    # 4. fused into an empty map
    c = make_engine(rc.VS, rc.TRUNC)
    c.fuse_map(a)
    # 5. through device records
    d = make_engine(rc.VS, rc.TRUNC)
    pos = [tuple(int(x) for x in p) for p in m.pos]
    multi.import_blocks_device(d, pos, multi.export_blocks_device(a, pos, len(pos), "cuda"))
    d.synchronize()
    torch.cuda.synchronize()
    for e, name in ((b, "loaded"), (d, "device records")):
        assert e.num_active_blocks() == len(m)
        for v in views:
            _same_images(_render(e, v), mine[v.name], f"edited: {name}: {v.name}")
    set_a, set_c = fuse_ref.by_position(fuse_ref.dump_set(a)), fuse_ref.by_position(fuse_ref.dump_set(c))
    assert np.array_equal(set_a[0], set_c[0])
    if all(np.array_equal(x, y) for x, y in zip(set_a[1:], set_c[1:])):
        for v in views:
            _same_images(_render(c, v), mine[v.name], f"edited: fused: {v.name}")
    else:
        # a fusion leaves the voxels that do not contribute (weight 0) as a fresh block has them: the expectation is
        # fuse_ref's, rendered by an oracle
        want_set, info = fuse_ref.fuse(fuse_ref.empty_set(), set_a)
        fuse_ref.assert_sets_match(set_c, want_set, colour_known=info["colour_known"], what="fused into an empty map")
        o_c = make_oracle(rc.VS, rc.TRUNC, threads=8)
        o_c.import_blocks(*set_c)
        for v in views:
            _compare(c, o_c, v, f"edited: fused: {v.name}")

    # 6. frames on top: they allocate, update and carve; from here on the probabilities are computed, not imported
    h = w = 0
    for i in range(2):
        f = synthetic.frame("wall", i, scale=0.25)
        h, w = f["depth"].shape
        for e in (a, o):
            e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
    assert a.num_active_blocks() == o.num_active_blocks() > len(m)
    for v in views:
        _compare(a, o, v, f"edited: {v.name} after two frames", exact=False)
    wall = rc.View("wall", None, f["intrinsics"], h, w, f["pose"], 8.0, (0.0, 1.0))
    _compare(a, o, wall, "edited: the frames' own view", exact=False)


def test_chains(make_engine, make_oracle):
    """512 buckets for 500 blocks: find_block's chain walk, over dead nodes after the deletes, inside the march"""
    from kat_cases import ref_hash
    views = [rc.octants_view(), rc.rim_view()]
    m = views[0].build()
    gpu, cpu = _pair(make_engine, make_oracle, m, bucket_bits=9)
    entries, blocks = gpu.dump_directory()
    home = np.array([ref_hash((b["x"], b["y"], b["z"]), 9) for b in blocks])
    # (505 blocks over 512 buckets of two entries each: about 80 overflow into chains)
    assert ((entries >> 1) != home).sum() >= 50, "hardly any block is chained"
    for v in views:
        _compare(gpu, cpu, v, f"chains: {v.name} as imported")
    _delete_and_reimport(gpu, cpu, m, views, "chains")
