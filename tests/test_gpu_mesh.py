"""k_marching_cubes, the three-launch scans and the compaction (ra-slam_amd/csrc/kernels_mesh.h, query.inc) on the
crafted maps of tests/mesh_cases.py, against the CPU oracle and the numpy reference: every sign pattern inside blocks and
across their faces, absent and under-weight neighbours, both cull thresholds, zeros, the ends of the voxel range, scans
of three passes with a full and a one-item last tile, maps read back from a file and maps edited in place.

The maps are imported, not integrated: both sides hold the same floats, every vertex operation is one correctly rounded
float32 operation and the only contraction candidate multiplies by 0 or 1, so every case asserts EQUAL triangle rows and
EQUAL exported vertices.  Equality holds on the MI355X in every case: no operation of the export differs from the
oracle's or the reference's.
"""
import numpy as np
import pytest

import mesh_cases as mc

pytestmark = pytest.mark.gpu


def _pair(make_engine, make_oracle, m):
    gpu, cpu = make_engine(mc.VS, mc.TRUNC), make_oracle(mc.VS, mc.TRUNC, threads=8)
    for e in (gpu, cpu):
        if len(m):
            e.import_blocks(*m)
    return gpu, cpu


def _positions(e):
    b = e.dump_directory()[1]
    return np.stack([b["x"], b["y"], b["z"]], axis=1)


def _compare(gpu, cpu, what, want=None):
    """the engine's mesh against the oracle's (and the reference's); the buffers themselves where both directories list
    the blocks in the same order.  Returns the engine's mesh."""
    got, ref = gpu.gather_valid_mesh(), cpu.gather_valid_mesh()
    print(f"mesh {what}: {gpu.num_active_blocks()} blocks")
    assert gpu.num_active_blocks() == cpu.num_active_blocks()
    mc.assert_same_mesh(got, ref, f"{what}: engine against oracle")
    if want is not None:
        mc.assert_same_mesh(got, want, f"{what}: engine against reference")
    same_order = np.array_equal(_positions(gpu), _positions(cpu))
    print(f"mesh {what}: the directories list the blocks in {'the same' if same_order else 'another'} order")
    if same_order:
        assert np.array_equal(got[1], ref[1]), f"{what}: triangle index buffers differ"
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]), f"{what}: vertex buffers differ"
    return got


def _same_arrays(a, b, what):
    assert all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b)), what


@pytest.mark.parametrize("name", mc.CASES)
def test_cases(name, make_engine, make_oracle):
    """noise, sphere, single_block, empty, edge_hi, edge_lo, edge_wrap; a second call returns the same arrays (the scratch is
    allocated per call: no vmask of the first may show)"""
    m = mc.cases()[name]
    gpu, cpu = _pair(make_engine, make_oracle, m)
    got = _compare(gpu, cpu, name, mc.reference(name))
    _same_arrays(gpu.gather_valid_mesh(), got, f"{name}: a second call differs")
    if name == "empty":
        assert len(got[0]) == 0 and len(got[1]) == 0 and len(got[2]) == 0
        return
    assert len(got[1]) > 0
    if name == "noise":
        want = mc.reference(name)
        assert mc.unreferenced(got[0], got[1]) == mc.unreferenced(want[0], want[1]) > 0
    if name in ("noise", "sphere", "single_block"):
        mc.assert_vertex_probabilities(m, got[0], got[2])
    if name == "sphere":
        mc.assert_closed_sphere(got[0], got[1], mc.SPHERE_CENTRE, mc.SPHERE_RADIUS)
        mc.assert_on_sphere(got[0], mc.SPHERE_CENTRE, mc.SPHERE_RADIUS)


def test_scan(make_engine, make_oracle):
    """3875, 3912 and 4101 blocks on one pair, the map growing: three passes of k_scan_tile_sums for vertices and
    triangles alike, a last vertex tile of one item, a last triangle tile exactly full, and a generic count"""
    gpu, cpu = _pair(make_engine, make_oracle, mc.empty())
    done = 0
    for m in mc.big_maps():
        more = m.take(np.arange(done, len(m)))
        for e in (gpu, cpu):
            e.import_blocks(*more)
        done = len(m)
        assert gpu.num_active_blocks() == len(m)
        v, tri, p = _compare(gpu, cpu, f"scan {len(m)}", mc.reference(("big", len(m))))
        print(f"mesh scan {len(m)}: scan tiles (vertices, triangles) {mc.scan_tiles(len(m))}")
        assert tri.min() >= 0 and tri.max() < len(v) and len(p) == len(v)
        assert len(np.unique(tri.reshape(-1))) == len(v)          # (a shell: every exported vertex is referenced)


def test_mapfile(make_engine, tmp_path):
    """load_map rebuilds the free list through mask_positions, at three passes here: the loaded map meshes alike, holds
    as many blocks, and still takes new ones"""
    m = mc.big_map()
    a = make_engine(mc.VS, mc.TRUNC)
    a.import_blocks(*m)
    mine = a.gather_valid_mesh()
    mc.assert_same_mesh(mine, mc.reference(("big", len(m))), "mapfile: before saving")
    a.save_map(tmp_path / "big.map")
    b = make_engine(mc.VS, mc.TRUNC)
    b.load_map(tmp_path / "big.map")
    assert b.num_active_blocks() == a.num_active_blocks() == len(m)
    mc.assert_same_mesh(b.gather_valid_mesh(), mine, "mapfile: loaded")
    # the rebuilt free list hands out blocks that ARE free: another map, far from this one, is added and the mesh is the
    # two meshes side by side
    far = mc.edge_maps()["edge_lo"]
    b.import_blocks(*far)
    assert b.num_active_blocks() == len(m) + len(far)
    both = [mc.reference(("big", len(m))), mc.reference("edge_lo")]
    v, tri, p = b.gather_valid_mesh()
    rows = np.concatenate([mc.tri_rows(*r[:3]) for r in both])
    assert np.array_equal(mc.tri_rows(v, tri, p), rows[np.lexsort(rows.T[::-1])]), "mapfile: loaded, then grown"
    assert np.array_equal(mc.vertex_rows(v, p), mc.vertex_rows(np.concatenate([r[0] for r in both]),
                                                               np.concatenate([r[2] for r in both])))


def test_edited(make_engine, make_oracle):
    """every third block deleted, imported back in reverse order (pool slots are reused in another order), then 50 more
    blocks: equal to the oracle after each step, and the deleted blocks' triangles gone.  Which blocks a delete pass
    takes out is not fixed by the recipe (see below), so the set that survives is read from the oracle's directory, the
    engine must hold as many, and the expected mesh after the deletes is mesh_ref of that set; after the re-import the
    expectation is the recipe's own again (the mesh as first imported, then the whole sphere)."""
    base, more = mc.edited_maps()
    gpu, cpu = _pair(make_engine, make_oracle, base)
    before = _compare(gpu, cpu, "edited: as imported", mc.mesh_ref(base))
    gone = base.take(np.arange(0, len(base), 3))
    for e in (gpu, cpu):
        e.test_delete(gone.pos)
    # (one call is one carve pass: a delete that finds its bucket locked by another of the pass is dropped, in both
    # implementations alike)
    assert gpu.num_active_blocks() == cpu.num_active_blocks() <= len(base) - 0.9 * len(gone)
    held = mc.present(base, cpu.dump_directory()[1])
    assert len(held) == cpu.num_active_blocks()
    after = _compare(gpu, cpu, "edited: after the deletes", mc.mesh_ref(held))
    deleted = mc.block_keys(base.pos)[~np.isin(mc.block_keys(base.pos), mc.block_keys(held.pos))]
    assert np.isin(mc.block_keys(mc.owners(before[0], before[1])), deleted).any()
    assert not np.isin(mc.block_keys(mc.owners(after[0], after[1])), deleted).any()
    assert len(after[1]) < len(before[1])
    back = gone.take(np.arange(len(gone))[::-1])
    for e in (gpu, cpu):
        e.import_blocks(*back)
    again = _compare(gpu, cpu, "edited: after the re-import")
    mc.assert_same_mesh(again, before, "edited: the re-import did not restore the mesh")
    for e in (gpu, cpu):
        e.import_blocks(*more)
    assert gpu.num_active_blocks() == len(base) + len(more)
    whole = _compare(gpu, cpu, "edited: with 50 more blocks", mc.reference("sphere"))
    mc.assert_closed_sphere(whole[0], whole[1], mc.SPHERE_CENTRE, mc.SPHERE_RADIUS)


def test_download_all_mesh(make_engine, tmp_path):
    """the three files hold what gather_valid_mesh returns"""
    gpu = make_engine(mc.VS, mc.TRUNC)
    gpu.import_blocks(*mc.noise_blocks())
    v, tri, p = gpu.gather_valid_mesh()
    fv, fi, fp = tmp_path / "v.bin", tmp_path / "i.bin", tmp_path / "p.bin"
    gpu.download_all_mesh(fv, fi, fp)
    assert len(tri) > 0
    assert np.array_equal(np.fromfile(fv, "<f4").reshape(-1, 3), v)
    assert np.array_equal(np.fromfile(fi, "<i4").reshape(-1, 3), tri)
    assert np.array_equal(np.fromfile(fp, "<f4"), p)
