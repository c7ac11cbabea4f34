"""Map checkpoints of the HIP engine at their edges (include/ratsdf_map.h, ra-slam_amd/csrc/mapfile.inc).

a. A well-formed file whose directory is no hash table, or whose header names no configuration an engine can have,
   is refused by the host validation before anything is launched (the cases of tests/mapfile_cases.py; the rule is
   mapfile_ref.check_directory).  Such a file reaches load_map only after map_file_info -- host only -- has refused
   it: a cyclic directory is never put on a card.
b. Files from directories with long chains, a chain across the table's end and dead chain nodes still load.
c. k_map_pack / k_map_unpack and their double-buffered host loops at the chunk edges (2 records per workgroup, the
   grid cap of 2048 workgroups, the chunk of 2048 records, the event wait of the third chunk, a colour section that
   starts a chunk, no live block at all), against bytes the test wrote itself."""
import numpy as np
import pytest

import mapfile_cases as mc
import mapfile_ref as ref
from kat_cases import chain_positions
from parity import assert_maps_equal
from ratsdf import synthetic
from test_gpu_mapfile import _run, _same_snapshot, _snapshot
from test_gpu_resample import CFG, craft, engine

pytestmark = pytest.mark.gpu

VS = 0.02


def _refused(call, path):
    import ratsdf
    with pytest.raises(ratsdf.RatsdfError) as ei:
        call(path)
    return ei.value.status


# ---- a. refused loads ------------------------------------------------------------------------------------------
def test_files_with_a_wrong_directory_are_refused_and_leave_the_map_untouched(tmp_path, make_engine, make_oracle):
    import ratsdf
    kw = dict(block_bits=14, bucket_bits=10)
    frames = synthetic.stream("sphere", 6, scale=0.25, noise=True, holes=True)
    gpu, cpu = make_engine(VS, 6 * VS, **kw), make_oracle(VS, 6 * VS, threads=8, **kw)
    _run([gpu, cpu], frames[:4])
    good = tmp_path / "good.map"
    gpu.save_map(good)
    data = good.read_bytes()
    m = ref.parse(data)
    assert ref.check_directory(m) is None and len(mc.chained(m)) >= 4
    assert ratsdf.map_file_info(good)["n_blocks"] == gpu.num_active_blocks()
    cases = mc.defects(data)
    assert set(cases) == ({f.__name__ for f in mc.D2_DEFECTS + mc.D1_DEFECTS + mc.D3_DEFECTS}
                          | set(mc.HEADER_DEFECTS))
    before = _snapshot(gpu)
    for name, (blob, violation) in cases.items():
        assert ref.check_directory(ref.parse(blob)) == violation, name
        p = tmp_path / "bad.map"
        p.write_bytes(blob)
        assert _refused(ratsdf.map_file_info, p) == 1, name  # (host only; a failure here keeps the file off the card)
        assert _refused(gpu.load_map, p) == 1, name
        _same_snapshot(before, _snapshot(gpu))
    _run([gpu, cpu], frames[4:])
    assert_maps_equal(gpu, cpu)


def test_create_refuses_what_a_file_may_not_hold(make_engine):
    """rule H is the range of ratsdf_create_ex: an engine cannot save a header that a load would refuse"""
    import ratsdf
    for kw in (dict(voxel_size=float("inf")), dict(truncation=float("inf")), dict(voxel_size=float("nan")),
               dict(shard_slab_bits=ref.MAX_SHARD_SLAB_BITS + 1), dict(shard_rank=3, shard_count=3)):
        with pytest.raises(ratsdf.RatsdfError) as ei:
            make_engine(**{"voxel_size": VS, "truncation": 6 * VS, **CFG, **kw})
        assert ei.value.status == 1, kw


# ---- b. files from chained directories -------------------------------------------------------------------------
def _allocate(e, positions, passes):
    for _ in range(passes):  # one insertion per bucket per pass (voxel_hash.cu:67-104)
        e.test_allocate(positions)


def test_files_from_chained_directories_load(tmp_path, make_engine):
    """The engine's Delete unlinks a node as the reference's does (voxel_hash.cu:135-187), so test_delete leaves no
    dead chain node: the carved file holds shorter chains.  (A file with a block behind a dead node is refused, rule
    D3: one loaded here before that rule existed lost the blocks behind the node at the next allocation.)"""
    kw = dict(block_bits=14, bucket_bits=9)
    per_bucket, buckets = 8, ((1 << 9) - 1, 100, 7)  # two home entries and a chain of 6 nodes each
    positions = [p for b in buckets for p in chain_positions(b, per_bucket, bucket_bits=9)]
    a = make_engine(VS, 6 * VS, **kw)
    _allocate(a, positions, per_bucket)
    assert a.num_active_blocks() == len(positions)
    full = tmp_path / "full.map"
    a.save_map(full)
    m = ref.parse(full.read_bytes())
    chains = mc.chains(m)
    assert sorted(c[0] >> 1 for c in chains) == sorted(buckets) and all(len(c) == 1 + 6 for c in chains)
    assert mc.wrap_links(m) and ref.check_directory(m) is None
    deleted = []
    for k in (0, 3, -1):  # a head, a middle node, a tail; one deletion per bucket per pass
        a.test_delete([mc.position(m, c[k]) for c in chains])
        deleted += [mc.position(m, c[k]) for c in chains]
    assert a.num_active_blocks() == len(positions) - len(deleted)

    path = tmp_path / "carved.map"
    a.save_map(path)
    m = ref.parse(path.read_bytes())
    assert np.all(m["blocks"]["idx"] >= 0) and len(m["blocks"]) == len(positions) - len(deleted)
    assert sorted(len(c) for c in mc.chains(m)) == [1 + 3] * 3 and ref.check_directory(m) is None
    b = make_engine(VS, 6 * VS, **kw)
    b.load_map(path)
    _same_snapshot(_snapshot(a), _snapshot(b))
    # the deleted positions come back at the same places, from the same free list, on both
    for e in (a, b):
        _allocate(e, deleted, 3)
        assert e.num_active_blocks() == len(positions)
    _same_snapshot(_snapshot(a), _snapshot(b))
    again = tmp_path / "again.map"
    b.save_map(again)
    assert ref.check_directory(ref.parse(again.read_bytes())) is None
    a.save_map(path)
    assert again.read_bytes() == path.read_bytes()


# ---- c. chunk edges, byte for byte -----------------------------------------------------------------------------
def _grid_positions(n):
    i = np.arange(n)
    return np.stack([i % 32 - 16, (i // 32) % 32 - 16, i // 1024 - 3], axis=1).astype(np.int16)


@pytest.mark.parametrize("n_live,n_free", [(1, 0), (2, 1), (2047, 2), (2048, 2049), (2049, 4097), (4097, 2048),
                                           (0, 3)])
def test_chunk_edges_byte_for_byte(tmp_path, n_live, n_free):
    """n_live live blocks and n_free free blocks that have been in use: chunks of 2048 records, the colour section
    after the records"""
    import ratsdf
    n = n_live + n_free
    num_block = 1 << CFG["block_bits"]
    pos, t, c, p = craft(_grid_positions(n), seed=1000 + n)
    gone = np.zeros(n, dtype=bool)
    gone[np.random.default_rng(n).permutation(n)[:n_free]] = True
    a = engine(VS, (pos, t, c, p))
    b = engine(VS)
    try:
        # where the import has put each block (the placement only: every voxel word below is the test's own)
        _, blocks = a.dump_directory()
        row = {tuple(int(v) for v in q): j for j, q in enumerate(pos)}
        pool_row = {int(blk["idx"]): row[int(blk["x"]), int(blk["y"]), int(blk["z"])] for blk in blocks}
        assert len(pool_row) == n
        for _ in range(16):  # one deletion per bucket per pass (voxel_hash.cu:135-187)
            if a.num_active_blocks() > n_live:
                a.test_delete(pos[gone])
        assert a.num_active_blocks() == n_live
        path = tmp_path / "a.map"
        a.save_map(path)
        data = path.read_bytes()
        # (the checksum in Python is a loop over 64-bit words: for the large files the load below checks it)
        m = ref.parse(data, verify_checksum=n <= 64)

        assert m["num_free"] == num_block - n_live and m["free_low"] == num_block - n
        assert np.array_equal(m["heap"][:m["free_low"]], np.arange(m["free_low"]))
        used_free = m["heap"][m["free_low"]:]
        assert sorted(int(v) for v in used_free) == sorted(k for k, j in pool_row.items() if gone[j])
        live = m["blocks"]["idx"] >= 0
        assert int(live.sum()) == n_live == len(m["tsdf"]) and len(m["free_rgbw"]) == n_free
        assert np.all(m["blocks"]["idx"][live] >= m["free_low"])
        assert ref.check_directory(m) is None
        # the record of the entry at position p is what was imported at p, word for word
        rows = np.array([row[int(blk["x"]), int(blk["y"]), int(blk["z"])] for blk in m["blocks"][live]], dtype=np.int64)
        assert not gone[rows].any() and len(set(rows.tolist())) == n_live
        assert all(pool_row[int(k)] == j for k, j in zip(m["blocks"]["idx"][live], rows))
        for name, want in (("tsdf", t), ("rgbw", c), ("prob", p)):
            assert np.array_equal(m[name].view("<u4").reshape(n_live, 512),
                                  want[rows].view("<u4").reshape(n_live, 512)), name
        # the colour section: the deleted blocks' colour (the weight byte with it), in heap order
        free_rows = np.array([pool_row[int(k)] for k in used_free], dtype=np.int64)
        assert np.array_equal(m["free_rgbw"].view("<u4").reshape(n_free, 512),
                              c[free_rows].view("<u4").reshape(n_free, 512))

        assert ratsdf.map_file_info(path)["n_blocks"] == n_live
        b.load_map(path)
        _same_snapshot(_snapshot(a), _snapshot(b))
        # of a free block the map holds the colour words only: AquireBlock writes tsdf and probability anew
        x, y = a.dump_voxels(used_free)[1], b.dump_voxels(used_free)[1]
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        assert np.array_equal(y.view("<u4").reshape(n_free, 512), c[free_rows].view("<u4").reshape(n_free, 512))
        again = tmp_path / "b.map"
        b.save_map(again)
        assert again.read_bytes() == data
    finally:
        a.close()
        b.close()
