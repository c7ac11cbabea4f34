"""Map checkpoint files (include/ratsdf_map.h) without a GPU: the engine library's host-side validation
(ratsdf_map_file_info) against files written by tests/mapfile_ref.py from the CPU oracle's public dumps.  Two
independent implementations of the format pin it."""
import struct

import numpy as np
import pytest

import mapfile_ref as ref
from ratsdf import synthetic


@pytest.fixture(scope="module")
def oracle_map(oracle_lib):
    from ratsdf._abi import Engine
    vs = 0.02
    e = Engine(oracle_lib, vs, 6 * vs, block_bits=14, bucket_bits=16, threads=8)
    for f in synthetic.stream("sphere", 6, scale=0.25, noise=True, holes=True):
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
    data = ref.from_dumps(e)
    n_blocks = len(e.dump_directory()[0])
    e.close()
    return data, n_blocks


def _info(tmp_path, data, name="m.map"):
    import ratsdf
    p = tmp_path / name
    p.write_bytes(bytes(data))
    return ratsdf.map_file_info(p)


def _refused(tmp_path, data):
    import ratsdf
    with pytest.raises(ratsdf.RatsdfError) as ei:
        _info(tmp_path, data)
    assert ei.value.status == 1


def _rewrite(data, mutate):
    """parse, change, write again with a valid checksum: the refusal must come from the check of the content"""
    m = ref.parse(data)
    m = mutate(m) or m
    cfg = {k: m[k] for k in ("voxel_size", "truncation", "block_bits", "bucket_bits", "shard_rank", "shard_count",
                             "shard_slab_bits")}
    return ref.build(cfg, m["entry_index"], m["blocks"], m["heap"], m["free_low"], m["segm_live"], m["tsdf"],
                     m["rgbw"], m["prob"], m["free_rgbw"], version=m.get("version", 1))


def test_oracle_made_file_is_accepted(tmp_path, oracle_map):
    data, n_blocks = oracle_map
    assert n_blocks > 100
    info = _info(tmp_path, data)
    assert info["n_blocks"] == n_blocks
    assert info["voxel_size"] == np.float32(0.02) and info["truncation"] == np.float32(6 * 0.02)
    assert (info["block_bits"], info["bucket_bits"]) == (14, 16)
    assert (info["shard_rank"], info["shard_count"], info["shard_slab_bits"]) == (0, 1, 2)
    # the rewrite helper itself reproduces the file byte for byte
    assert _rewrite(data, lambda m: None) == data


def test_truncated_or_extended_file_is_refused(tmp_path, oracle_map):
    data, _ = oracle_map
    for cut in (len(data) - 1, len(data) - 8, len(data) // 2, 63, 0):
        _refused(tmp_path, data[:cut])
    _refused(tmp_path, data + b"\0" * 8)


def test_one_flipped_byte_in_each_section_is_refused(tmp_path, oracle_map):
    data, _ = oracle_map
    m = ref.parse(data)
    n_ent, nf = len(m["entry_index"]), m["num_free"]
    offsets = {
        "header: voxel size": 16, "header: num_free": 48, "header: n_blocks": 60,
        "entries": 64 + 16 * (n_ent // 2) + 3, "heap": 64 + 16 * n_ent + 4 * (nf // 2) + 1,
        "voxels": m["voxel_offset"] + 12345, "trailer": len(data) - 3,
    }
    if len(m["free_rgbw"]):
        offsets["colour of free blocks"] = len(data) - 8 - m["free_rgbw"].nbytes + 5
    for what, off in offsets.items():
        bad = bytearray(data)
        bad[off] ^= 0x10
        import ratsdf
        p = tmp_path / "flip.map"
        p.write_bytes(bytes(bad))
        with pytest.raises(ratsdf.RatsdfError) as ei:
            ratsdf.map_file_info(p)
        assert ei.value.status == 1, what


def test_wrong_version_is_refused(tmp_path, oracle_map):
    data, _ = oracle_map
    _refused(tmp_path, _rewrite(data, lambda m: m.update(version=2)))


def test_bad_pool_indices_and_heap_are_refused(tmp_path, oracle_map):
    data, _ = oracle_map

    def set_idx(value, which=0):
        def f(m):
            live = np.flatnonzero(m["blocks"]["idx"] >= 0)
            m["blocks"]["idx"][live[which]] = value
        return f

    _refused(tmp_path, _rewrite(data, set_idx(1 << 14)))          # past the pool
    m = ref.parse(data)
    live = m["blocks"]["idx"][m["blocks"]["idx"] >= 0]
    _refused(tmp_path, _rewrite(data, set_idx(int(live[1]))))     # a pool block named twice
    _refused(tmp_path, _rewrite(data, set_idx(-2)))               # neither a block nor a dead chain node

    def heap_dup(m):
        m["heap"][0] = int(live[0])                               # a free block that is also live
    _refused(tmp_path, _rewrite(data, heap_dup))

    def heap_range(m):
        m["heap"][-1] = 1 << 14
    _refused(tmp_path, _rewrite(data, heap_range))

    def below_free_low(m):
        m["heap"][[0, 1]] = m["heap"][[1, 0]]                     # never-used blocks out of their positions
    assert ref.parse(data)["free_low"] >= 2
    _refused(tmp_path, _rewrite(data, below_free_low))

    def entry_range(m):
        m["entry_index"][-1] = 2 << 16                            # past the directory
    _refused(tmp_path, _rewrite(data, entry_range))

    def entry_order(m):
        m["entry_index"][[0, 1]] = m["entry_index"][[1, 0]]       # not ascending
    _refused(tmp_path, _rewrite(data, entry_order))


def test_dead_chain_nodes_are_accepted(tmp_path, oracle_map):
    """an entry with idx -1 and a chain offset is stored (lookups walk over it); with offset 0 it would be empty and
    must not be in the file"""
    data, n_blocks = oracle_map
    m = ref.parse(data)
    e_free = int(np.setdiff1d(np.arange(2 << 16), m["entry_index"])[0])

    def add(offset):
        def f(mm):
            node = np.zeros(1, dtype=mm["blocks"].dtype)
            node["x"], node["offset"], node["idx"] = 7, offset, -1
            order = np.argsort(np.append(mm["entry_index"], e_free), kind="stable")
            mm["entry_index"] = np.append(mm["entry_index"], e_free)[order]
            mm["blocks"] = np.append(mm["blocks"], node)[order]
        return f

    assert _info(tmp_path, _rewrite(data, add(3)))["n_blocks"] == n_blocks
    _refused(tmp_path, _rewrite(data, add(0)))


def test_header_counts_must_agree_with_the_sections(tmp_path, oracle_map):
    data, _ = oracle_map

    def patch(off, fmt, value):
        body = bytearray(data[:-8])
        struct.pack_into(fmt, body, off, value)
        return bytes(body) + struct.pack("<Q", ref.checksum(body))

    m = ref.parse(data)
    _refused(tmp_path, patch(56, "<I", len(m["entry_index"]) + 1))  # n_entries
    _refused(tmp_path, patch(60, "<I", int(np.count_nonzero(m["blocks"]["idx"] >= 0)) - 1))  # n_blocks
    _refused(tmp_path, patch(52, "<i", m["num_free"] + 1))           # free_low above num_free
    _refused(tmp_path, patch(24, "<i", 30))                          # block_bits out of range


def test_missing_file_is_refused(tmp_path):
    import ratsdf
    with pytest.raises(ratsdf.RatsdfError) as ei:
        ratsdf.map_file_info(tmp_path / "absent.map")
    assert ei.value.status == 1


def test_oracle_reports_not_implemented(tmp_path, make_oracle):
    import ratsdf
    e = make_oracle(0.02, 0.12)
    for call in (e.save_map, e.load_map):
        with pytest.raises(ratsdf.RatsdfError) as ei:
            call(tmp_path / "x.map")
        assert ei.value.status == 6
