"""An independent writer and reader of the map checkpoint format (include/ratsdf_map.h, DESIGN.md 3 "Map files").

Written from the format's description only, so that the engine's files and this module's pin each other: the
tests build files from the CPU oracle's public dumps and check that the engine accepts them, and parse the
engine's files and compare them with the oracle's state.
"""
import struct

import numpy as np

from ratsdf._abi import BLOCK_DTYPE, RGBW_DTYPE

MAGIC = b"RATSDFMP"
HEADER = struct.Struct("<8sII2f10I")  # magic, version, header size, voxel size, truncation, 10 x 32-bit fields
assert HEADER.size == 64
ENTRY_DTYPE = np.dtype([("entry", "<u4"), ("x", "<i2"), ("y", "<i2"), ("z", "<i2"), ("offset", "<i2"),
                        ("idx", "<i4")])
assert ENTRY_DTYPE.itemsize == 16
RECORD_WORDS = 3 * 512
_MASK = (1 << 64) - 1


def checksum(data):
    """FNV-1a over the bytes read as little-endian 64-bit words, the last one zero-padded"""
    data = bytes(data)
    if len(data) % 8:
        data += b"\0" * (8 - len(data) % 8)
    h = 0xcbf29ce484222325
    for w in np.frombuffer(data, dtype="<u8").tolist():
        h = ((h ^ w) * 0x100000001b3) & _MASK
    return h


def build(cfg, entry_index, blocks, heap, free_low, segm_live, tsdf, rgbw, prob, free_rgbw, version=1):
    """The bytes of a map file.  cfg: voxel_size, truncation, block_bits, bucket_bits, shard_rank, shard_count,
    shard_slab_bits; entry_index / blocks: the stored entries, ascending; heap: heap[0 : num_free]; tsdf / rgbw /
    prob: [n_blocks, 512] for the entries with idx >= 0, in entry order; free_rgbw: [num_free - free_low, 512], the
    colour of the free blocks heap[free_low : num_free]."""
    blocks = np.asarray(blocks, dtype=BLOCK_DTYPE)
    heap = np.ascontiguousarray(heap, dtype="<i4")
    ent = np.zeros(len(blocks), dtype=ENTRY_DTYPE)
    ent["entry"] = entry_index
    for f in ("x", "y", "z", "offset", "idx"):
        ent[f] = blocks[f]
    n_blocks = len(tsdf)  # (== the entries with idx >= 0 in a well-formed file)
    rec = np.zeros((n_blocks, RECORD_WORDS), dtype="<u4")
    rec[:, 0:512] = np.ascontiguousarray(tsdf, dtype="<f4").reshape(n_blocks, 512).view("<u4")
    rec[:, 512:1024] = np.ascontiguousarray(rgbw, dtype=RGBW_DTYPE).reshape(n_blocks, 512).view("<u4")
    rec[:, 1024:1536] = np.ascontiguousarray(prob, dtype="<f4").reshape(n_blocks, 512).view("<u4")
    head = HEADER.pack(MAGIC, version, 64, cfg["voxel_size"], cfg["truncation"], cfg["block_bits"],
                       cfg["bucket_bits"], cfg["shard_rank"], cfg["shard_count"], cfg["shard_slab_bits"],
                       int(segm_live), len(heap), int(free_low), len(ent), n_blocks)
    free = np.ascontiguousarray(free_rgbw, dtype=RGBW_DTYPE).reshape(-1, 512)
    body = head + ent.tobytes() + heap.tobytes() + rec.tobytes() + free.tobytes()
    return body + struct.pack("<Q", checksum(body))


def engine_config(engine):
    """the configuration fields of a map file for an engine made with default shard settings"""
    return dict(voxel_size=engine.voxel_size, truncation=engine.truncation, block_bits=engine.block_bits,
                bucket_bits=engine.bucket_bits, shard_rank=0, shard_count=1, shard_slab_bits=2)


def from_dumps(engine, segm_live=1):
    """a map file's bytes from an engine's public dumps (the oracle's: it keeps no dead chain nodes -- the
    reference's Delete leaves {offset 0, idx -1} -- and no low-water mark of the free count, so free_low is the
    longest prefix of the heap that holds its own positions and colour 0 -- what the mark guarantees)"""
    entry_index, blocks = engine.dump_directory()
    num_free, heap = engine.dump_heap()
    heap = heap[:num_free]
    ident = np.flatnonzero(heap != np.arange(num_free))
    free_low = int(ident[0]) if ident.size else num_free
    if free_low:
        _, c, _ = engine.dump_voxels(heap[:free_low])
        coloured = np.flatnonzero(c.view("<u4").any(axis=1))
        free_low = int(coloured[0]) if coloured.size else free_low
    tsdf, rgbw, prob = engine.dump_voxels(blocks["idx"])
    _, free_rgbw, _ = engine.dump_voxels(heap[free_low:])
    return build(engine_config(engine), entry_index, blocks, heap, free_low, segm_live, tsdf, rgbw, prob, free_rgbw)


def parse(data):
    """a map file's bytes -> dict of its header fields and sections (checks sizes and the checksum)"""
    data = bytes(data)
    (magic, version, hsize, vs, tr, bb, kb, srank, scount, sslab, segm_live, num_free, free_low, n_entries,
     n_blocks) = HEADER.unpack_from(data, 0)
    assert magic == MAGIC and version == 1 and hsize == 64
    off = 64
    ent = np.frombuffer(data, dtype=ENTRY_DTYPE, count=n_entries, offset=off)
    off += 16 * n_entries
    heap = np.frombuffer(data, dtype="<i4", count=num_free, offset=off)
    off += 4 * num_free
    rec = np.frombuffer(data, dtype="<u4", count=n_blocks * RECORD_WORDS, offset=off).reshape(n_blocks, RECORD_WORDS)
    off += rec.nbytes
    free = np.frombuffer(data, dtype=RGBW_DTYPE, count=(num_free - free_low) * 512, offset=off).reshape(-1, 512)
    off += free.nbytes
    assert len(data) == off + 8, "file size does not match the header"
    assert struct.unpack_from("<Q", data, off)[0] == checksum(data[:off]), "checksum"
    blocks = np.zeros(n_entries, dtype=BLOCK_DTYPE)
    for f in ("x", "y", "z", "offset", "idx"):
        blocks[f] = ent[f]
    return dict(voxel_size=vs, truncation=tr, block_bits=bb, bucket_bits=kb, shard_rank=srank, shard_count=scount,
                shard_slab_bits=sslab, segm_live=segm_live, num_free=num_free, free_low=free_low,
                entry_index=ent["entry"].astype(np.int32), blocks=blocks, heap=heap.copy(),
                tsdf=rec[:, 0:512].copy().view("<f4"), rgbw=rec[:, 512:1024].copy().view(RGBW_DTYPE),
                prob=rec[:, 1024:1536].copy().view("<f4"), free_rgbw=free.copy(),
                voxel_offset=off - free.nbytes - rec.nbytes)
