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


MAX_SHARD_SLAB_BITS = 31  # RATSDF_MAX_SHARD_SLAB_BITS (include/ratsdf.h)


def check_directory(m):
    """The directory rule of include/ratsdf_map.h on a parse() dict: None, or the name of the first violation --
    "H <field>" (the header names no configuration an engine can have), "D1" (a walk along the offsets does not end),
    "D2" (a live entry is not what a lookup of its position finds) or "D3" (the lookup steps over a dead node to find
    it).  Restated from the rule's text, one plain
    lookup per live entry; the engine's check is organised differently."""
    import math

    from kat_cases import ref_hash
    for f in ("voxel_size", "truncation"):
        if not (math.isfinite(m[f]) and m[f] > 0):
            return "H " + f
    if m["shard_count"] < 1:
        return "H shard_count"
    if m["shard_count"] > 1 and not 0 <= m["shard_rank"] < m["shard_count"]:
        return "H shard_rank"
    if not 1 <= m["shard_slab_bits"] <= MAX_SHARD_SLAB_BITS:
        return "H shard_slab_bits"
    bits = m["bucket_bits"]
    mask = (2 << bits) - 1
    b = m["blocks"]
    stored = {int(e): (int(b["x"][i]), int(b["y"][i]), int(b["z"][i]), int(b["offset"][i]), int(b["idx"][i]))
              for i, e in enumerate(m["entry_index"])}
    empty = (0, 0, 0, 0, -1)  # what an entry that is not stored reads as

    def offset(e):
        return stored.get(e, empty)[3]

    def step(e):  # int16 offset, sign-extended, added modulo 2^32, masked
        return ((e + (offset(e) & 0xFFFFFFFF)) & 0xFFFFFFFF) & mask

    def holds(e, p):
        x, y, z, _, idx = stored.get(e, empty)
        return idx >= 0 and (x, y, z) == p

    ends = set()  # D1, memoised: entries from which the walk is known to reach offset 0
    for e in stored:
        path, cur = [], e
        while cur not in ends and offset(cur) != 0:
            if len(path) >= len(stored):
                return "D1"
            path.append(cur)
            cur = step(cur)
        ends.update(path)

    def lookup(p):
        e0 = 2 * ref_hash(p, bits)
        if holds(e0, p):
            return e0
        if holds(e0 + 1, p):
            return e0 + 1
        last, over_dead = e0 + 1, False
        while offset(last) != 0:
            over_dead = over_dead or stored[last][4] < 0
            last = step(last)
            if holds(last, p):
                return "behind a dead node" if over_dead else last
        return None

    found = {e: lookup((x, y, z)) for e, (x, y, z, _, idx) in stored.items() if idx >= 0}
    if any(got != e and got != "behind a dead node" for e, got in found.items()):
        return "D2"
    if any(got != e for e, got in found.items()):
        return "D3"
    return None


def parse(data, verify_checksum=True):
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
    assert not verify_checksum or struct.unpack_from("<Q", data, off)[0] == checksum(data[:off]), "checksum"
    blocks = np.zeros(n_entries, dtype=BLOCK_DTYPE)
    for f in ("x", "y", "z", "offset", "idx"):
        blocks[f] = ent[f]
    return dict(voxel_size=vs, truncation=tr, block_bits=bb, bucket_bits=kb, shard_rank=srank, shard_count=scount,
                shard_slab_bits=sslab, segm_live=segm_live, num_free=num_free, free_low=free_low,
                entry_index=ent["entry"].astype(np.int32), blocks=blocks, heap=heap.copy(),
                tsdf=rec[:, 0:512].copy().view("<f4"), rgbw=rec[:, 512:1024].copy().view(RGBW_DTYPE),
                prob=rec[:, 1024:1536].copy().view("<f4"), free_rgbw=free.copy(),
                voxel_offset=off - free.nbytes - rec.nbytes)
