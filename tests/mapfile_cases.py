"""Map files that are well formed -- sizes, indices, heap and checksum all right -- and whose directory or header is
wrong, made from a good file's bytes: the cases of tests/test_mapfile_directory.py (no GPU) and of
tests/test_gpu_mapfile_cases.py.  Every case names the part of the directory rule (include/ratsdf_map.h,
mapfile_ref.check_directory) that it breaks."""
import struct

import numpy as np

import mapfile_ref as ref
from kat_cases import ref_hash

CFG_KEYS = ("voxel_size", "truncation", "block_bits", "bucket_bits", "shard_rank", "shard_count", "shard_slab_bits")
# byte offsets of header fields (include/ratsdf_map.h)
OFF_VOXEL_SIZE, OFF_TRUNCATION, OFF_SHARD_RANK, OFF_SHARD_COUNT, OFF_SHARD_SLAB_BITS = 16, 20, 32, 36, 40


def write(m):
    """a parse() dict back into bytes with a valid checksum"""
    return ref.build({k: m[k] for k in CFG_KEYS}, m["entry_index"], m["blocks"], m["heap"], m["free_low"],
                     m["segm_live"], m["tsdf"], m["rgbw"], m["prob"], m["free_rgbw"])


def rewrite(data, mutate):
    """parse, change, write again with a valid checksum: a refusal must come from the check of the content"""
    m = ref.parse(data)
    mutate(m)
    return write(m)


def patch(data, off, fmt, value):
    """one header field overwritten in place (signed fields too), the checksum made right again"""
    body = bytearray(data[:-8])
    struct.pack_into(fmt, body, off, value)
    return bytes(body) + struct.pack("<Q", ref.checksum(body))


# ---- reading a directory ---------------------------------------------------------------------------------------
def n_entry(m):
    return 2 << m["bucket_bits"]


def record(m, entry):
    """index of the stored record of `entry`"""
    i = int(np.searchsorted(m["entry_index"], entry))
    assert i < len(m["entry_index"]) and m["entry_index"][i] == entry, f"entry {entry} is not stored"
    return i


def stored(m, entry):
    i = int(np.searchsorted(m["entry_index"], entry))
    return i < len(m["entry_index"]) and m["entry_index"][i] == entry


def position(m, entry):
    b = m["blocks"][record(m, entry)]
    return int(b["x"]), int(b["y"]), int(b["z"])


def live(m, entry):
    return stored(m, entry) and m["blocks"]["idx"][record(m, entry)] >= 0


def bucket_of(m, entry):
    """the bucket a live entry's position hashes to"""
    return ref_hash(position(m, entry), m["bucket_bits"])


def at_home(m, entry):
    return live(m, entry) and bucket_of(m, entry) == entry >> 1


def chained(m):
    """the live entries that sit outside their bucket's two home entries"""
    return [int(e) for e in m["entry_index"] if live(m, int(e)) and bucket_of(m, int(e)) != int(e) >> 1]


def wrap_links(m):
    """the stored entries whose offset leads across the table's end"""
    off = m["blocks"]["offset"].astype(np.int64)
    to = m["entry_index"].astype(np.int64) + off
    return [int(e) for e in m["entry_index"][(off != 0) & ((to < 0) | (to >= n_entry(m)))]]


def chains(m):
    """[list head, node, node, ...] (entry indices) for every bucket whose list head links on, longest first"""
    out = []
    for e in m["entry_index"]:
        e = int(e)
        if e & 1 and m["blocks"]["offset"][record(m, e)] != 0:
            c = [e]
            while stored(m, c[-1]) and m["blocks"]["offset"][record(m, c[-1])] != 0:
                c.append((c[-1] + int(m["blocks"]["offset"][record(m, c[-1])])) & (n_entry(m) - 1))
                assert len(c) <= len(m["entry_index"]) + 1, "the good file's chain does not end"
            if not stored(m, c[-1]):  # (the last link may lead to a deleted tail: an empty entry, not in the file)
                c.pop()
            out.append(c)
    return sorted(out, key=lambda c: (-len(c), c[0]))


def free_entries(m, count, even=True):
    """`count` entries that are not stored and that no stored offset leads to"""
    taken = set(int(e) for e in m["entry_index"])
    taken |= set((int(e) + int(o)) & (n_entry(m) - 1) for e, o in zip(m["entry_index"], m["blocks"]["offset"]))
    out = [e for e in range(0, n_entry(m), 2 if even else 1) if e not in taken]
    assert len(out) >= count
    return out[:count]


# ---- changing a directory --------------------------------------------------------------------------------------
def set_position(m, entry, p):
    i = record(m, entry)
    m["blocks"]["x"][i], m["blocks"]["y"][i], m["blocks"]["z"][i] = p


def set_offset(m, entry, value):
    assert -32768 <= value <= 32767
    m["blocks"]["offset"][record(m, entry)] = value


def link(m, src, dst, forward=False):
    """src's offset made to lead to dst: the shortest way round the table, or, with `forward`, upwards (through the
    table's end if dst lies below src)"""
    n = n_entry(m)
    v = (dst - src) % n
    if not forward and v >= n // 2:
        v -= n
    assert v != 0
    set_offset(m, src, v)


def add_dead(m, entry, offset):
    """a dead chain node {idx -1, offset} stored at an entry that was not"""
    assert not stored(m, entry) and offset != 0
    node = np.zeros(1, dtype=m["blocks"].dtype)
    node["x"], node["offset"], node["idx"] = 7, offset, -1
    index = np.append(m["entry_index"], np.int32(entry))
    order = np.argsort(index, kind="stable")
    m["entry_index"] = index[order]
    m["blocks"] = np.append(m["blocks"], node)[order]


def unstore(m, entry):
    """a dead chain node taken out of the file (it then reads as {offset 0, idx -1})"""
    i = record(m, entry)
    assert m["blocks"]["idx"][i] < 0
    m["entry_index"] = np.delete(m["entry_index"], i)
    m["blocks"] = np.delete(m["blocks"], i)


def kill(m, entry):
    """a live entry that links on made a dead chain node, as a delete that kept the links would leave it: the entry
    keeps its offset, its pool block goes on top of the free list, its record leaves the voxel section and its colour
    joins the free blocks' (the file stays well formed, and lookups walk over the node)"""
    i = record(m, entry)
    assert m["blocks"]["idx"][i] >= 0 and m["blocks"]["offset"][i] != 0
    j = int(np.count_nonzero(m["blocks"]["idx"][:i] >= 0))  # its place in the voxel section
    m["heap"] = np.append(m["heap"], m["blocks"]["idx"][i]).astype("<i4")
    m["num_free"] += 1
    m["free_rgbw"] = np.concatenate([m["free_rgbw"], m["rgbw"][j:j + 1]])
    for k in ("tsdf", "rgbw", "prob"):
        m[k] = np.delete(m[k], j, axis=0)
    m["blocks"]["idx"][i] = -1


def _elsewhere(m, entry, avoid):
    """a position near `entry`'s that no entry holds and that hashes to none of the buckets in `avoid`"""
    held = set(zip(m["blocks"]["x"].tolist(), m["blocks"]["y"].tolist(), m["blocks"]["z"].tolist()))
    x, y, z = position(m, entry)
    for dx in range(1, 1000):
        p = (x + dx, y, z)
        if p not in held and ref_hash(p, m["bucket_bits"]) not in avoid:
            return p
    raise AssertionError("no position found")


def _live_chain(m):
    """(chain, k): the longest chain and the place in it of its last live node, which is not the list head"""
    for c in chains(m):
        for k in range(len(c) - 1, 0, -1):
            if live(m, c[k]):
                return c, k
    raise AssertionError("the good file has no live chain node")


def _full_bucket(m):
    """a bucket's first home entry, where both home entries are live blocks of that bucket"""
    for e in m["entry_index"]:
        e = int(e)
        if not e & 1 and at_home(m, e) and at_home(m, e + 1):
            return e
    raise AssertionError("the good file has no bucket with two blocks at home")


# ---- the defects -----------------------------------------------------------------------------------------------
# a live entry's position or placement: rule D2
def moved_home_entry(m):
    e = next(int(e) for e in m["entry_index"] if at_home(m, int(e)))
    set_position(m, e, _elsewhere(m, e, {e >> 1}))


def moved_chain_node(m):
    c, k = _live_chain(m)
    set_position(m, c[k], _elsewhere(m, c[k], {c[0] >> 1, c[k] >> 1}))


def cut_link(m):
    c, k = _live_chain(m)
    if live(m, c[k - 1]):
        set_offset(m, c[k - 1], 0)
    else:  # (a dead node with offset 0 is an empty entry, which a file does not store)
        unstore(m, c[k - 1])


def duplicate_in_home_entries(m):
    e = _full_bucket(m)
    set_position(m, e + 1, position(m, e))


def duplicate_in_chain(m):
    c, k = _live_chain(m)
    home = next(e for e in (c[0] - 1, c[0]) if at_home(m, e))
    set_position(m, c[k], position(m, home))


# the chain offsets: rule D1
def two_entry_cycle(m):
    c = chains(m)[0]
    link(m, c[-1], c[-2])


def self_cycle(m):
    """an offset of the table's size leads back to the entry itself"""
    assert self_cycle_exists(m)
    set_offset(m, chains(m)[0][-1], n_entry(m))


def self_cycle_exists(m):
    return n_entry(m) <= 32767


def long_cycle(m):
    """a ring of three entries or more behind the longest chain's list head, which leads into it and is not part of
    it; a chain too short for that is closed as a whole, with a block from elsewhere taken in if it has two entries"""
    c = list(chains(m)[0])
    if len(c) >= 4:
        link(m, c[-1], c[1])
        return
    if len(c) < 3:
        extra = next(int(e) for e, b in zip(m["entry_index"], m["blocks"])
                     if b["idx"] >= 0 and b["offset"] == 0 and not int(e) & 1 and int(e) not in c)
        link(m, c[-1], extra)
        c.append(extra)
    link(m, c[-1], c[0])
    assert len(c) >= 3


def cycle_through_the_end(m):
    """a ring with a link across the table's end: a chain that wraps, closed; without one, the highest and the lowest
    entry with offset 0 linked upwards through the end and back"""
    wrap = set(wrap_links(m))
    for c in chains(m):
        if wrap & set(c[:-1]):
            link(m, c[-1], c[0])
            return
    ends = [int(e) for e, b in zip(m["entry_index"], m["blocks"]) if b["idx"] >= 0 and b["offset"] == 0]
    lo, hi = ends[0], ends[-1]
    assert lo < hi
    link(m, hi, lo, forward=True)
    link(m, lo, hi, forward=True)
    assert wrap_links(m)


def dead_cycle(m):
    """two dead nodes on no chain that lead to each other"""
    a, b = free_entries(m, 2)
    add_dead(m, a, b - a)
    add_dead(m, b, a - b)


# a dead node with a block behind it: rule D3
def dead_list_head(m):
    c, _ = _live_chain(m)
    kill(m, c[0])


def dead_node_before_a_block(m):
    """the node before the chain's last block: a middle node where the chain has one, else the list head"""
    c, k = _live_chain(m)
    kill(m, c[k - 1])


D3_DEFECTS = [dead_list_head, dead_node_before_a_block]
D2_DEFECTS = [moved_home_entry, moved_chain_node, cut_link, duplicate_in_home_entries, duplicate_in_chain]
D1_DEFECTS = [two_entry_cycle, self_cycle, long_cycle, cycle_through_the_end, dead_cycle]

_BAD_FLOATS = {"nan": float("nan"), "inf": float("inf"), "zero": 0.0, "negative": -0.02}


def header_defects(data):
    """{name: (bytes, violation)}: rule H"""
    out = {}
    for field, off in (("voxel_size", OFF_VOXEL_SIZE), ("truncation", OFF_TRUNCATION)):
        for what, v in _BAD_FLOATS.items():
            out[f"{field}_{what}"] = (patch(data, off, "<f", v), "H " + field)
    out["shard_count_zero"] = (patch(data, OFF_SHARD_COUNT, "<i", 0), "H shard_count")
    three = patch(data, OFF_SHARD_COUNT, "<i", 3)
    out["shard_rank_is_count"] = (patch(three, OFF_SHARD_RANK, "<i", 3), "H shard_rank")
    out["shard_rank_negative"] = (patch(three, OFF_SHARD_RANK, "<i", -1), "H shard_rank")
    for v in (0, -1, ref.MAX_SHARD_SLAB_BITS + 1, 40):
        out[f"shard_slab_bits_{v}"] = (patch(data, OFF_SHARD_SLAB_BITS, "<i", v), "H shard_slab_bits")
    return out


HEADER_DEFECTS = ([f"{f}_{w}" for f in ("voxel_size", "truncation") for w in _BAD_FLOATS] +
                  ["shard_count_zero", "shard_rank_is_count", "shard_rank_negative"] +
                  [f"shard_slab_bits_{v}" for v in (0, -1, ref.MAX_SHARD_SLAB_BITS + 1, 40)])


def defects(data):
    """{name: (bytes, violation)} of every defect for the good file `data`; a self-cycle is left out where no int16
    offset is a multiple of the table's size (bucket_bits >= 14)"""
    out = {}
    for rule, group in (("D2", D2_DEFECTS), ("D1", D1_DEFECTS), ("D3", D3_DEFECTS)):
        for f in group:
            if f is self_cycle and not self_cycle_exists(ref.parse(data)):
                continue
            out[f.__name__] = (rewrite(data, f), rule)
    out.update(header_defects(data))
    return out


def with_orphan_dead_node(data):
    """the good file with a dead chain node on no chain, leading to an entry that is not stored: accepted"""
    def f(m):
        a, b = free_entries(m, 2)
        add_dead(m, a, b - a)
    return rewrite(data, f)
