"""Crafted maps, bounds and a numpy restatement for the record read-outs: ratsdf_query (TSDFSystem::Query),
ratsdf_gather_valid, ratsdf_gather_valid_semantic and the ratsdf_download_all file.  Written once and run against the CPU
oracle (tests/test_query_cases.py, no GPU) and the HIP engine (tests/test_gpu_query.py).  Same role as raycast_cases.py:
no GPU and no torch at import.

The restatement follows include/ratsdf.h and the reference lines it cites, not the engine's code:
  * voxel_tsdf.cuh:28-33 and voxel_tsdf.cu:534: every bound is the float32 product of the bound and (float)(1. / vs),
    converted as static_cast<short> of device code: truncation towards zero, NaN -> 0, saturation at the int32 range,
    and only then the cut to the low 16 bits;
  * voxel_tsdf.cu:15-26: a block is taken when, per axis, g >= min and g + 7 <= max, g = (short)(block << 3), the sums
    evaluated in int;
  * voxel_tsdf.cu:35-62: voxel t of block b lies at float((short)((short)(b << 3) + t)) * vs; tsdf and probability are
    copied;
  * ratsdf.h: blocks by ascending hash-entry index, voxels by x + 8y + 64z.
Everything is compared as bytes: NaN payloads, -0.0 and denormals count.

The maps are written voxel by voxel.  load() brings the blocks into the directory with test_allocate passes (the
reference's own insertion, one per bucket and pass, in list order: where an entry index is stated by hand it follows
from that) and then overwrites their voxels with import_blocks.  Every voxel value is a function of the voxel's integer
coordinate 8 * block + local, so a record from another voxel or block shows; weights include 0 (the gathers do not
filter on weight).  The block SPECIAL_ROW of every map holds NaNs, -0.0, +-inf and denormals in known slots.
"""
import functools
from typing import NamedTuple

import numpy as np

from kat_cases import ref_hash
from ratsdf._abi import RGBW_DTYPE, VOXEL_SEGM_DTYPE, VOXEL_TSDF_DTYPE
from raycast_cases import BlockSet, block_keys

VS = 0.02
TRUNC = 6 * VS
F = np.float32
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
def wrap16(v):
    """the low 16 bits of integers as int16 values (held in int64)"""
    return ((np.asarray(v).astype(np.int64) + 32768) & 0xFFFF) - 32768


def float_to_short(p):
    """static_cast<short>(float) of device code, for a float32 array: int64 values in the int16 range"""
    p = np.asarray(p, dtype=F)
    nan = np.isnan(p)
    with np.errstate(invalid="ignore"):
        t = np.trunc(np.where(nan, F(0), p).astype(np.float64))
    i = np.where(t >= 2.0 ** 31, INT_MAX, np.where(t <= -2.0 ** 31, INT_MIN, np.clip(t, INT_MIN, INT_MAX))).astype(np.int64)
    return wrap16(np.where(nan, 0, i))


def grid_bounds(bounds, vs):
    """(xmin, xmax, ymin, ymax, zmin, zmax) in metres -> the six int16 of BoundingCube<short>, as a tuple of ints"""
    scale = F(1.0 / float(F(vs)))
    with np.errstate(over="ignore", invalid="ignore"):
        prod = np.asarray(bounds, dtype=F) * scale
    return tuple(int(v) for v in float_to_short(prod))


def select(blocks, gb):
    """[n] bool: the blocks (positions [n, 3]) that lie wholly inside the grid bounds `gb`; int64 arithmetic"""
    g = wrap16(np.asarray(blocks).astype(np.int64).reshape(-1, 3) << 3)
    lo = np.array([gb[0], gb[2], gb[4]], dtype=np.int64)
    hi = np.array([gb[1], gb[3], gb[5]], dtype=np.int64)
    return np.all((g >= lo) & (g + 7 <= hi), axis=1)


_T = np.arange(512)
LOCAL = np.stack([_T & 7, (_T >> 3) & 7, _T >> 6], axis=1)      # voxel x + 8y + 64z of a block


def records(blocks, entry_index, tsdf, prob, vs, semantic):
    """the records of `blocks` ([n, 3], with their hash-entry indices, which must ascend) holding the voxels tsdf /
    prob ([n, 512] float32): 16-byte records, or 20-byte ones with the probability"""
    blocks = np.asarray(blocks).astype(np.int64).reshape(-1, 3)
    entry_index = np.asarray(entry_index).astype(np.int64)
    assert len(entry_index) == len(blocks) and (np.diff(entry_index) > 0).all(), "blocks go by ascending entry index"
    n = len(blocks)
    out = np.zeros((n, 512), dtype=VOXEL_SEGM_DTYPE if semantic else VOXEL_TSDF_DTYPE)
    g = wrap16(wrap16(blocks << 3)[:, None, :] + LOCAL[None])                  # (short)((short)(b << 3) + t)
    for k, name in enumerate(("x", "y", "z")):
        out[name] = g[..., k].astype(F) * F(vs)
    out["tsdf"].view(np.uint32)[...] = np.ascontiguousarray(tsdf, dtype=F).reshape(n, 512).view(np.uint32)
    if semantic:
        out["prob"].view(np.uint32)[...] = np.ascontiguousarray(prob, dtype=F).reshape(n, 512).view(np.uint32)
    return out.reshape(-1)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def first_difference(got, want):
    """for messages: (record index, block, voxel slot) of the first record whose bytes differ, or the two lengths"""
    if len(got) != len(want):
        return f"{len(got)} records, {len(want)} expected"
    a = np.ascontiguousarray(got).view(np.uint8).reshape(len(got), -1)
    b = np.ascontiguousarray(want).view(np.uint8).reshape(len(want), -1)
    bad = np.flatnonzero((a != b).any(axis=1))
    if len(bad) == 0:
        return "equal"
    i = int(bad[0])
    return f"{len(bad)} records differ, the first is record {i} (block {i >> 9}, slot {i & 511}): {got[i]} != {want[i]}"


def rows_of(m, blocks):
    """the rows of the map `m` that hold the blocks at `blocks` ([n, 3]); every one must be there"""
    keys = block_keys(m.pos)
    order = np.argsort(keys)
    want = block_keys(np.asarray(blocks).reshape(-1, 3))
    at = np.minimum(np.searchsorted(keys[order], want), len(keys) - 1)
    assert (keys[order][at] == want).all(), "the directory holds a block the map does not"
    return order[at]


def directory_positions(dir_blocks):
    return np.stack([dir_blocks["x"], dir_blocks["y"], dir_blocks["z"]], axis=1).astype(np.int64)


def expected(m, entry_index, dir_blocks, semantic, gb=None, vs=VS):
    """what a read-out of the map `m` must return given the directory (entry indices and blocks as dump_directory()
    or a hand-written table states them): every block, or with `gb` the blocks inside those grid bounds"""
    structured = isinstance(dir_blocks, np.ndarray) and dir_blocks.dtype.names is not None
    pos = directory_positions(dir_blocks) if structured else np.asarray(dir_blocks).astype(np.int64).reshape(-1, 3)
    entry_index = np.asarray(entry_index).astype(np.int64)
    rows = rows_of(m, pos)
    if gb is not None:
        keep = select(pos, gb)
        pos, entry_index, rows = pos[keep], entry_index[keep], rows[keep]
    return records(pos, entry_index, m.tsdf[rows], m.prob[rows], vs, semantic)


# ---------------------------------------------------------------------------------------------------------------------
# voxel values
SPECIAL_ROW = 0
# slot -> bits: a quiet NaN with a payload, -0.0, +inf, -inf, the smallest denormal, a negative signalling NaN; a
# negative denormal in the last slot
SPECIAL_TSDF = {0: 0x7FC12345, 1: 0x80000000, 2: 0x7F800000, 3: 0xFF800000, 4: 0x00000001, 5: 0xFFA00001,
                511: 0x80000100}
SPECIAL_PROB = {7: 0x7FC00ABC, 8: 0x80000000, 9: 0x00000002, 10: 0x7F800000, 504: 0xFF800000}


def voxel_coordinates(pos):
    """[n, 512, 3] int64: 8 * block + local, NOT wrapped (block 4096 and block -4096 get different values)"""
    return np.asarray(pos).astype(np.int64).reshape(-1, 3)[:, None, :] * 8 + LOCAL[None]


def tsdf_of(v):
    """(k - 2^23) / 2^23 with k = (73856093 x + 19349669 y + 83492791 z) mod 16777213: exact in float32, in [-1, 1),
    and scattered: neighbouring voxels, blocks and strides of either do not repeat a value"""
    k = np.mod(73856093 * v[..., 0] + 19349669 * v[..., 1] + 83492791 * v[..., 2], 16777213)
    return ((k - 2 ** 23).astype(np.float64) / 2.0 ** 23).astype(F)


def prob_of(v):
    """((7 x + 13 y + 17 z) mod 1021) / 1024: exact in float32, in [0, 1)"""
    return (np.mod(7 * v[..., 0] + 13 * v[..., 1] + 17 * v[..., 2], 1021).astype(np.float64) / 1024.0).astype(F)


def make_map(pos, special_row=SPECIAL_ROW):
    pos = np.asarray(pos, dtype=np.int64).reshape(-1, 3)
    assert len(np.unique(block_keys(pos))) == len(pos) and pos.min() >= -32768 and pos.max() <= 32767
    v = voxel_coordinates(pos)
    rgbw = np.zeros(v.shape[:2], dtype=RGBW_DTYPE)
    rgbw["r"] = (37 * v[..., 0]) & 255
    rgbw["g"] = (59 * v[..., 1]) & 255
    rgbw["b"] = (83 * v[..., 2]) & 255
    rgbw["weight"] = (v[..., 0] + 3 * v[..., 1] + 5 * v[..., 2]) & 3            # 0 .. 3: a quarter are unobserved
    tsdf, prob = tsdf_of(v), prob_of(v)
    if special_row is not None:
        for slot, bits in SPECIAL_TSDF.items():
            tsdf.view(np.uint32)[special_row, slot] = bits
        for slot, bits in SPECIAL_PROB.items():
            prob.view(np.uint32)[special_row, slot] = bits
    return BlockSet(pos.astype(np.int16), tsdf, rgbw, prob)


def _cube(lo, hi):
    """all integer points of [lo, hi) per axis, [n, 3], x slowest"""
    ax = [np.arange(int(a), int(b)) for a, b in zip(lo, hi)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the maps.  `engine`: the table sizes the map is loaded into.
class Map(NamedTuple):
    name: str
    blocks: BlockSet
    engine: dict


@functools.lru_cache(maxsize=None)
def signs():
    """4 x 4 x 4 blocks around the origin, blocks -2 .. 1 per axis (voxels -16 .. 15): all eight sign combinations"""
    return Map("signs", make_map(_cube((-2, -2, -2), (2, 2, 2))), dict(block_bits=8, bucket_bits=12))


NUM_BUCKET = 1 << 21
LAST = 2 * NUM_BUCKET
# kat_cases.case_collision's blocks, in its list order, and five more in buckets of their own
COLLISION = [(33, 180, 42), (61, 16, 170), (63, 171, 45), (0, 0, 0)]
APART = [(1, 1, 1), (-1, -1, -1), (1, 0, 0), (0, -3, 0), (-4096, 4095, 2)]


def known_order_entries():
    """{entry index: block} of the known_order map after load(), without asking any engine: voxel_hash.cu:46-108 under
    the list-order linearisation puts the first of the three colliders into the first slot of bucket 2^21 - 1 (entry
    last - 2), the second into the list-head slot (last - 1), the third where the probe from there wraps to: entry 2, the
    first free slot after bucket 0's entry 0, which block (0, 0, 0) took (kat_cases.case_collision states the same).  A
    block alone in bucket h takes that bucket's first slot, entry 2h."""
    table = {LAST - 2: COLLISION[0], LAST - 1: COLLISION[1], 2: COLLISION[2], 0: COLLISION[3]}
    for p in APART:
        h = ref_hash(p)
        assert h not in (0, 1, NUM_BUCKET - 1) and 2 * h not in table      # bucket 1's first slot is entry 2: taken
        table[2 * h] = p
    return table


@functools.lru_cache(maxsize=None)
def known_order():
    """entry 0, entry 2, five entries in between and the table's last word (the default 2^21 buckets: 65536 occupancy
    words, 256 workgroups of the selection).  The special block is the LAST entry's."""
    return Map("known_order", make_map(COLLISION + APART, special_row=1), dict(block_bits=8, bucket_bits=21))


EDGE_BLOCKS = [(4095, 0, 0), (-4096, 0, 0), (0, 4095, 0), (0, -4096, 0), (0, 0, 4095), (0, 0, -4096), (4096, 0, 0),
               (0, 0, 0)]


@functools.lru_cache(maxsize=None)
def edges():
    """blocks 4095 and -4096 on each axis (voxels 32760 .. 32767 and -32768 .. -32761), block 4096 on x, whose voxel
    coordinates wrap to -32768 .. -32761 like block -4096's, and the block at the origin"""
    return Map("edges", make_map(EDGE_BLOCKS, special_row=6), dict(block_bits=8, bucket_bits=12))


SIZES = (1, 3, 4, 5, 409, 410, 511, 512, 513, 4095, 4096, 4097)
# 2^13 pool blocks for up to 4097; 2^15 buckets: 65536 entries are 1024 occupancy words, four workgroups of the
# selection kernels, and the directory and its bitmaps stay below 1 MiB
SIZES_ENGINE = dict(block_bits=13, bucket_bits=15)
# 512-voxel blocks of 16-byte records reach 4 MiB at 512 blocks, of 20-byte records at 410: the host copy changes there
assert 511 * 512 * 16 < 4 << 20 <= 512 * 512 * 16 and 409 * 512 * 20 < 4 << 20 <= 410 * 512 * 20


@functools.lru_cache(maxsize=None)
def sizes(n):
    """n blocks along a line in x that crosses zero, at y = 3, z = -2"""
    assert 1 <= n <= 4097
    x = np.arange(n) - min(n // 2, 2000)
    pos = np.stack([x, np.full(n, 3), np.full(n, -2)], axis=1)
    return Map(f"sizes_{n}", make_map(pos, special_row=n - 1), SIZES_ENGINE)


def sizes_one_block_box(n):
    """a box that takes the single block (0, 3, -2) of sizes(n), and one in the empty space beside the line"""
    return voxel_box((0, 7), (24, 31), (-16, -9)), voxel_box((0, 7), (40, 47), (-16, -9))


@functools.lru_cache(maxsize=None)
def tiny_table():
    """200 blocks in a directory of 512 buckets (1024 entries: 16 occupancy words, one partial workgroup): full
    buckets and chains"""
    pos = _cube((-3, -3, -3), (3, 3, 3))
    pos = pos[(np.arange(len(pos)) % 27) >= 2]           # 216 - 16
    assert len(pos) == 200
    return Map("tiny_table", make_map(pos, special_row=199), dict(block_bits=9, bucket_bits=9))


def maps():
    """the maps every bounds-free read-out runs on (sizes(n) is driven size by size)"""
    return [signs(), known_order(), edges(), tiny_table()]


def load(e, m, passes=64):
    """the map `m` (a Map or a BlockSet) into the engine `e`: test_allocate passes in list order until every block is
    in (one insertion per bucket and pass), then the voxels.  Returns the number of passes."""
    b = m.blocks if isinstance(m, Map) else m
    for used in range(passes + 1):
        if e.num_active_blocks() == len(b):
            break
        e.test_allocate(b.pos)
    assert e.num_active_blocks() == len(b), f"{e.num_active_blocks()} of {len(b)} blocks after {passes} passes"
    e.import_blocks(*b)
    assert e.num_active_blocks() == len(b)
    return used


# ---------------------------------------------------------------------------------------------------------------------
# bounds
class Case(NamedTuple):
    name: str
    bounds: tuple     # metres: xmin, xmax, ymin, ymax, zmin, zmax
    grid: tuple       # the six int16 they convert to, by hand
    count: int        # the blocks of the map they select, by hand


def at(v):
    """metres that convert to voxel `v` whatever the rounding of the product: half a voxel further from zero (the
    conversion truncates towards zero), 0 for voxel 0"""
    return float(F((v + (0.5 if v > 0 else -0.5 if v < 0 else 0.0)) * VS))


def voxel_box(x, y, z):
    """bounds in metres that convert to the voxel ranges x, y, z (each (min, max), inclusive)"""
    return tuple(at(v) for ax in (x, y, z) for v in ax)


ALL = (-16, 15)           # the voxel range of `signs` per axis
NAN, INF = float("nan"), float("inf")


def _x(name, xmin, xmax, grid_x, count, y=ALL, z=ALL):
    """a case of `signs` whose x bounds are given in METRES, y and z in voxels"""
    yz = voxel_box((0, 0), y, z)[2:]
    return Case(name, (xmin, xmax) + yz, tuple(grid_x) + tuple(y) + tuple(z), count)


def signs_cases():
    """x-blocks -2, -1, 0, 1 start at voxels -16, -8, 0, 8 and end at -9, -1, 7, 15; a selected x-range of k blocks
    with all of y and z counts 16 k blocks."""
    a = at
    return [
        Case("everything", voxel_box(ALL, ALL, ALL), ALL * 3, 64),
        # faces exactly on block boundaries
        _x("xmax_on_last_voxel", a(-16), a(7), (-16, 7), 48),            # 8 * 0 + 7: block 0 is in
        _x("xmax_one_short", a(-16), a(6), (-16, 6), 32),                # 8 * 0 + 6: block 0 is out
        _x("xmin_on_first_voxel", a(-8), a(15), (-8, 15), 48),           # 8 * -1: block -1 is in
        _x("xmin_one_inside", a(-7), a(15), (-7, 15), 32),               # 8 * -1 + 1: block -1 is out
        # half-voxel offsets: truncation towards zero (floor would make -7.5 -> -8, rounding 6.5 -> 7)
        _x("xmin_-8.9_voxels", -8.9 * VS, a(15), (-8, 15), 48),
        _x("xmin_-7.5_voxels", -7.5 * VS, a(15), (-7, 15), 32),
        _x("xmax_7.9_voxels", a(-16), 7.9 * VS, (-16, 7), 48),
        _x("xmax_6.5_voxels", a(-16), 6.5 * VS, (-16, 6), 32),
        _x("xmax_-0.5_voxels", a(-16), -0.5 * VS, (-16, 0), 32),         # -0.5 -> 0 (blocks -2, -1 either way)
        _x("xmin_0.5_voxels", 0.5 * VS, a(15), (0, 15), 32),
        # decimal literals: float32(1 / float32(0.02)) is exactly 50, and float32(0.16) * 50 = 7.99999982... rounds to
        # the float32 8.0; likewise -8.0 and 16.0.  1.06 is the first multiple of 2 cm whose float32 product lands
        # below its integer: 52.999996 -> 52.
        _x("xmin_0.16", 0.16, a(15), (8, 15), 16),
        _x("xmax_0.16", a(-16), 0.16, (-16, 8), 48),                     # block 1 would need xmax >= 15
        _x("xmin_-0.16", -0.16, a(15), (-8, 15), 48),
        _x("xmax_0.32", a(-16), 0.32, (-16, 16), 64),
        _x("xmax_1.06", a(-16), 1.06, (-16, 52), 64),
        # inverted, one block, no whole block, an empty region
        _x("inverted", a(15), a(-16), (15, -16), 0),
        Case("inverted_z_only", voxel_box(ALL, ALL, (15, -16)), ALL + ALL + (15, -16), 0),
        Case("one_block", voxel_box((-8, -1), (0, 7), (-16, -9)), (-8, -1, 0, 7, -16, -9), 1),
        Case("one_block_loose", voxel_box((-15, 6), (-7, 14), (-16, -2)), (-15, 6, -7, 14, -16, -2), 1),   # (-1, 0, -2)
        Case("no_whole_block", voxel_box((-7, 6), (-15, 14), (1, 14)), (-7, 6, -15, 14, 1, 14), 0),
        Case("seven_voxels_wide", voxel_box((0, 6), ALL, ALL), (0, 6) + ALL + ALL, 0),
        Case("empty_region", voxel_box((800, 1200), (800, 1200), (-1200, -800)), (800, 1200, 800, 1200, -1200, -800), 0),
        # the whole int16 range, given as products: float32(-655.36) * 50 is exactly -32768, float32(655.34) * 50 is
        # 32767.002 -> 32767
        Case("int16_range", (-32768 * VS, 32767 * VS) * 3, (-32768, 32767) * 3, 64),
        # beyond the int16 range the low 16 bits remain: 40000 -> -25536 and -40000 -> 25536 (inverted: nothing),
        # 65551 -> 15 and -65552 -> -16 (everything)
        _x("wrap_40000", a(-40000), a(40000), (25536, -25536), 0),
        _x("wrap_onto_the_map", a(-65552), a(65551), (-16, 15), 64),
        _x("wrap_xmax_65543", a(-16), a(65543), (-16, 7), 48),
        # a caller's "everything": 5e10 saturates at INT_MAX, whose low 16 bits are -1, -5e10 at INT_MIN: 0
        Case("1e9_box", (-1e9, 1e9) * 3, (0, -1) * 3, 0),
        _x("1e9_in_x_only", -1e9, 1e9, (0, -1), 0),
        # NaN -> 0, +inf -> INT_MAX -> -1, -inf -> INT_MIN -> 0, in single members
        _x("xmin_nan", NAN, a(15), (0, 15), 32),
        _x("xmax_nan", a(-16), NAN, (-16, 0), 32),
        _x("xmax_inf", a(-16), INF, (-16, -1), 32),                      # blocks -2, -1: g + 7 <= -1
        _x("xmin_-inf", -INF, a(15), (0, 15), 32),
        _x("xmin_inf", INF, a(15), (-1, 15), 32),                        # g >= -1: blocks 0, 1
        _x("xmax_-inf", a(-16), -INF, (-16, 0), 32),
        Case("ymax_inf_zmin_nan", (a(-16), a(15), a(-16), INF, NAN, a(15)),
             ALL + (-16, -1) + (0, 15), 16),                             # y-blocks -2, -1 and z-blocks 0, 1: 4 * 2 * 2
    ]


def edges_cases():
    """the eight blocks of `edges`; the box of the other two axes is voxels 0 .. 7 unless stated"""
    lo, hi, zero = (-32768, -32761), (32760, 32767), (0, 7)
    full = (-32768, 32767)
    return [
        Case("everything", voxel_box(full, full, full), full * 3, 8),
        Case("x_4095_alone", voxel_box(hi, zero, zero), hi + zero + zero, 1),
        Case("y_4095_alone", voxel_box(zero, hi, zero), zero + hi + zero, 1),
        Case("z_4095_alone", voxel_box(zero, zero, hi), zero + zero + hi, 1),
        Case("y_-4096_alone", voxel_box(zero, lo, zero), zero + lo + zero, 1),
        Case("z_-4096_alone", voxel_box(zero, zero, lo), zero + zero + lo, 1),
        # block 4096's g is (short)32768 = -32768: it is taken through the low end of the range, with block -4096
        Case("x_low_end_takes_4096_too", voxel_box(lo, zero, zero), lo + zero + zero, 2),
        Case("x_4095_one_short", voxel_box((32760, 32766), zero, zero), (32760, 32766) + zero + zero, 0),
        Case("x_-4096_one_inside", voxel_box((-32767, -32761), zero, zero), (-32767, -32761) + zero + zero, 0),
        # g + 7 is evaluated in int: xmax = 32767 takes block 4095 (32760 + 7), and not by a sum that wrapped
        Case("x_upper_half", voxel_box((1, 32767), zero, zero), (1, 32767) + zero + zero, 1),
        Case("x_lower_half", voxel_box((-32768, -1), zero, zero), (-32768, -1) + zero + zero, 2),
        Case("origin_alone", voxel_box(zero, zero, zero), zero * 3, 1),
        Case("1e9_box", (-1e9, 1e9) * 3, (0, -1) * 3, 0),
    ]


def cases_of(m):
    return {"signs": signs_cases, "edges": edges_cases}[m.name]()


# ---------------------------------------------------------------------------------------------------------------------
# what the tests assert, for the oracle and the engine alike
def assert_same(got, want, what):
    assert same_bytes(got, want), f"{what}: {first_difference(got, want)}"


def directory_of(e, m):
    """dump_directory() of an engine that holds the map `m`, checked for what the restatement relies on: entry
    indices ascend, and the blocks are the map's, each once"""
    ei, bl = e.dump_directory()
    b = m.blocks if isinstance(m, Map) else m
    assert len(ei) == len(b) and (np.diff(ei.astype(np.int64)) > 0).all()
    assert np.array_equal(np.sort(block_keys(directory_positions(bl))), np.sort(block_keys(b.pos)))
    return ei, bl


def check_query(e, blocks, case, directory, what, vs=VS):
    """ratsdf_query of `case` against the restatement; returns the number of records"""
    gb = grid_bounds(case.bounds, vs)
    got = e.query(case.bounds)
    assert_same(got, expected(blocks, directory[0], directory[1], False, gb, vs), f"{what}: query {case.name}")
    return len(got)


def check_gathers(e, blocks, directory, path, what, vs=VS):
    """gather_valid, gather_valid_semantic and the download_all file (written to `path`) against the restatement"""
    want16 = expected(blocks, directory[0], directory[1], False, None, vs)
    want20 = expected(blocks, directory[0], directory[1], True, None, vs)
    assert_same(e.gather_valid(), want16, f"{what}: gather_valid")
    sem = e.gather_valid_semantic()
    assert_same(sem, want20, f"{what}: gather_valid_semantic")
    e.download_all(path)
    data = np.fromfile(path, dtype=np.uint8)
    assert np.array_equal(data, want20.view(np.uint8)), f"{what}: the download_all file"
    assert np.array_equal(data, sem.view(np.uint8)), f"{what}: the file is not gather_valid_semantic's bytes"
