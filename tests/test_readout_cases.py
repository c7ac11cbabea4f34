"""The crafted point-sampling / ESDF / surface cases (tests/readout_cases.py) without a GPU: the two independent
restatements of the map agree (the BlockSet the map was written from, and the CPU oracle that loaded it), the field
restatement agrees with the O(n^2) definition and with closed forms, the maps are what they claim, and every wrong
variant of the contract the cases are meant to catch is caught by its named set, by a stated minimum of records."""
import numpy as np
import pytest

import esdf_ref
import query_cases as qc
import readout_cases as rc
import sample_ref
import surface_ref
from kat_cases import ref_hash
from ratsdf._abi import SAMPLE_ALLOCATED, SAMPLE_NEAREST

F = np.float32


def _oracle_with(make_oracle, m):
    e = make_oracle(rc.VS, rc.TRUNC, **m.engine)
    rc.load(e, m)
    return e


def _wrong_samples(name, look=None, perm=None, **kw):
    ps = rc.point_set(name)
    with np.errstate(invalid="ignore", over="ignore"):
        return sample_ref.sample(ps.points, rc.VS, rc.blockset_lookup(ps.map.blocks, look=look, perm=perm), **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the two restatements of the map agree
@pytest.mark.parametrize("name", rc.SAMPLE_MAPS)
def test_blockset_lookup_is_the_oracles(name, make_oracle):
    m = rc.get_map(name)
    e = _oracle_with(make_oracle, m)
    sets = [ps for ps in rc.point_sets() if ps.map.name == m.name]
    assert sets
    for ps in sets:
        with np.errstate(invalid="ignore", over="ignore"):
            want = sample_ref.sample(ps.points, rc.VS, sample_ref.oracle_lookup(e))
        assert sample_ref.same_bytes(rc.expected_samples(ps.name), want), ps.name


@pytest.mark.parametrize("name", rc.ESDF_MAPS)
def test_box_state_is_the_oracles(name, make_oracle):
    m = rc.get_map(name)
    e = _oracle_with(make_oracle, m)
    mine = [b for b in rc.boxes() if b.map == m.name]
    assert mine
    for b in mine:
        want = esdf_ref.box_state(e, b.origin, b.dims, b.occupied_below)
        assert esdf_ref.same_bytes(rc.expected_state(b.name), want), b.name


# ---------------------------------------------------------------------------------------------------------------------
# the field restatement
def test_edt_is_the_definition_on_the_small_boxes():
    small = [b for b in rc.boxes() if b.voxels <= 1100]
    assert len(small) >= 40 and {b.map for b in small} >= {"esdf_lines", "edges", "known_order", "esdf_random"}
    # the random box's corner brings rows and columns without any obstacle beside ones with some to the definition
    o = esdf_ref.obstacles(rc.expected_state("random_crop_obs"))
    for lines in (o.any(axis=2), o.any(axis=1), o.any(axis=0)):
        assert 0.1 * lines.size < lines.sum() < 0.9 * lines.size
    assert sum(int(not o[z].any()) for z in range(o.shape[0])) == 2 and 30 <= o.sum() <= 300
    for b in small:
        o = esdf_ref.obstacles(rc.expected_state(b.name), b.unknown_occupied)
        for targets in (o, ~o):
            a, d = esdf_ref.edt_d2(targets), esdf_ref.brute_d2(targets)
            assert (a is None and d is None) or np.array_equal(a, d), b.name


def test_lines_slabs_and_the_plane_by_hand():
    by_hand = [b for b in rc.boxes() if b.by_hand is not None]
    assert len(by_hand) == 3 * len(rc.LINE_X) + 6 * len(rc.LINE_YZ) + 1 + 4
    for b in by_hand:
        assert esdf_ref.same_bytes(rc.expected_field(b.name), b.by_hand()), b.name
    vs = F(rc.VS)
    # the closed forms themselves, at a few voxels written out
    f = rc.expected_field("x1024_last")[0, 0]
    assert f[0] == F(1023) * vs and f[1022] == vs and f[1023] == -vs          # sqrtf(k^2) is k; the obstacle: -1 voxel
    f = rc.expected_field("x129_both")[0, 0]
    assert f[64] == F(64) * vs and f[63] == F(63) * vs and f[65] == F(63) * vs and f[0] == f[128] == -vs
    assert rc.expected_field("x1_first")[0, 0, 0] == -np.inf and (rc.expected_field("x2_both") == -np.inf).all()
    assert rc.expected_field("x2_first")[0, 0].tolist() == [-vs, vs]
    f = rc.expected_field("slab_y_one_free")
    assert f[6, 700, 2] == vs and f[6, 0, 2] == -(F(700) * vs) and f[6, 1023, 2] == -(F(323) * vs)
    assert f[0, 700, 7] == -(np.sqrt(F(36 + 25)) * vs)
    assert (rc.expected_field("slab_z_all_occupied") == -np.inf).all()
    f = rc.expected_field("plane_1024")[0]
    assert f[1023, 1023] == np.sqrt(F(2 * 511 ** 2)) * vs and f[0, 1023] == np.sqrt(F(512 ** 2 + 511 ** 2)) * vs
    assert f[0, 0] == f[512, 512] == -vs and f[0, 255] == F(255) * vs


def test_the_esdf_boxes_hold_what_the_issue_lists():
    names = {b.name for b in rc.boxes()}
    for n in rc.LINE_X:
        assert {f"x{n}_first", f"x{n}_last", f"x{n}_both"} <= names
    assert max(b.voxels for b in rc.boxes()) == 1 << 20
    for b in rc.boxes():
        o, d = np.array(b.origin), np.array(b.dims)
        assert (d >= 1).all() and (d <= 1024).all() and (o >= -32768).all() and (o + d - 1 <= 32767).all(), b.name
    r = rc.box("random_rank_12_obs")
    assert (r.dims[0] * r.dims[2]) % 64 and (r.dims[0] * r.dims[1]) % 64 and r.dims[0] * r.dims[2] > 64
    # lines with no obstacle beside lines with some, in every pass: whole planes and rows of the box are free
    for name in (n for n in sorted(names) if n.startswith("random_rank") and n.endswith("_obs")):
        o = esdf_ref.obstacles(rc.expected_state(name))
        rows, cols_y = o.any(axis=2), o.any(axis=1)
        assert 0 < rows.sum() < rows.size and 0 < cols_y.sum() < cols_y.size
        assert not o[list(rc.RANDOM_FREE_PLANES_Z)].any() and not o[:, rc.RANDOM_FREE_PLANE_Y].any()
        assert not any(o[z, y].any() for y, z in rc.RANDOM_FREE_ROWS_YZ)
    few = esdf_ref.obstacles(rc.expected_state("random_rank_12_obs"))
    assert 1 <= few.sum() <= rc.RANDOM_HANDFUL
    s = rc.expected_state("random_all_but_a_handful_unk")
    assert (s == esdf_ref.FREE).sum() == rc.RANDOM_HANDFUL and (s == esdf_ref.UNKNOWN).sum() > 1000   # absent, weight 0
    assert (~esdf_ref.obstacles(s, True)).sum() == rc.RANDOM_HANDFUL
    # every state occurs at the range ends, and block -4096 is the one at voxel -32768
    s = rc.expected_state("edge_x_low_16")
    assert (s[:, :, 8:] == esdf_ref.UNKNOWN).all() and len(np.unique(s[:, :, :8])) == 3
    e = rc.edges().blocks
    lo, hi = e.pos.tolist().index([-4096, 0, 0]), e.pos.tolist().index([4096, 0, 0])
    st = lambda row: np.where(e.rgbw["weight"][row] == 0, 0, np.where(e.tsdf[row] <= 0, 2, 1)).reshape(8, 8, 8)
    assert np.array_equal(s[:, :, :8], st(lo)) and (s[:, :, :8] != st(hi)).sum() > 100


# ---------------------------------------------------------------------------------------------------------------------
# the maps are what they claim
def _chains(ei, bl, num_entry):
    """the entry chains of a directory dump: {head entry: [entries walked from it]} by the offsets"""
    offset = {int(k): int(o) for k, o in zip(ei, bl["offset"])}
    chains = {}
    for head in (k for k in offset if k & 1):
        walk, at = [head], head
        while offset.get(at, 0):
            at = (at + offset[at]) & (num_entry - 1)
            assert at in offset and at not in walk
            walk.append(at)
        chains[head] = walk
    return chains


def test_tiny_table_has_full_buckets_and_chains(make_oracle):
    m = rc.tiny_table()
    e = _oracle_with(make_oracle, m)
    ei, bl = e.dump_directory()
    taken = set(int(k) for k in ei)
    full = [h for h in range(1 << m.engine["bucket_bits"]) if {2 * h, 2 * h + 1} <= taken]
    assert len(full) >= 20
    chains = _chains(ei, bl, 2 << m.engine["bucket_bits"])
    assert max(len(c) for c in chains.values()) >= 3
    home = np.array([ref_hash(p, m.engine["bucket_bits"]) for p in qc.directory_positions(bl)])
    assert ((ei >> 1) != home).sum() >= 20                          # blocks only a chain walk finds


def test_known_order_wraps_at_the_end_of_the_table(make_oracle):
    m = rc.known_order()
    e = _oracle_with(make_oracle, m)
    ei, bl = e.dump_directory()
    table = qc.known_order_entries()
    assert {int(k): tuple(int(v) for v in p) for k, p in zip(ei, qc.directory_positions(bl))} == table
    chains = _chains(ei, bl, qc.LAST)
    assert chains[qc.LAST - 1] == [qc.LAST - 1, 2]                  # the walk leaves the table's end and wraps to entry 2
    # the points of the wrapped block are in the sets, allocated
    for name in ("known_order_integer", "known_order_jitter"):
        cell = rc.cell_of(rc.point_set(name).points)
        inside = np.all((cell >> 3) == np.array(table[2]), axis=1) & np.all((cell & 7) < 7, axis=1)
        assert inside.sum() >= 100 and (rc.expected_samples(name)["flags"][inside] & SAMPLE_ALLOCATED).all()


def test_corner_subsets_has_every_subset_once():
    m = rc.corner_subsets()
    assert len(m.blocks) == 1024 <= 1 << m.engine["block_bits"]
    rel = m.blocks.pos.astype(np.int64) - np.array(rc.CLUSTER_BASE)
    cell, corner = rel // rc.CLUSTER_STEP, rel % rc.CLUSTER_STEP
    assert (corner <= 1).all() and (cell >= 0).all() and (cell < np.array(rc.CLUSTER_GRID)).all()
    cluster = (cell[:, 0] << 5) | (cell[:, 1] << 2) | cell[:, 2]
    subset = np.zeros(256, dtype=np.int64)
    np.add.at(subset, cluster, 1 << ((corner[:, 0] << 2) | (corner[:, 1] << 1) | corner[:, 2]))
    assert subset.tolist() == list(range(256))                      # cluster s holds subset s: each exactly once
    assert (m.blocks.pos < 0).any(axis=0).all() and (m.blocks.pos > 0).any(axis=0).all()
    # the set visits, per cluster, the 19 straddling cells at 8 fractions; the nearest voxel takes every corner
    ps = rc.point_set("corner_subsets")
    assert len(ps.points) == 256 * 19 * 8
    cell = rc.cell_of(ps.points)
    assert sorted(np.unique(((cell & 7) == 7).sum(axis=1), return_counts=True)[1].tolist()) == [256 * 8, 256 * 48, 256 * 96]
    want = rc.expected_samples("corner_subsets")
    alloc = (want["flags"] & SAMPLE_ALLOCATED) != 0
    near = (want["flags"] & SAMPLE_NEAREST) != 0
    assert alloc.sum() > 1000 and (near & ~alloc).sum() > 5000 and (~near).sum() > 5000


def test_point_sets_hold_what_the_issue_lists():
    sets = {ps.name: ps for ps in rc.point_sets()}
    assert 20000 <= len(sets["corner_subsets"].points) <= 60000 and max(rc.BATCH_LENGTHS) < 20000
    vs = F(rc.VS)
    for name in ("signs_integer", "signs_halves", "signs_odd"):
        assert not rc.touches_special(rc.signs(), sets[name].points).any()
    assert rc.touches_special(rc.signs(), sets["specials"].points).all()
    g = sets["signs_halves"].points / vs
    assert (g - np.floor(g) == F(0.5)).all() and {-2.5, 2.5, -0.5, 0.5} <= set(np.unique(g).tolist())
    g = sets["signs_integer"].points / vs
    assert g.min() == -17 and g.max() == 16 and (g == np.floor(g)).mean() > 0.6
    p = sets["signs_odd"].points
    g = p / vs
    assert (p.view(np.uint32) == 0x80000000).any() and (p.view(np.uint32) == 1).any()      # -0.0, a denormal
    assert (p.view(np.uint32) == 0x80000001).any()                                        # a negative one: floor -1
    for i in (-16, -8, 1, 8):
        assert (g == np.nextafter(F(i), F(np.inf))).any() or (g == np.nextafter(F(i), F(-np.inf))).any()
    assert sum(int((g == np.nextafter(F(i), F(s))).any()) for i in (-16, -9, -8, -1, 1, 7, 8, 15)
               for s in (-np.inf, np.inf)) >= 8
    # the range ends: every cell inside is allocated, every cell one voxel further out is all defaults
    cell = rc.cell_of(sets["edges_inside"].points)
    for a in range(3):
        assert ((cell[:, a] == 32766).sum() >= 100) and ((cell[:, a] == -32768).sum() >= 100)
    assert ((rc.expected_samples("edges_inside")["flags"] & SAMPLE_ALLOCATED) != 0).all()
    out = rc.expected_samples("edges_outside")
    assert (out["flags"] == 0).all() and (out["tsdf"].view(np.uint32) == 0x7FC00000).all() and (out["prob"] == 0).all()
    cell = rc.cell_of(sets["edges_outside"].points)
    assert set(np.unique(cell.max(axis=1))) >= {32767} and set(np.unique(cell.min(axis=1))) >= {-32769}
    # voxel -32768 shows block -4096's probability (a function of the unwrapped coordinate), not block 4096's
    pts, want = sets["edges_inside"].points, rc.expected_samples("edges_inside")
    cell = rc.cell_of(pts)
    low = (cell[:, 0] == -32768) & ((pts / vs - cell)[:, 0] < 0.5)
    near = cell[low] + ((pts[low] / vs - cell[low]) >= 0.5)
    assert low.sum() >= 50 and np.array_equal(want["prob"][low], qc.prob_of(near))
    assert (want["prob"][low] != qc.prob_of(near + np.array([65536, 0, 0]))).all()


def test_nan_records_stay_inside_their_bound():
    """records whose tsdf or gradient is NaN while ALLOCATED is set (compared as "is NaN", not as bits): in the
    specials set only, and in at most a tenth of it"""
    for ps in rc.point_sets():
        nan = rc.nan_components(rc.expected_samples(ps.name)).any(axis=1)
        if ps.name == "specials":
            assert ps.nan_allowed and 0 < nan.sum() <= 0.1 * len(nan)
        else:
            assert not ps.nan_allowed and not nan.any(), ps.name
    # the rule itself: bits of such components are free, everything else is not
    want = rc.expected_samples("specials")
    got = want.copy()
    i = int(np.flatnonzero(rc.nan_components(want)[:, 0])[0])
    got["tsdf"].view(np.uint32)[i] = 0xFFC00001
    rc.assert_samples(got, want, "another NaN", nan_allowed=True)
    with pytest.raises(AssertionError):
        rc.assert_samples(got, want, "another NaN", nan_allowed=False)
    got["tsdf"][i] = 1.0
    with pytest.raises(AssertionError):
        rc.assert_samples(got, want, "a number for a NaN", nan_allowed=True)
    got = want.copy()
    j = int(np.flatnonzero((want["flags"] & SAMPLE_ALLOCATED) == 0)[0])
    got["tsdf"].view(np.uint32)[j] = 0xFFC00000                       # the default NaN is compared as bits
    with pytest.raises(AssertionError):
        rc.assert_samples(got, want, "default", nan_allowed=True)


# ---------------------------------------------------------------------------------------------------------------------
# the cases discriminate: each wrong variant differs from the contract on at least `least` records of its set
def test_mirrored_pairing_is_caught():
    """at an integer point the mirrored pairing returns the voxel one step up every axis: nearly every allocated
    record of signs_integer, whose voxels all differ"""
    ps = rc.point_set("signs_integer")
    alloc = int(((rc.expected_samples(ps.name)["flags"] & SAMPLE_ALLOCATED) != 0).sum())
    assert alloc > 30000 and rc.differing(rc.mirrored_samples(ps), rc.expected_samples(ps.name)) >= 0.9 * alloc


@pytest.mark.parametrize("perm", rc.PERMUTATIONS)
def test_permuted_corner_map_is_caught(perm):
    """a transposition of two axes leaves 64 of the 256 subsets as they are; in each of the other 192 clusters the
    all-7 cell alone has 8 records: 1536.  (The cells with 7 on two axes add more.)"""
    assert rc.differing(_wrong_samples("corner_subsets", perm=perm), rc.expected_samples("corner_subsets")) >= 1536


def test_round_half_even_is_caught():
    """per axis half of the exact halves have an even floor on the side where half-even and half-away part: at least
    a quarter of the records of signs_halves"""
    n = len(rc.point_set("signs_halves").points)
    assert rc.differing(_wrong_samples("signs_halves", nearest=np.rint), rc.expected_samples("signs_halves")) >= n // 4
    assert rc.differing(_wrong_samples("signs_odd", nearest=np.rint), rc.expected_samples("signs_odd")) >= 1000


def test_trunc_for_floor_is_caught():
    """trunc is floor + 1 on every negative non-integer coordinate: seven in eight triples of halves have one"""
    n = len(rc.point_set("signs_halves").points)
    assert rc.differing(_wrong_samples("signs_halves", floor=np.trunc), rc.expected_samples("signs_halves")) >= n // 2
    assert rc.differing(_wrong_samples("signs_odd", floor=np.trunc), rc.expected_samples("signs_odd")) >= 1000


def test_missing_range_guard_is_caught():
    """one voxel beyond either end the far corner wraps onto the block at the other end, which `edges` holds: every
    record of edges_outside becomes ALLOCATED"""
    n = len(rc.point_set("edges_outside").points)
    wrong = _wrong_samples("edges_outside", guard=False)
    assert rc.differing(wrong, rc.expected_samples("edges_outside")) == n and (wrong["flags"] & SAMPLE_ALLOCATED).all()


def test_block_4096_for_voxel_minus_32768_is_caught():
    ps = rc.point_set("edges_inside")
    low = int((rc.cell_of(ps.points)[:, 0] == -32768).sum())
    wrong = _wrong_samples("edges_inside", look=rc.WrappedLookup(ps.map.blocks))
    assert low >= 100 and rc.differing(wrong, rc.expected_samples("edges_inside")) == low


@pytest.mark.parametrize("variant,least", [("less_than", 5), ("denormals_flushed", 4), ("nan_occupied", 12)])
def test_wrong_state_comparisons_are_caught(variant, least):
    """over the six thresholds on signs_weighted.  `<`: the voxel that equals the threshold (-0.0 twice, the denormal,
    +inf, -inf).  Flushing: the positive denormal at 0 and -0, and -0.0 and the negative denormal's neighbour at the
    negative denormal threshold.  NaN: the two NaN voxels at every threshold."""
    total = 0
    for b in (b for b in rc.boxes() if b.map == "signs_weighted" and not b.unknown_occupied):
        wrong = rc.box_state(rc.get_map(b.map).blocks, b.origin, b.dims, b.occupied_below,
                             occupied=rc.WRONG_STATES[variant])
        total += int((wrong != rc.expected_state(b.name)).sum())
    assert total >= least


# ---------------------------------------------------------------------------------------------------------------------
# surface points
def test_surface_boxes_have_points_and_no_special_voxel(make_oracle):
    for name, map_name, origin, dims, least in rc.SURFACE_BOXES:
        m = rc.get_map(map_name)
        sp = rc.special_voxels(m)
        lo, hi = np.array(origin) - 1, np.array(origin) + np.array(dims) + 1      # what the box's owners read
        assert not np.all((sp >= lo) & (sp <= hi), axis=1).any(), name
        pts = surface_ref.surface_points(surface_ref.blocks_of(*m.blocks), origin, dims, rc.VS)
        assert len(pts) >= least and np.isfinite(pts["pos"]).all() and np.isfinite(pts["normal"]).all(), name
    # what makes them boxes on CHAINED directories: the oracle's directory (the engine's is checked equal to the table
    # in the GPU file) has block (63, 171, 45) at entry 2, reached from its home bucket 2^21 - 1 across the table's end,
    # and tiny_table's box holds blocks that lie outside their home bucket
    boxes = {b[0]: b for b in rc.SURFACE_BOXES}
    inside = lambda b, pos: np.all((pos * 8 + 7 >= np.array(b[2])) & (pos * 8 < np.array(b[2]) + np.array(b[3])), axis=1)
    table = qc.known_order_entries()
    assert table[2] == (63, 171, 45) and ref_hash(table[2]) == qc.NUM_BUCKET - 1
    assert inside(boxes["known_order_63_171_45"], np.array([table[2]]))[0]
    assert inside(boxes["known_order_33_180_42"], np.array([table[qc.LAST - 2]]))[0]
    m = rc.tiny_table()
    e = _oracle_with(make_oracle, m)
    ei, bl = e.dump_directory()
    pos = qc.directory_positions(bl)
    home = np.array([ref_hash(p, m.engine["bucket_bits"]) for p in pos])
    assert (((ei >> 1) != home) & inside(boxes["tiny_table"], pos)).sum() >= 10
