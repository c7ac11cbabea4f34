"""The crafted query / gather cases (tests/query_cases.py) on the CPU oracle alone, no GPU: the builders' self-checks,
the hand-stated grid bounds, block counts and entry indices, and the oracle's four read-outs against the numpy
restatement, byte for byte.  The oracle runs every size of query_cases.SIZES, 4097 blocks included."""
import numpy as np
import pytest

import query_cases as qc
from kat_cases import ref_hash

F = np.float32


def _oracle_with(make_oracle, m):
    e = make_oracle(qc.VS, qc.TRUNC, **m.engine)
    qc.load(e, m)
    return e


def _bits(x):
    return int(np.asarray(x, dtype=F).view(np.uint32))


def test_maps_are_what_they_say():
    for m in qc.maps() + [qc.sizes(n) for n in qc.SIZES]:
        b = m.blocks
        assert b.pos.dtype == np.int16 and b.tsdf.dtype == F and b.prob.dtype == F
        assert b.tsdf.shape == b.rgbw.shape == b.prob.shape == (len(b), 512) and b.pos.shape == (len(b), 3)
        assert len(np.unique(qc.block_keys(b.pos))) == len(b)
        assert len(b) <= 1 << m.engine["block_bits"]
        assert (b.rgbw["weight"] == 0).any() and (b.rgbw["weight"] > 0).any()
        # the special values, once per map: everything else is finite and normal
        odd = ~np.isfinite(b.tsdf) | ((np.abs(b.tsdf) < np.finfo(F).tiny) & (b.tsdf.view(np.uint32) != 0))
        assert int(odd.sum()) == len(qc.SPECIAL_TSDF) and len(np.unique(np.nonzero(odd)[0])) == 1
        row = int(np.nonzero(odd)[0][0])
        for slot, bits in qc.SPECIAL_TSDF.items():
            assert int(b.tsdf.view(np.uint32)[row, slot]) == bits
        for slot, bits in qc.SPECIAL_PROB.items():
            assert int(b.prob.view(np.uint32)[row, slot]) == bits
    assert [len(qc.sizes(n).blocks) for n in qc.SIZES] == list(qc.SIZES)
    assert len(qc.signs().blocks) == 64 and len(qc.edges().blocks) == 8 and len(qc.tiny_table().blocks) == 200
    assert len({tuple(s) for s in (qc.signs().blocks.pos < 0)}) == 8
    # different voxels hold different values: tsdf alone tells the voxels of a map apart (but for a few coincidences)
    for m in (qc.signs(), qc.tiny_table(), qc.sizes(513)):
        t = m.blocks.tsdf[np.isfinite(m.blocks.tsdf)]
        assert len(np.unique(t)) > 0.98 * t.size
    # blocks 4096 and -4096 share their wrapped voxel coordinates and differ in every value
    e = qc.edges().blocks
    hi, lo = e.pos.tolist().index([4096, 0, 0]), e.pos.tolist().index([-4096, 0, 0])
    assert (e.tsdf[hi] != e.tsdf[lo]).all()


def test_a_voxel_by_hand():
    """block (-1, 2, 0) of tiny_table, local (7, 0, 3) = voxel (-1, 16, 3), slot 7 + 0 + 3 * 64 = 199"""
    b = qc.tiny_table().blocks
    row = b.pos.tolist().index([-1, 2, 0])
    k = (-73856093 + 16 * 19349669 + 3 * 83492791) % 16777213       # 486216984 - 28 * 16777213
    assert k == 16455020
    assert b.tsdf[row, 199] == F((16455020 - 8388608) / 8388608)
    assert b.prob[row, 199] == F(((-7 + 13 * 16 + 17 * 3) % 1021) / 1024) == F(252 / 1024)
    assert tuple(b.rgbw[row, 199]) == ((37 * -1) & 255, (59 * 16) & 255, (83 * 3) & 255, (-1 + 48 + 15) & 3)
    # its record: voxel -1 lies at float32(-1) * float32(0.02)
    r = qc.records([[-1, 2, 0]], [5], b.tsdf[row:row + 1], b.prob[row:row + 1], qc.VS, True)
    assert len(r) == 512 and r.dtype.itemsize == 20
    assert (r["x"][199], r["y"][199], r["z"][199]) == (F(-1) * F(0.02), F(16) * F(0.02), F(3) * F(0.02))
    assert r["tsdf"][199] == b.tsdf[row, 199] and r["prob"][199] == b.prob[row, 199]
    assert (r["x"][0], r["x"][1], r["y"][8], r["z"][64]) == (F(-8) * F(0.02), F(-7) * F(0.02), F(17) * F(0.02), F(0.02))


def test_conversion_by_hand():
    f2s = lambda v: int(qc.float_to_short(F(v)))
    assert [f2s(v) for v in (7.99, -7.99, -7.5, -8.9, 0.5, -0.5, 32767.9, -32768.9)] == \
        [7, -7, -7, -8, 0, 0, 32767, -32768]
    assert [f2s(v) for v in (40000.0, -40000.0, 65536.0, 2.0 ** 31, -2.0 ** 31, 5e10, -5e10, 2.0 ** 31 - 128)] == \
        [40000 - 65536, 65536 - 40000, 0, -1, 0, -1, 0, -128]
    assert [f2s(v) for v in (np.nan, np.inf, -np.inf)] == [0, -1, 0]
    # 2 cm voxels: the scale is exactly 50; 0.16f * 50 rounds to the float32 8.0, 1.06f * 50 stays below 53
    assert F(1.0 / float(F(0.02))) == F(50)
    assert F(0.16) * F(50) == F(8) and F(1.06) * F(50) < F(53)
    assert qc.grid_bounds((0.16, -0.16, 0.32, 1.06, -1e9, 1e9), 0.02) == (8, -8, 16, 52, 0, -1)
    # the records' wrapped coordinates: block 4096 holds voxels -32768 .. -32761
    r = qc.records([[4096, 4095, -4096]], [0], np.zeros((1, 512), F), np.zeros((1, 512), F), qc.VS, False)
    assert r["x"][0] == F(-32768) * F(0.02) and r["x"][7] == F(-32761) * F(0.02)
    assert r["y"][511] == F(32767) * F(0.02) and r["z"][0] == F(-32768) * F(0.02)
    # and the containment test on them, in wide integers
    sel = lambda b, gb: bool(qc.select([b], gb)[0])
    assert sel((4095, 0, 0), (32760, 32767, 0, 7, 0, 7)) and not sel((4095, 0, 0), (32760, 32766, 0, 7, 0, 7))
    assert sel((4096, 0, 0), (-32768, -32761, 0, 7, 0, 7)) and not sel((4096, 0, 0), (32760, 32767, 0, 7, 0, 7))


@pytest.mark.parametrize("m", [qc.signs(), qc.edges()], ids=lambda m: m.name)
def test_bounds_cases_state_their_grid_and_count(m):
    cases = qc.cases_of(m)
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert qc.grid_bounds(c.bounds, qc.VS) == c.grid, c.name
        assert int(qc.select(m.blocks.pos, c.grid).sum()) == c.count, c.name
    full = [c for c in cases if c.count > 0]
    assert len(full) > len(cases) - len(full) > 0          # more cases select something than select nothing


def test_known_order_entries_agree_with_the_oracle(make_oracle, tmp_path):
    m = qc.known_order()
    table = qc.known_order_entries()
    assert sorted(table)[0] == 0 and sorted(table)[1] == 2 and sorted(table)[-2:] == [qc.LAST - 2, qc.LAST - 1]
    assert {(k >> 6) for k in table} >= {0, (qc.LAST >> 6) - 1}             # the first and the last occupancy word
    assert all(k == 2 * ref_hash(p) for k, p in table.items() if p in qc.APART)
    e = _oracle_with(make_oracle, m)
    ei, bl = e.dump_directory()
    assert {int(k): tuple(int(v) for v in p) for k, p in zip(ei, qc.directory_positions(bl))} == table
    assert all(int(o) == (3 if int(k) == qc.LAST - 1 else 0) for k, o in zip(ei, bl["offset"]))
    # the read-outs in that order, the order taken from the hand-written table alone
    order = sorted(table)
    qc.check_gathers(e, m.blocks, (order, [table[k] for k in order]), tmp_path / "all.bin", m.name)


@pytest.mark.parametrize("m", qc.maps(), ids=lambda m: m.name)
def test_oracle_gathers(m, make_oracle, tmp_path):
    e = _oracle_with(make_oracle, m)
    qc.check_gathers(e, m.blocks, qc.directory_of(e, m), tmp_path / "all.bin", m.name)


@pytest.mark.parametrize("m", [qc.signs(), qc.edges()], ids=lambda m: m.name)
def test_oracle_queries(m, make_oracle):
    e = _oracle_with(make_oracle, m)
    d = qc.directory_of(e, m)
    for c in qc.cases_of(m):
        assert qc.check_query(e, m.blocks, c, d, m.name) == 512 * c.count, c.name


def test_oracle_queries_on_the_chained_tables(make_oracle):
    """known_order and tiny_table under boxes that take some of their blocks"""
    for m, box, count in ((qc.known_order(), qc.voxel_box((-8, 15), (-24, 15), (-8, 15)), 5),
                          # (x-blocks -2 .. 1, y-blocks -3 .. 0, z-blocks -1 .. 2; the map lacks (-1, -2, 0) and (-1, -2, 1) of them)
                          (qc.tiny_table(), qc.voxel_box((-16, 15), (-24, 7), (-8, 23)), 4 * 4 * 4 - 2)):
        e = _oracle_with(make_oracle, m)
        c = qc.Case("box", box, qc.grid_bounds(box, qc.VS), count)
        assert int(qc.select(m.blocks.pos, c.grid).sum()) == count
        assert qc.check_query(e, m.blocks, c, qc.directory_of(e, m), m.name) == 512 * count


@pytest.mark.parametrize("n", qc.SIZES)
def test_oracle_sizes(n, make_oracle, tmp_path):
    m = qc.sizes(n)
    e = _oracle_with(make_oracle, m)
    d = qc.directory_of(e, m)
    qc.check_gathers(e, m.blocks, d, tmp_path / "all.bin", m.name)
    one, none = qc.sizes_one_block_box(n)
    full = qc.voxel_box((-32768, 32767), (24, 31), (-16, -9))
    for box, count in ((full, n), (one, 1), (none, 0)):
        c = qc.Case("box", box, qc.grid_bounds(box, qc.VS), count)
        assert qc.check_query(e, m.blocks, c, d, m.name) == 512 * count
