"""Point sampling, the ESDF and surface points of the HIP engine on the crafted maps, point sets and boxes of
tests/readout_cases.py, against restatements that never ask an engine: byte for byte, both entry points of each.  The
maps are imported, so the engine holds the very floats the restatements are fed, the probability included; they are
loaded into the maps' own small directories, so blocks are found by chain walks and across the table's end.  The one
tolerance is the NaN rule of readout_cases.assert_samples, for the `specials` set alone.
(tests/test_readout_cases.py shows without a GPU that the restatements agree with the CPU oracle and that the sets
catch the wrong variants they are meant for.)"""
import numpy as np
import pytest

import query_cases as qc
import readout_cases as rc
import surface_ref
from kat_cases import ref_hash
from ratsdf import devmem
from ratsdf._abi import SAMPLE_DTYPE

pytestmark = pytest.mark.gpu

def _engine_with(make_engine, m):
    e = make_engine(rc.VS, rc.TRUNC, **m.engine)
    rc.load(e, m)
    return e


def _sample_both(e, pts, want, what, nan_allowed=False):
    """ratsdf_sample_points and ratsdf_sample_points_device on the same points"""
    rc.assert_samples(e.sample_points(pts), want, f"{what}: sample_points", nan_allowed)
    d_xyz = devmem.DeviceArray(pts)
    d_out = devmem.DeviceArray(np.full(len(pts), 0xA5, dtype=np.uint8).repeat(32).view(SAMPLE_DTYPE))
    e.sample_points_device(d_xyz.data_ptr(), len(pts), d_out.data_ptr())
    e.synchronize()
    rc.assert_samples(d_out.numpy(), want, f"{what}: sample_points_device", nan_allowed)


@pytest.mark.parametrize("name", rc.SAMPLE_MAPS)
def test_point_sets(name, make_engine):
    m = rc.get_map(name)
    e = _engine_with(make_engine, m)
    ei, bl = qc.directory_of(e, m)
    if m.name == "tiny_table":      # blocks that only a chain walk finds
        home = np.array([ref_hash(p, m.engine["bucket_bits"]) for p in qc.directory_positions(bl)])
        assert ((ei >> 1) != home).sum() >= 20
    if m.name == "known_order":     # the chain that leaves the table's end and wraps to entry 2
        table = qc.known_order_entries()
        assert {int(k): tuple(int(v) for v in p) for k, p in zip(ei, qc.directory_positions(bl))} == table
    sets = [ps for ps in rc.point_sets() if ps.map.name == m.name]
    assert sets
    for ps in sets:
        _sample_both(e, ps.points, rc.expected_samples(ps.name), ps.name, ps.nan_allowed)


def test_batch_lengths(make_engine):
    """a single point, one short of a workgroup, a workgroup, one more: the head of the set, and a stretch from its
    middle (the records do not depend on their neighbours)"""
    ps = rc.point_set("corner_subsets")
    e = _engine_with(make_engine, ps.map)
    want = rc.expected_samples(ps.name)
    for n in rc.BATCH_LENGTHS:
        for at in (0, 20001):
            _sample_both(e, ps.points[at:at + n], want[at:at + n], f"{ps.name}[{at}:{at}+{n}]")


def _differ(got, want):
    """None, or where two arrays of a box differ as bytes"""
    a, b = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    if a.dtype != b.dtype or a.shape != b.shape:
        return f"{a.dtype}{got.shape} for {b.dtype}{want.shape}"
    bits = {1: np.uint8, 4: np.uint32}[a.dtype.itemsize]
    bad = np.flatnonzero(a.view(bits) != b.view(bits))
    if len(bad) == 0:
        return None
    z, y, x = np.unravel_index(int(bad[0]), want.shape)
    return f"{len(bad)} of {b.size} voxels differ, the first at box voxel ({x}, {y}, {z}): {a[bad[0]]} != {b[bad[0]]}"


def _check_box(e, b):
    """both entry points, each with and without the state output"""
    want, want_st = rc.expected_field(b.name), rc.expected_state(b.name)
    args = (b.origin, b.dims, b.occupied_below, b.unknown_occupied)
    got, st = e.esdf(*args, with_state=True)
    assert got.shape == want.shape and st.shape == want_st.shape and got.dtype == want.dtype and st.dtype == want_st.dtype
    assert _differ(st, want_st) is None, f"{b.name}: esdf state: {_differ(st, want_st)}"
    assert _differ(got, want) is None, f"{b.name}: esdf: {_differ(got, want)}"
    got = e.esdf(*args)
    assert _differ(got, want) is None, f"{b.name}: esdf without the states: {_differ(got, want)}"
    for with_state in (True, False):
        d_out = devmem.DeviceArray(np.full(want.shape, -7, dtype=np.float32))
        d_st = devmem.DeviceArray(np.full(want.shape, 9, dtype=np.uint8))
        e.esdf_device(b.origin, b.dims, d_out.data_ptr(), d_st.data_ptr() if with_state else 0, b.occupied_below,
                      b.unknown_occupied)
        e.synchronize()
        got, st = d_out.numpy(), d_st.numpy()
        assert _differ(got, want) is None, f"{b.name}: esdf_device (states: {with_state}): {_differ(got, want)}"
        if with_state:
            assert _differ(st, want_st) is None, f"{b.name}: esdf_device state: {_differ(st, want_st)}"
        else:
            assert (st == 9).all(), f"{b.name}: esdf_device wrote states it was not asked for"


@pytest.mark.parametrize("name", rc.ESDF_MAPS)
def test_esdf_boxes(name, make_engine):
    m = rc.get_map(name)
    e = _engine_with(make_engine, m)
    mine = [b for b in rc.boxes() if b.map == m.name]
    assert mine
    for b in mine:
        _check_box(e, b)


def test_small_boxes_after_the_largest(make_engine):
    """the workspace only grows and stays laid out for the 2^20 voxels it grew to: small boxes right after"""
    e = _engine_with(make_engine, rc.esdf_lines())
    for name in ("x2_first", "plane_1024", "x65_both", "x1_first", "y65_both", "z1024_last", "x1024_both"):
        _check_box(e, rc.box(name))


@pytest.mark.parametrize("name,map_name,origin,dims,least", rc.SURFACE_BOXES, ids=[s[0] for s in rc.SURFACE_BOXES])
def test_surface_points_on_the_chained_directories(name, map_name, origin, dims, least, make_engine):
    """tiny_table: blocks at the end of chains; known_order_63_171_45: the block behind the table-end wrap"""
    m = rc.get_map(map_name)
    e = _engine_with(make_engine, m)
    blocks = surface_ref.blocks_of(*m.blocks)
    for min_weight, min_prob in ((1, 0.0), (2, 0.25)):
        got = e.surface_points(origin, dims, min_weight, min_prob)
        want = surface_ref.surface_points(blocks, origin, dims, rc.VS, min_weight, min_prob)
        assert len(want) >= (least if min_weight == 1 else least // 4)
        assert surface_ref.same_bytes(got, want), (name, min_weight, min_prob, len(got), len(want))
