"""ratsdf_query, ratsdf_gather_valid, ratsdf_gather_valid_semantic and the ratsdf_download_all file of the HIP engine on
the crafted maps of tests/query_cases.py, against the numpy restatement of their contract: byte for byte, order
included, no tolerance -- the maps are imported, so the engine holds the very floats the restatement is fed.  The
directory the restatement orders the blocks by is the engine's own dump (checked against the CPU oracle's, which loads
the map the same way), and for `known_order` a table written by hand.  Only the carving case integrates frames: there the
probability, which the engine computes by another expression than the oracle, keeps the bar of tests/parity.py.
"""
import ctypes as C

import numpy as np
import pytest

import query_cases as qc
from parity import TOL, assert_directory_equal, assert_maps_equal
from ratsdf import synthetic
from ratsdf._abi import Bounds

pytestmark = pytest.mark.gpu


def _pair(make_engine, make_oracle, m):
    """the engine and the oracle, both holding the map; the engine's directory, equal to the oracle's"""
    gpu, cpu = make_engine(qc.VS, qc.TRUNC, **m.engine), make_oracle(qc.VS, qc.TRUNC, **m.engine)
    for e in (gpu, cpu):
        qc.load(e, m)
    assert_directory_equal(gpu, cpu)
    return gpu, cpu, qc.directory_of(gpu, m)


@pytest.mark.parametrize("m", qc.maps(), ids=lambda m: m.name)
def test_gathers(m, make_engine, make_oracle, tmp_path):
    gpu, _, d = _pair(make_engine, make_oracle, m)
    qc.check_gathers(gpu, m.blocks, d, tmp_path / "all.bin", m.name)


@pytest.mark.parametrize("m", [qc.signs(), qc.edges()], ids=lambda m: m.name)
def test_bounds_cases(m, make_engine, make_oracle):
    gpu, _, d = _pair(make_engine, make_oracle, m)
    for c in qc.cases_of(m):
        assert qc.check_query(gpu, m.blocks, c, d, m.name) == 512 * c.count, c.name


def test_known_order(make_engine, make_oracle, tmp_path):
    """entry 0, entry 2, the table's last two entries and five in between come out in the order written by hand"""
    m = qc.known_order()
    gpu, _, d = _pair(make_engine, make_oracle, m)
    table = qc.known_order_entries()
    order = sorted(table)
    assert [int(k) for k in d[0]] == order
    assert [tuple(int(v) for v in p) for p in qc.directory_positions(d[1])] == [table[k] for k in order]
    by_hand = (order, [table[k] for k in order])
    qc.check_gathers(gpu, m.blocks, by_hand, tmp_path / "all.bin", m.name)
    box = qc.voxel_box(*((-32768, 32767),) * 3)
    everything = qc.Case("everything", box, qc.grid_bounds(box, qc.VS), len(order))
    some = qc.voxel_box((-8, 15), (-24, 15), (-8, 15))           # the five blocks around the origin
    for c in (everything, qc.Case("around_the_origin", some, qc.grid_bounds(some, qc.VS), 5)):
        assert qc.check_query(gpu, m.blocks, c, by_hand, m.name) == 512 * c.count


def _size_boxes(n):
    one, none = qc.sizes_one_block_box(n)
    return [(qc.voxel_box((-32768, 32767), (24, 31), (-16, -9)), n), (one, 1), (none, 0)]


@pytest.mark.parametrize("n", qc.SIZES)
def test_sizes(n, make_engine, make_oracle, tmp_path):
    """16-byte and 20-byte records on both sides of 4096 selected blocks (the download kernel's two grids) and of
    4 MiB (the single copy and the 16-piece copy with its short last piece)"""
    m = qc.sizes(n)
    gpu, _, d = _pair(make_engine, make_oracle, m)
    qc.check_gathers(gpu, m.blocks, d, tmp_path / "all.bin", m.name)
    for box, count in _size_boxes(n):
        c = qc.Case(f"{count}_blocks", box, qc.grid_bounds(box, qc.VS), count)
        assert qc.check_query(gpu, m.blocks, c, d, m.name) == 512 * count


def test_small_results_after_a_large_one(make_engine, make_oracle, tmp_path):
    """the download buffers only grow: after 4097 blocks, one block and then none come out alone"""
    n = qc.SIZES[-1]
    m = qc.sizes(n)
    gpu, _, d = _pair(make_engine, make_oracle, m)
    (full, _), (one, _), (none, _) = _size_boxes(n)
    for box, count in ((full, n), (one, 1), (none, 0), (one, 1)):
        c = qc.Case(f"{count}_blocks", box, qc.grid_bounds(box, qc.VS), count)
        assert qc.check_query(gpu, m.blocks, c, d, m.name) == 512 * count
    qc.check_gathers(gpu, m.blocks, d, tmp_path / "all.bin", m.name)
    # the empty result through the raw entry point: n == 0 and a buffer that can be given back
    b, p, cnt = Bounds(*none), C.c_void_p(), C.c_size_t(77)
    assert gpu.lib.fn["query"](gpu._h, C.byref(b), C.byref(p), C.byref(cnt)) == 0
    assert cnt.value == 0
    assert gpu.lib.fn["free_buffer"](p) == 0


def test_tiny_table(make_engine, make_oracle, tmp_path):
    """16 occupancy words, chains; again after a third of the blocks is deleted (dead chain nodes stay behind)"""
    m = qc.tiny_table()
    gpu, cpu, d = _pair(make_engine, make_oracle, m)
    home = np.array([qc.ref_hash(p, 9) for p in qc.directory_positions(d[1])])
    assert ((d[0] >> 1) != home).sum() >= 20, "hardly any block is chained"
    box = qc.voxel_box((-16, 15), (-24, 7), (-8, 23))
    c = qc.Case("box", box, qc.grid_bounds(box, qc.VS), 62)      # (tests/test_query_cases.py counts them)
    qc.check_gathers(gpu, m.blocks, d, tmp_path / "all.bin", m.name)
    assert qc.check_query(gpu, m.blocks, c, d, m.name) == 512 * c.count
    gone = m.blocks.take(np.arange(0, 200, 3))
    for e in (gpu, cpu):
        e.test_delete(gone.pos)
    # (one call is one carve pass: a delete that finds its bucket locked by another of the pass is dropped, alike
    # in both implementations)
    ei, bl = assert_directory_equal(gpu, cpu)
    assert 200 - len(gone) <= len(ei) <= 200 - 0.9 * len(gone) and (np.diff(ei) > 0).all()
    left = m.blocks.take(qc.rows_of(m.blocks, qc.directory_positions(bl)))
    deleted = ~np.isin(qc.block_keys(gone.pos), qc.block_keys(left.pos))
    assert deleted.sum() >= 0.9 * len(gone)
    qc.check_gathers(gpu, m.blocks, (ei, bl), tmp_path / "left.bin", "tiny_table after the deletes")
    n = qc.check_query(gpu, m.blocks, c, (ei, bl), "tiny_table after the deletes")
    assert 0 < n < 512 * c.count
    # deleted blocks are gone: no record lies in one of them
    got = gpu.gather_valid()
    first = got[::512]
    vox = np.stack([first[k] for k in ("x", "y", "z")], axis=1)
    want = (qc.directory_positions(bl) * 8).astype(np.float32) * np.float32(qc.VS)
    assert np.array_equal(vox, want) and len(first) == len(left)


# ---------------------------------------------------------------------------------------------------------------------
# integrated maps
VS_I, TRUNC_I = 0.01, 0.06


def _integrate(engines, frames, sync=False):
    for f in frames:
        for e in engines:
            e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
            if sync:
                e.synchronize()


@pytest.fixture(scope="module")
def churn():
    return synthetic.stream("sphere", 12, scale=0.25, noise=True, holes=True)


def _from_map(src, semantic, gb=None):
    """the restatement fed from the map of `src` (directory and voxels as it dumps them)"""
    ei, bl = src.dump_directory()
    pos = qc.directory_positions(bl)
    keep = qc.select(pos, gb) if gb is not None else np.ones(len(pos), dtype=bool)
    t, _, p = src.dump_voxels(bl["idx"][keep])
    return qc.records(pos[keep], ei[keep], t, p, VS_I, semantic)


def _assert_integrated(got, want, what):
    """positions and tsdf bit for bit; the probability within the parity bar"""
    assert got.dtype == want.dtype and len(got) == len(want), f"{what}: {len(got)} records, {len(want)} expected"
    for k in ("x", "y", "z", "tsdf"):
        assert qc.same_bytes(got[k], want[k]), f"{what}: {k} differs"
    if "prob" in got.dtype.names:
        worst = float(np.max(np.abs(got["prob"] - want["prob"]), initial=0))
        print(f"{what}: probability differs by at most {worst}")
        assert worst <= TOL, f"{what}: probability differs by {worst}"


def test_after_a_carving_batch(make_engine, make_oracle, churn):
    """query and gather_valid_semantic right behind integrate_device_batch of a frame that carves, no synchronisation
    in between: they see the frame complete, its deferred pool releases included"""
    from ratsdf import devmem
    oracle = make_oracle(VS_I, TRUNC_I, threads=8)
    carve = None
    for i, f in enumerate(churn):
        _integrate([oracle], [f])
        if i >= 2 and oracle.last_frame_stats()["deleted_blocks"] > 0:
            carve = i
            break
    assert carve is not None, "no frame of the stream carves"
    dev, host = make_engine(VS_I, TRUNC_I), make_engine(VS_I, TRUNC_I)
    _integrate([dev], churn[:carve])
    _integrate([host], churn[:carve + 1], sync=True)
    f = churn[carve]
    bufs = [devmem.DeviceArray(np.ascontiguousarray(f[k])) for k in ("rgb", "depth", "ht", "lt")]
    batch = dev.make_batch([bufs[0].data_ptr()], [bufs[1].data_ptr()], [bufs[2].data_ptr()], [bufs[3].data_ptr()],
                           f["height"], f["width"], 4.0, [f["intrinsics"]], [f["pose"]])
    box = (-0.33, 0.47, -0.26, 0.60, 1.05, 1.65)      # part of the map
    gb = qc.grid_bounds(box, VS_I)
    dev.integrate_device_batch(batch)
    got_q = dev.query(box)                       # no synchronisation in between
    assert host.last_frame_stats()["deleted_blocks"] > 0
    want_q = host.query(box)
    assert qc.same_bytes(got_q, want_q), qc.first_difference(got_q, want_q)
    assert 0 < len(got_q) < len(host.gather_valid())
    _assert_integrated(got_q, _from_map(oracle, False, gb), "query after the batch")

    # the same for the 20-byte gather, on a fresh pair of engines
    dev2 = make_engine(VS_I, TRUNC_I)
    _integrate([dev2], churn[:carve])
    batch2 = dev2.make_batch([bufs[0].data_ptr()], [bufs[1].data_ptr()], [bufs[2].data_ptr()], [bufs[3].data_ptr()],
                             f["height"], f["width"], 4.0, [f["intrinsics"]], [f["pose"]])
    dev2.integrate_device_batch(batch2)
    got_s = dev2.gather_valid_semantic()         # no synchronisation in between
    want_s = host.gather_valid_semantic()
    assert qc.same_bytes(got_s, want_s), qc.first_difference(got_s, want_s)
    _assert_integrated(got_s, _from_map(oracle, True), "gather_valid_semantic after the batch")


def _snapshot(e):
    ei, blocks = e.dump_directory()
    nf, heap = e.dump_heap()
    t, c, p = e.dump_voxels(blocks["idx"])
    return ei, blocks, nf, heap[:nf].copy(), t, c, p


def test_read_outs_are_read_only(make_engine, make_oracle, churn, tmp_path):
    gpu, cpu = make_engine(VS_I, TRUNC_I), make_oracle(VS_I, TRUNC_I, threads=8)
    _integrate([gpu, cpu], churn[:6])
    before = _snapshot(gpu)
    assert len(gpu.query((-0.77, 0.83, -0.60, 0.60, 1.05, 1.65))) > 0
    assert len(gpu.gather_valid()) == len(gpu.gather_valid_semantic()) == 512 * len(before[0])
    gpu.download_all(tmp_path / "all.bin")
    for x, y in zip(before, _snapshot(gpu)):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y
    _integrate([gpu, cpu], churn[6:10])
    assert_maps_equal(gpu, cpu)


# ---------------------------------------------------------------------------------------------------------------------
# errors
def test_a_device_error_is_reported_by_every_read_out(make_engine, tmp_path):
    import ratsdf
    small = make_engine(VS_I, TRUNC_I, block_bits=6)   # 64 blocks: the first frame exhausts the pool
    with pytest.raises(ratsdf.RatsdfError) as ei:
        _integrate([small], [synthetic.frame("room", 0, scale=0.25)])
        small.synchronize()
    assert ei.value.status == 3
    for call in (lambda: small.query((-1, 1, -1, 1, 0, 2)), small.gather_valid, small.gather_valid_semantic,
                 lambda: small.download_all(tmp_path / "all.bin")):
        with pytest.raises(ratsdf.RatsdfError) as ei:
            call()
        assert ei.value.status == 3


def test_bad_arguments(make_engine, tmp_path):
    import ratsdf
    e = make_engine(qc.VS, qc.TRUNC, **qc.signs().engine)
    qc.load(e, qc.signs())
    fn, h = e.lib.fn, e._h
    b, p, n = Bounds(-1, 1, -1, 1, -1, 1), C.c_void_p(), C.c_size_t()
    assert fn["query"](h, None, C.byref(p), C.byref(n)) == 1
    assert fn["query"](h, C.byref(b), None, C.byref(n)) == 1
    assert fn["query"](h, C.byref(b), C.byref(p), None) == 1
    assert fn["query"](None, C.byref(b), C.byref(p), C.byref(n)) == 1
    for name in ("gather_valid", "gather_valid_semantic"):
        assert fn[name](h, None, C.byref(n)) == 1 and fn[name](h, C.byref(p), None) == 1
    assert fn["download_all"](h, None) == 1
    with pytest.raises(ratsdf.RatsdfError) as ei:
        e.download_all(tmp_path / "no_such_directory" / "all.bin")
    assert ei.value.status == 1
    # none of it disturbed the engine
    d = qc.directory_of(e, qc.signs())
    qc.check_gathers(e, qc.signs().blocks, d, tmp_path / "all.bin", "signs after the refused calls")
