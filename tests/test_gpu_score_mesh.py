"""The label score against a mesh of the HIP engine (include/ratsdf_score_mesh.h) against its numpy restatement
(tests/score_mesh_ref.py) on the crafted cases of tests/score_mesh_cases.py: score table and per-voxel records byte for
byte, through both entry points.  Maps are imported from the cases' block sets; an engine's directory dump only says in
which order they are gathered."""
import ctypes as C

import numpy as np
import pytest

import query_cases as qc
import score_mesh_cases as mc
import score_mesh_ref as mr
import score_ref
from ratsdf import devmem
from ratsdf._abi import LABEL_SCORE_DTYPE, VOXEL_LABEL_DTYPE, LabelScore, ScoreParams

pytestmark = pytest.mark.gpu


def _engine(make_engine, c, **kw):
    e = make_engine(c.vs, 6 * c.vs, **{**c.engine, **kw})
    qc.load(e, c.blocks)
    return e


def _rows(e, c):
    return mc.rows_in_order(c, qc.directory_of(e, c.blocks)[1])


def _snapshot(e):
    ei, blocks = e.dump_directory()
    nf, heap = e.dump_heap()
    t, col, p = e.dump_voxels(blocks["idx"])
    return [ei, blocks, np.int64(nf), heap[:nf].copy(), t, col, p]


def _same_snapshot(a, b):
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def _device_score(e, s, n_voxels, capacity, params, with_records=True):
    """score_mesh_device into fresh buffers filled with a pattern: (score record, records, count)"""
    d_score = devmem.DeviceArray(np.full(520, -7, dtype=np.int64))
    d_pv = devmem.DeviceArray(np.full(max(n_voxels, 1) * 2, -9, dtype=np.int32)) if with_records else 0
    d_count = devmem.DeviceArray(np.full(1, -5, dtype=np.int64))
    e.score_mesh_device(s, d_score, d_pv, capacity, d_count, **params)
    e.synchronize()
    rec = d_score.numpy().view(LABEL_SCORE_DTYPE).reshape(())
    pv = d_pv.numpy().view(VOXEL_LABEL_DTYPE)[:n_voxels] if with_records else None
    return rec, pv, int(d_count.numpy()[0])


def _first_difference(got, want):
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    return f"{len(bad)} records differ, the first: {bad[:1]} {got[bad[:1]]} != {want[bad[:1]]}"


@pytest.mark.parametrize("name", mc.NAMES)
def test_both_entry_points_equal_the_restatement(make_engine, name):
    c = mc.case(name)
    e = _engine(make_engine, c)
    before = _snapshot(e)
    want_rec, want_pv = mc.expected(c, _rows(e, c))
    with e.label_mesh(c.vertices, c.labels, c.triangles, c.cell) as s:
        info = s.info
        want_info = mc.expected_info(c)
        print(name, info)
        assert info == want_info, (info, want_info)
        got, pv = e.score_mesh(s, per_voxel=True, **c.params)
        print(name, got)
        assert isinstance(got, LabelScore) and pv.dtype == VOXEL_LABEL_DTYPE
        assert pv.tobytes() == want_pv.tobytes(), _first_difference(pv, want_pv)
        assert got.record.tobytes() == want_rec.tobytes(), (got.record, want_rec)
        assert e.score_mesh(s, **c.params) == got                        # without the records: the same table
        # the records line up with gather_valid_semantic of the same engine
        sem = e.gather_valid_semantic()
        assert len(sem) == len(pv)
        q = score_ref.voxel_positions(c.blocks.pos[_rows(e, c)], c.vs).reshape(-1, 3)
        assert np.array_equal(np.stack([sem["x"], sem["y"], sem["z"]], axis=1), q)
        # the device form: everything, a prefix, and a pure count
        n = len(want_pv)
        rec, dpv, count = _device_score(e, s, n, n, c.params)
        assert rec.tobytes() == want_rec.tobytes() and dpv.tobytes() == want_pv.tobytes() and count == n
        cap = n // 2 + 3
        rec, dpv, count = _device_score(e, s, n, cap, c.params)
        assert rec.tobytes() == want_rec.tobytes() and count == n
        assert dpv[:cap].tobytes() == want_pv[:cap].tobytes()
        assert (dpv[cap:].view(np.int32) == -9).all()                    # nothing beyond the capacity
        rec, _, count = _device_score(e, s, n, 0, c.params, with_records=False)
        assert rec.tobytes() == want_rec.tobytes() and count == n
    _same_snapshot(before, _snapshot(e))                                 # the map is only read


def test_the_point_score_on_the_same_vertices_counts_the_wall_differently(make_engine):
    c = mc.case("mesh_against_points")
    e = _engine(make_engine, c)
    with e.label_mesh(c.vertices, c.labels, c.triangles) as m, e.label_set(c.vertices, c.labels) as s:
        mesh, points = e.score_mesh(m, **c.params), e.score_labels(s, **c.params)
    assert mesh.selected == points.selected == 1024
    assert mesh.confusion != points.confusion
    assert mesh.confusion[1] + mesh.confusion[3] > 300 and points.confusion[1] + points.confusion[3] == 0
    assert mesh.record.tobytes() == mc.expected(c, _rows(e, c))[0].tobytes()


def test_empty_map_and_refused_arguments(make_engine):
    import ratsdf
    c = mc.case("tris_257")
    e = make_engine(c.vs, 6 * c.vs, **c.engine)
    with e.label_mesh(c.vertices, c.labels, c.triangles) as s:
        got, pv = e.score_mesh(s, per_voxel=True, **c.params)
        assert got.record.tobytes() == np.zeros((), dtype=LABEL_SCORE_DTYPE).tobytes() and len(pv) == 0
        cell = s.info["cell"]
        bad = [dict(tsdf_below=float("nan")), dict(p_cutoff=float("nan")), dict(max_dist=0.0), dict(max_dist=-1.0),
               dict(max_dist=float("inf")), dict(max_dist=float("nan")), dict(max_dist=64.5 * cell),
               dict(min_weight=256)]
        for kw in bad:
            with pytest.raises(ratsdf.RatsdfError) as ei:
                e.score_mesh(s, **{**c.params, **kw})
            assert ei.value.status == 1, kw
        e.score_mesh(s, **{**c.params, "max_dist": 64.0 * cell})         # the largest reach is admitted
        # flags, reserved words, alignment, capacity, NULLs: nothing is written
        out = np.full(520, -3, dtype=np.int64)
        fn = e.lib.fn["score_mesh"]
        for params in (ScoreParams(0.1, 0.3, 0.5, 0, 1), ScoreParams(0.1, 0.3, 0.5, 0, 0, (C.c_uint32 * 3)(0, 0, 1))):
            assert fn(e._h, s._h, C.byref(params), out.ctypes.data, None, None) == 1
        ok = ScoreParams(0.1, 0.3, 0.5, 0, 0)
        assert fn(e._h, None, C.byref(ok), out.ctypes.data, None, None) == 1
        assert fn(e._h, s._h, None, out.ctypes.data, None, None) == 1
        assert fn(e._h, s._h, C.byref(ok), None, None, None) == 1
        assert (out == -3).all()
        d = devmem.DeviceArray(np.full(522, -3, dtype=np.int64))
        dev = e.lib.fn["score_mesh_device"]
        p = d.data_ptr()
        for args in ((p + 4, None, 0, p + 4160), (p, p + 4164, 8, p + 4160), (p, None, 0, p + 4164),
                     (p, None, -1, p + 4160), (None, None, 0, p + 4160), (p, None, 0, None)):
            assert dev(e._h, s._h, C.byref(ok), *args) == 1, args
        e.synchronize()
        assert (d.numpy() == -3).all()
    # mesh sets that are refused, from host arrays and from device pointers: a label of 3 (on a vertex no triangle
    # uses), an index of -1, an index of V; a bad cell
    v, l, t = c.vertices, c.labels, c.triangles
    assert not (t == 0).any()                                            # (vertex 0 is the unused one)
    label3 = np.where(np.arange(len(l)) == 0, 3, l).astype(np.uint8)
    minus, beyond = t.copy(), t.copy()
    minus[200, 1], beyond[256, 2] = -1, len(v)
    for vv, ll, tt, cell in ((v, label3, t, 0.0), (v, l, minus, 0.0), (v, l, beyond, 0.0), (v, l, t, -0.5),
                             (v, l, t, float("nan")), (v, l, t, float("inf")), (v[:0], l[:0], t[:1] * 0, 0.0)):
        with pytest.raises(ratsdf.RatsdfError) as ei:
            e.label_mesh(vv, ll, tt, cell)
        assert ei.value.status == 1
    d_v, d_l, d_t = devmem.DeviceArray(v), devmem.DeviceArray(l), devmem.DeviceArray(t)
    for ll, tt in ((label3, t), (l, minus), (l, beyond)):                # the build kernel counts both
        with pytest.raises(ratsdf.RatsdfError) as ei:
            e.label_mesh(d_v, devmem.DeviceArray(ll), devmem.DeviceArray(tt))
        assert ei.value.status == 1
    e.label_mesh(d_v, d_l, d_t).close()
    h = C.c_void_p(0x55)
    make = e.lib.fn["labelmesh_create"]
    assert make(e._h, None, None, 5, None, 0, 0.0, C.byref(h)) == 1 and h.value == 0x55
    assert make(e._h, v.ctypes.data, l.ctypes.data, len(v), None, 5, 0.0, C.byref(h)) == 1 and h.value == 0x55
    assert make(e._h, v.ctypes.data, l.ctypes.data, (1 << 26) + 1, t.ctypes.data, len(t), 0.0, C.byref(h)) == 1
    assert make(e._h, v.ctypes.data, l.ctypes.data, len(v), t.ctypes.data, (1 << 26) + 1, 0.0, C.byref(h)) == 1
    assert make(e._h, v.ctypes.data, l.ctypes.data, len(v), t.ctypes.data, len(t), 0.0, None) == 1
    assert h.value == 0x55
    with e.label_mesh(v, l, t[:0]) as s:                                 # T == 0 is a valid, empty set
        assert s.info["kept"] == 0 and s.info["vertices"] == len(v) and s.info["cells"] == (1, 1, 1)


@pytest.mark.parametrize("name", ("non_finite", "ref_cap", "crowded_600", "tris_0", "coincident"))
def test_a_set_from_device_pointers_equals_one_from_host_arrays(make_engine, name):
    c = mc.case(name)
    e = _engine(make_engine, c)
    d_v, d_l, d_t = devmem.DeviceArray(c.vertices), devmem.DeviceArray(c.labels), devmem.DeviceArray(c.triangles)
    with e.label_mesh(c.vertices, c.labels, c.triangles, c.cell) as host, \
            e.label_mesh(d_v, d_l, d_t, c.cell) as dev:
        assert host.info == dev.info
        a, pa = e.score_mesh(host, per_voxel=True, **c.params)
        b, pb = e.score_mesh(dev, per_voxel=True, **c.params)
        assert a == b and pa.tobytes() == pb.tobytes()
        assert d_v.numpy().tobytes() == c.vertices.tobytes() and d_l.numpy().tobytes() == c.labels.tobytes()
        assert d_t.numpy().tobytes() == c.triangles.tobytes()


@pytest.mark.parametrize("cell", (0.05, 0.4))
def test_no_result_depends_on_the_grid(make_engine, cell):
    for name in ("spanning", "covering_box", "slivers"):
        c = mc.case(name)
        e = _engine(make_engine, c)
        want_rec, want_pv = mc.expected(c, _rows(e, c))
        with e.label_mesh(c.vertices, c.labels, c.triangles, cell) as s:
            assert s.info["cell"] == float(np.float32(cell))
            got, pv = e.score_mesh(s, per_voxel=True, **{**c.params, "max_dist": min(c.params["max_dist"], 64 * cell)})
        assert got.record.tobytes() == want_rec.tobytes() and pv.tobytes() == want_pv.tobytes()


def test_a_set_is_shared_by_engines_of_different_voxel_size(make_engine):
    """built by the engine of 1 / 64 (cell 1 / 8), used by that one and by one of 0.02"""
    a, b = mc.case("ties"), mc.case("cell_border")
    ea, eb = _engine(make_engine, a), _engine(make_engine, b)
    v, lab, t = mc.join((a.vertices, a.labels, a.triangles), (b.vertices, b.labels, b.triangles))
    with ea.label_mesh(v, lab, t) as s:
        assert s.info["cell"] == 0.125
        for e, c in ((ea, a), (eb, b), (ea, a)):
            b_ = c.blocks
            rows = _rows(e, c)
            want = mr.score(b_.pos[rows], b_.tsdf[rows], b_.rgbw["weight"][rows], b_.prob[rows], c.vs, v, lab, t,
                            **c.params)
            got, pv = e.score_mesh(s, per_voxel=True, **c.params)
            assert got.record.tobytes() == want[0].tobytes() and pv.tobytes() == want[1].tobytes()


def test_frames_of_the_golden_room_scored_against_a_triangulated_surface(make_engine):
    """the four frames of tests/golden/room_160x120_2cm_4f.npz integrated by the engine; the mesh is the engine's own
    welded surface mesh of a box of the map, every vertex labelled by its probability, so that triangles of mixed
    labels occur.  The restatement reads the engine's voxels; tsdf_below and the thinned mesh keep the brute force small."""
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
    import make_golden
    from ratsdf import synthetic
    scene, n, cam, scale, vs, sem, noise, holes = make_golden.CASES["room_160x120_2cm_4f"]
    e = make_engine(vs, 6 * vs)
    for i in range(n):
        f = synthetic.frame(scene, i, cam=cam, scale=scale, semantic=sem, noise=noise, holes=holes)
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
    ei, bl = e.dump_directory()
    tsdf, rgbw, prob = e.dump_voxels(bl["idx"])
    pos = qc.directory_positions(bl)
    lo, hi = pos.min(axis=0) * 8, pos.max(axis=0) * 8 + 7
    verts, tris = e.surface_mesh([int(v) for v in lo], [int(v) for v in hi - lo + 1])
    keep = np.flatnonzero(np.arange(len(tris)) % max(1, len(tris) // 1800) == 0)[:2000]
    tris = np.ascontiguousarray(tris[keep]).astype(np.int32).reshape(-1, 3)
    pts = np.ascontiguousarray(verts["pos"])
    lab = np.where(np.arange(len(verts)) % 7 == 0, 0, np.where(verts["prob"] > 0.5, 2, 1)).astype(np.uint8)
    below = float(np.sort(np.abs(tsdf).ravel())[1500])                   # (the 1 500 voxels nearest to the surface)
    params = dict(tsdf_below=below, max_dist=0.1, p_cutoff=0.5, min_weight=0)
    want = mr.score(pos, tsdf, rgbw["weight"], prob, vs, pts, lab, tris, **params)
    assert 1000 < int(want[0]["selected"]) <= 1500, want[0]["selected"]
    before = _snapshot(e)
    with e.label_mesh(pts, lab, tris) as s:
        info = s.info
        got, pv = e.score_mesh(s, per_voxel=True, **params)
    print(got, info)
    assert info["kept"] > 1000 and info["mixed"] > 0 and info["refs"] >= info["kept"]
    assert info["mixed"] == mr.mixed_triangles(pts, lab, tris)
    assert pv.tobytes() == want[1].tobytes(), _first_difference(pv, want[1])
    assert got.record.tobytes() == want[0].tobytes()
    assert min(got.confusion) >= 0 and sum(got.confusion) > 300 and got.unannotated > 0
    _same_snapshot(before, _snapshot(e))
