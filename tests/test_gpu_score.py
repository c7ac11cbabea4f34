"""The label score of the HIP engine (include/ratsdf_score.h) against its numpy restatement (tests/score_ref.py) on the
crafted cases of tests/score_cases.py: score table and per-voxel records byte for byte, through both entry points.
Maps are imported from the cases' block sets; an engine's directory dump only says in which order they are gathered."""
import ctypes as C

import numpy as np
import pytest

import fuse_ref
import query_cases as qc
import score_cases as sc
import score_ref
from ratsdf import devmem
from ratsdf._abi import LABEL_SCORE_DTYPE, VOXEL_LABEL_DTYPE, LabelScore, ScoreParams
from raycast_cases import BlockSet

pytestmark = pytest.mark.gpu


def _engine(make_engine, c, **kw):
    e = make_engine(c.vs, 6 * c.vs, **{**c.engine, **kw})
    qc.load(e, c.blocks)
    return e


def _rows(e, c):
    return sc.rows_in_order(c, qc.directory_of(e, c.blocks)[1])


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
    """score_labels_device into fresh buffers filled with a pattern: (score record, records, count)"""
    d_score = devmem.DeviceArray(np.full(520, -7, dtype=np.int64))
    d_pv = devmem.DeviceArray(np.full(max(n_voxels, 1) * 2, -9, dtype=np.int32)) if with_records else 0
    d_count = devmem.DeviceArray(np.full(1, -5, dtype=np.int64))
    e.score_labels_device(s, d_score, d_pv, capacity, d_count, **params)
    e.synchronize()
    rec = d_score.numpy().view(LABEL_SCORE_DTYPE).reshape(())
    pv = d_pv.numpy().view(VOXEL_LABEL_DTYPE)[:n_voxels] if with_records else None
    return rec, pv, int(d_count.numpy()[0])


@pytest.mark.parametrize("name", sc.NAMES)
def test_both_entry_points_equal_the_restatement(make_engine, name):
    c = sc.case(name)
    e = _engine(make_engine, c)
    before = _snapshot(e)
    want_rec, want_pv = sc.expected(c, _rows(e, c))
    with e.label_set(c.points, c.labels, c.cell) as s:
        info = s.info
        want_info = sc.expected_info(c.points, c.cell, c.vs)
        assert info == want_info, (info, want_info)
        got, pv = e.score_labels(s, per_voxel=True, **c.params)
        print(name, got, "cells", info["cells"], "cell", info["cell"])
        assert isinstance(got, LabelScore) and pv.dtype == VOXEL_LABEL_DTYPE
        assert got.record.tobytes() == want_rec.tobytes(), (got.record, want_rec)
        assert pv.tobytes() == want_pv.tobytes(), qc.first_difference(pv, want_pv)
        assert e.score_labels(s, **c.params) == got                      # without the records: the same table
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


def test_empty_map_and_refused_arguments(make_engine):
    import ratsdf
    c = sc.case("points_257")
    e = make_engine(c.vs, 6 * c.vs, **c.engine)
    with e.label_set(c.points, c.labels) as s:
        got, pv = e.score_labels(s, per_voxel=True, **c.params)
        assert got.record.tobytes() == np.zeros((), dtype=LABEL_SCORE_DTYPE).tobytes() and len(pv) == 0
        cell = s.info["cell"]
        bad = [dict(tsdf_below=float("nan")), dict(p_cutoff=float("nan")), dict(max_dist=0.0), dict(max_dist=-1.0),
               dict(max_dist=float("inf")), dict(max_dist=float("nan")), dict(max_dist=64.5 * cell),
               dict(min_weight=256)]
        for kw in bad:
            with pytest.raises(ratsdf.RatsdfError) as ei:
                e.score_labels(s, **{**c.params, **kw})
            assert ei.value.status == 1, kw
        e.score_labels(s, **{**c.params, "max_dist": 64.0 * cell})      # the largest reach is admitted
        # flags, reserved words, alignment, capacity, NULLs: nothing is written
        out = np.full(520, -3, dtype=np.int64)
        fn = e.lib.fn["score_labels"]
        for params in (ScoreParams(0.1, 0.3, 0.5, 0, 1), ScoreParams(0.1, 0.3, 0.5, 0, 0, (C.c_uint32 * 3)(0, 0, 1))):
            assert fn(e._h, s._h, C.byref(params), out.ctypes.data, None, None) == 1
        ok = ScoreParams(0.1, 0.3, 0.5, 0, 0)
        assert fn(e._h, None, C.byref(ok), out.ctypes.data, None, None) == 1
        assert fn(e._h, s._h, None, out.ctypes.data, None, None) == 1
        assert fn(e._h, s._h, C.byref(ok), None, None, None) == 1
        assert (out == -3).all()
        d = devmem.DeviceArray(np.full(522, -3, dtype=np.int64))
        dev = e.lib.fn["score_labels_device"]
        p = d.data_ptr()
        for args in ((p + 4, None, 0, p + 4160), (p, p + 4164, 8, p + 4160), (p, None, 0, p + 4164),
                     (p, None, -1, p + 4160), (None, None, 0, p + 4160), (p, None, 0, None)):
            assert dev(e._h, s._h, C.byref(ok), *args) == 1, args
        e.synchronize()
        assert (d.numpy() == -3).all()
    # label sets that are refused
    for pts, lab, cell in ((c.points, np.full(len(c.points), 3, np.uint8), 0.0), (c.points, c.labels, -0.5),
                           (c.points, c.labels, float("nan")), (c.points, c.labels, float("inf"))):
        with pytest.raises(ratsdf.RatsdfError) as ei:
            e.label_set(pts, lab, cell)
        assert ei.value.status == 1
    bad_labels = np.where(np.arange(len(c.points)) == 200, 9, c.labels).astype(np.uint8)
    d_xyz, d_bad = devmem.DeviceArray(c.points), devmem.DeviceArray(bad_labels)
    with pytest.raises(ratsdf.RatsdfError) as ei:                        # the build kernel counts labels above 2
        e.label_set(d_xyz, d_bad)
    assert ei.value.status == 1
    h = C.c_void_p(0x55)
    assert e.lib.fn["labelset_create"](e._h, None, None, 5, 0.0, C.byref(h)) == 1 and h.value == 0x55
    assert e.lib.fn["labelset_create"](e._h, c.points.ctypes.data, c.labels.ctypes.data, (1 << 26) + 1, 0.0,
                                       C.byref(h)) == 1 and h.value == 0x55


@pytest.mark.parametrize("name", ("non_finite", "doubled_cell", "crowded_2049", "points_0"))
def test_a_set_from_device_pointers_equals_one_from_host_arrays(make_engine, name):
    c = sc.case(name)
    e = _engine(make_engine, c)
    d_xyz, d_lab = devmem.DeviceArray(c.points), devmem.DeviceArray(c.labels)
    with e.label_set(c.points, c.labels, c.cell) as host, e.label_set(d_xyz, d_lab, c.cell) as dev:
        assert host.info == dev.info
        a, pa = e.score_labels(host, per_voxel=True, **c.params)
        b, pb = e.score_labels(dev, per_voxel=True, **c.params)
        assert a == b and pa.tobytes() == pb.tobytes()
        assert d_xyz.numpy().tobytes() == c.points.tobytes() and d_lab.numpy().tobytes() == c.labels.tobytes()


def test_a_set_is_shared_by_engines_of_different_voxel_size(make_engine):
    """built by the engine of 1 / 64 (cell 1 / 8), used by that one and by one of 0.02"""
    a, b = sc.case("ties"), sc.case("cell_border")
    ea, eb = _engine(make_engine, a), _engine(make_engine, b)
    pts = np.concatenate([a.points, b.points])
    lab = np.concatenate([a.labels, b.labels])
    with ea.label_set(pts, lab) as s:
        assert s.info["cell"] == 0.125
        for e, c in ((ea, a), (eb, b), (ea, a)):
            b_ = c.blocks
            rows = _rows(e, c)
            want = score_ref.score(b_.pos[rows], b_.tsdf[rows], b_.rgbw["weight"][rows], b_.prob[rows], c.vs, pts, lab,
                                   **c.params)
            got, pv = e.score_labels(s, per_voxel=True, **c.params)
            assert got.record.tobytes() == want[0].tobytes() and pv.tobytes() == want[1].tobytes()


def test_shard_scores_add_up_to_the_unsharded_engine(make_engine):
    c = sc.case("layout_tiny_table")
    whole = _engine(make_engine, c)
    shard = (2, 1)                                                       # (count, slab bits): pairs of blocks in x
    with whole.label_set(c.points, c.labels) as s:
        want = whole.score_labels(s, **c.params)
        total, blocks = None, 0
        for r in range(shard[0]):
            own = fuse_ref.shard_owned(c.blocks.pos, r, *shard)
            assert 0 < own.sum() < len(own)
            e = make_engine(c.vs, 6 * c.vs, shard_rank=r, shard_count=shard[0], shard_slab_bits=shard[1], **c.engine)
            qc.load(e, BlockSet(*(v[own] for v in c.blocks)))
            part = e.score_labels(s, **c.params)
            blocks += part.voxels // 512
            total = part if total is None else total + part
        assert blocks == len(c.blocks)
        assert total == want and total.iou == want.iou
    assert want.record.tobytes() == sc.expected(c, np.arange(len(c.blocks)))[0].tobytes()


def test_frames_of_the_golden_room_scored_against_its_own_surface(make_engine):
    """the four frames of tests/golden/room_160x120_2cm_4f.npz integrated by the engine; labelled points are every
    third surface point of the map, labelled by its probability.  The restatement reads the engine's voxels."""
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
    surf = e.surface_points([int(v) for v in lo], [int(v) for v in hi - lo + 1])[::3]
    assert len(surf) > 200
    pts = np.ascontiguousarray(surf["pos"])
    lab = np.where(np.arange(len(surf)) % 7 == 0, 0, np.where(surf["prob"] > 0.5, 2, 1)).astype(np.uint8)
    params = dict(tsdf_below=0.1, max_dist=0.1, p_cutoff=0.5, min_weight=0)
    want = score_ref.score(pos, tsdf, rgbw["weight"], prob, vs, pts, lab, **params)
    before = _snapshot(e)
    with e.label_set(pts, lab) as s:
        got, pv = e.score_labels(s, per_voxel=True, **params)
    print(got)
    assert got.record.tobytes() == want[0].tobytes() and pv.tobytes() == want[1].tobytes()
    assert got.selected > 1000 and min(got.confusion) >= 0 and sum(got.confusion) > 500 and got.unannotated > 0
    curve = got.pr_curve()
    assert (curve["tp"][128], curve["fp"][128]) != (0, 0) and np.all(np.diff(curve["tp"]) <= 0)
    _same_snapshot(before, _snapshot(e))
