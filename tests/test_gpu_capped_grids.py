"""The capped launches of the exposure and of the two label scores on the HIP engine, at the sizes of
tests/capped_grid_cases.py at which a workgroup strides over several items: k_exposure_walk (and the host form's upload
in pieces), the set builders' bounds, count / scatter, reference and cell passes, and the joins over more valid blocks
than they have workgroups.  Everything is compared byte for byte with the restatements (exposure_ref, score_ref,
score_mesh_ref); tests/test_capped_grid_cases.py shows without a GPU that the cases cross the caps read from the
sources and that a dropped, a doubled or a stale second sweep changes an output compared here."""
import ctypes as C
import time

import numpy as np
import pytest

import capped_grid_cases as cg
import exposure_ref as ref
import query_cases as qc
from ratsdf import devmem
from ratsdf._abi import EXPOSURE_SUMMARY_DTYPE, LABEL_SCORE_DTYPE, LAMP_RECORD_DTYPE, VOXEL_LABEL_DTYPE
from test_gpu_regions import _craft

pytestmark = pytest.mark.gpu

F = np.float32
MASK_POISON = np.uint64(0xABABABABABABABAB)
DOSE_POISON = F(-9.0)


# ---------------------------------------------------------------------------------------------------------------------
# exposure
def _room(make_engine):
    e = make_engine(cg.XVS, cg.XTRUNC)
    state = cg.room_state()
    _craft(e, cg.ROOM_ORIGIN, state)
    assert ref.same_bytes(ref.box_state(e, cg.ROOM_ORIGIN, cg.ROOM_DIMS), state)     # the map is the crafted room
    return e


def _host_form(e, c):
    """ratsdf_exposure on the caller's arrays as the case states them: the dose array holds the sentinel (or the prior
    dose), ACCUMULATE is set only where the case says so"""
    n, m = len(c.points), len(c.lamps)
    dose, mask = c.dose.copy(), np.full(n, MASK_POISON, dtype=np.uint64)
    table, summary = np.zeros(m, dtype=LAMP_RECORD_DTYPE), np.zeros(1, dtype=EXPOSURE_SUMMARY_DTYPE)
    params = e._exposure_params(0.0, np.inf, cg.EXPOSURE_PARAMS["min_irradiance"], cg.EXPOSURE_PARAMS["p_cutoff"],
                                False, c.accumulate)
    box = [(C.c_int32 * 3)(*v) for v in (cg.ROOM_ORIGIN, cg.ROOM_DIMS)]
    assert e.lib.fn["exposure"](e._h, *box, C.byref(params), c.points.ctypes.data, n, c.lamps.ctypes.data, m,
                                dose.ctypes.data, mask.ctypes.data, table.ctypes.data, summary.ctypes.data) == 0
    return dose, mask, table, summary[0]


def _device_form(e, c):
    n, m = len(c.points), len(c.lamps)
    d_points, d_lamps = devmem.DeviceArray(c.points), devmem.DeviceArray(c.lamps)
    d_dose = devmem.DeviceArray(np.concatenate([c.dose, np.full(8, DOSE_POISON, dtype=F)]))
    d_mask = devmem.DeviceArray(np.full(n + 8, MASK_POISON, dtype=np.uint64))
    d_table = devmem.DeviceArray(np.full((m + 2, 4), 0x6C6C6C6C, dtype=np.uint32))
    d_sum = devmem.DeviceArray(np.full(8 + 4, 0xEFEFEFEF, dtype=np.uint32))
    s = e.exposure_device(cg.ROOM_ORIGIN, cg.ROOM_DIMS, d_points, n, d_lamps, m, d_dose, d_mask, d_table, d_sum,
                          accumulate=c.accumulate, **cg.EXPOSURE_PARAMS)
    dose, mask, table, summary = d_dose.numpy(), d_mask.numpy(), d_table.numpy(), d_sum.numpy()
    assert np.all(dose[n:] == DOSE_POISON) and np.all(mask[n:] == MASK_POISON)       # the poison beyond n is intact
    assert np.all(table[m:] == 0x6C6C6C6C) and np.all(summary[8:] == 0xEFEFEFEF)
    assert d_points.numpy().tobytes() == c.points.tobytes() and d_lamps.numpy().tobytes() == c.lamps.tobytes()
    record = summary[:8].view(EXPOSURE_SUMMARY_DTYPE)[0]
    assert s.tobytes() == record.tobytes()
    return dose[:n], mask[:n], table[:m].reshape(-1).view(LAMP_RECORD_DTYPE), record


def _same_exposure(got, want, what):
    """as test_gpu_exposure._check compares: mask, dose, table, summary, byte for byte"""
    assert got[2].dtype == LAMP_RECORD_DTYPE == ref.LAMP_RECORD_DTYPE and got[3].dtype == ref.SUMMARY_DTYPE
    assert ref.same_bytes(got[1], want[1]), (what, np.flatnonzero(got[1] != want[1])[:5])
    assert ref.same_bytes(got[0], want[0]), (what, np.flatnonzero(got[0].view(np.uint32) != want[0].view(np.uint32))[:5])
    assert ref.same_bytes(got[2], want[2]), (what, got[2], want[2])
    assert got[3].tobytes() == want[3].tobytes(), (what, got[3], want[3])


@pytest.mark.parametrize("name", cg.EXPOSURE_NAMES)
def test_exposure_beyond_one_sweep_of_the_walk(make_engine, name):
    c = cg.exposure_case(name)
    n, m = len(c.points), len(c.lamps)
    t0 = time.perf_counter()
    want = cg.exposure_expected(name)
    t1 = time.perf_counter()
    e = _room(make_engine)
    two_pieces = 32 * n > cg.SWEEP["upload_points"] * 32
    print(f"{n} points, {m} lamps: {n / c.sweep:.2f} sweeps of the walk" +
          (", the host form uploads the points in two pieces" if two_pieces else "") +
          f"; restated in {t1 - t0:.2f} s")
    if m == 1:
        assert two_pieces and 32 * n > 32 << 20                      # larger than the page-locked buffer (kHostChunk)
    for form in (_host_form, _device_form, _host_form):
        got = form(e, c)
        _same_exposure(got, want, (name, form.__name__))
        if not c.accumulate:                                         # OUTSIDE points keep the caller's sentinel
            assert int((got[0] == cg.SENTINEL).sum()) == int(want[3]["points_outside"]) == int(got[3]["points_outside"])
    print(f"    engine calls: {time.perf_counter() - t1:.2f} s; {want[3]}")


# ---------------------------------------------------------------------------------------------------------------------
# the scores
def _score_engine(make_engine):
    """an engine holding the 4 100-block map, and the rows of the map in the order the engine gathers them"""
    blocks = cg.score_map()
    e = make_engine(cg.SVS, 6 * cg.SVS, **cg.SCORE_ENGINE)
    for lo in range(0, len(blocks.pos), 1024):
        e.import_blocks(*(a[lo:lo + 1024] for a in blocks))
    rows = qc.rows_of(blocks, qc.directory_positions(qc.directory_of(e, blocks)[1]))
    return e, rows


class _Forms:
    """the entry points of one kind of set"""

    def __init__(self, e, c):
        self.e, self.c, self.mesh = e, c, c.triangles is not None
        self.arrays = (c.vertices, c.labels) + ((c.triangles,) if self.mesh else ())

    def build(self, device=False):
        arrays = tuple(devmem.DeviceArray(a) for a in self.arrays) if device else self.arrays
        s = (self.e.label_mesh if self.mesh else self.e.label_set)(*arrays, self.c.cell)
        return s, arrays

    def host(self, s, per_voxel=True):
        return (self.e.score_mesh if self.mesh else self.e.score_labels)(s, per_voxel=per_voxel, **cg.SCORE_PARAMS)

    def device(self, s, n_voxels, capacity, with_records=True):
        """into fresh buffers filled with a pattern: (score record, records, count)"""
        d_score = devmem.DeviceArray(np.full(520, -7, dtype=np.int64))
        d_pv = devmem.DeviceArray(np.full(n_voxels * 2, -9, dtype=np.int32)) if with_records else 0
        d_count = devmem.DeviceArray(np.full(1, -5, dtype=np.int64))
        fn = self.e.score_mesh_device if self.mesh else self.e.score_labels_device
        fn(s, d_score, d_pv, capacity, d_count, **cg.SCORE_PARAMS)
        self.e.synchronize()
        rec = d_score.numpy().view(LABEL_SCORE_DTYPE).reshape(())
        pv = d_pv.numpy().view(VOXEL_LABEL_DTYPE)[:n_voxels] if with_records else None
        return rec, pv, int(d_count.numpy()[0])


@pytest.mark.parametrize("name", cg.SCORE_NAMES)
def test_scores_beyond_one_sweep_of_the_builders_and_the_join(make_engine, name):
    c = cg.score_case(name)
    t0 = time.perf_counter()
    e, rows = _score_engine(make_engine)
    t1 = time.perf_counter()
    want_info, want_rec, want_pv = cg.score_outputs(c, rows)
    t2 = time.perf_counter()
    n = len(want_pv)
    assert n == 512 * cg.N_BLOCKS
    crossed = {k: c.items / cg.stage_sweep(c, k) for k in ("bounds", "refs", "fill") if cg.stage_sweep(c, k)}
    print(f"{c.items} items: " + ", ".join(f"{v:.3f} sweeps of {k}" for k, v in crossed.items()) +
          f"; {cg.N_BLOCKS} blocks: {cg.N_BLOCKS / cg.SWEEP['join']:.3f} sweeps of the join; map loaded in "
          f"{t1 - t0:.2f} s, restated in {t2 - t1:.2f} s")
    f = _Forms(e, c)
    s, _ = f.build()
    d, d_arrays = f.build(device=True)
    try:
        assert s.info == want_info, (s.info, want_info)
        assert d.info == want_info, (d.info, want_info)              # from device pointers: the same set
        for a, host in zip(d_arrays, f.arrays):
            assert a.numpy().tobytes() == host.tobytes()             # the caller's arrays are only read
        got, pv = f.host(s)
        print("   ", got)
        assert pv.dtype == VOXEL_LABEL_DTYPE and pv.tobytes() == want_pv.tobytes(), qc.first_difference(pv, want_pv)
        assert got.record.tobytes() == want_rec.tobytes(), (got.record, want_rec)
        again, pv2 = f.host(s)                                       # the same call on the same set: the same bytes
        assert again.record.tobytes() == want_rec.tobytes() and pv2.tobytes() == want_pv.tobytes()
        assert f.host(s, per_voxel=False) == got
        other, pv3 = f.host(d)
        assert other.record.tobytes() == want_rec.tobytes() and pv3.tobytes() == want_pv.tobytes()
        # the device form: everything, a capacity that ends inside a block of the second sweep, a pure count
        rec, dpv, count = f.device(s, n, n)
        assert rec.tobytes() == want_rec.tobytes() and dpv.tobytes() == want_pv.tobytes() and count == n
        cap = 512 * (cg.SWEEP["join"] + 7) + 129
        assert cg.SWEEP["join"] * 512 < cap < 2 * cg.SWEEP["join"] * 512 and cap % 512 and (cap % 512) % 256
        rec, dpv, count = f.device(d, n, cap)
        assert rec.tobytes() == want_rec.tobytes() and count == n
        assert dpv[:cap].tobytes() == want_pv[:cap].tobytes(), qc.first_difference(dpv[:cap], want_pv[:cap])
        assert (dpv[cap:].view(np.int32) == -9).all()                # nothing beyond the capacity
        rec, _, count = f.device(s, n, 0, with_records=False)
        assert rec.tobytes() == want_rec.tobytes() and count == n
    finally:
        s.close()
        d.close()
    print(f"    engine calls: {time.perf_counter() - t2:.2f} s")
