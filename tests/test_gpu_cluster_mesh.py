"""The clustered mesh of the HIP engine (include/ratsdf_cluster_mesh.h) against the numpy restatement of its contract
(tests/cluster_mesh_ref.py): vertices byte for byte, triangles equal as arrays.  Crafted maps brought in with
import_blocks (the sphere of test_cluster_mesh_ref at k = 2, 4, 8 through both forms, boxes that cut clusters, a single
voxel layer, the ends of the grid, an absent block, weights, noise that makes the duplicate removal act), the capacity
rule of the device form, the awkward voxel values of surface_cases.py, a map built from real frames, and the read-only
/ error behaviour.  Nothing is larger than 4 x 4 x 4 blocks."""
import ctypes as C
import functools

import numpy as np
import pytest

import cluster_mesh_ref as cref
import surface_cases as sc
import surface_mesh_ref as mref
import surface_ref as ref
import test_cluster_mesh_ref as cpu
from ratsdf import synthetic

pytestmark = pytest.mark.gpu

VS, TRUNC = 0.02, 0.12
SMALL = dict(block_bits=10)        # crafted maps hold a handful of blocks
FACTORS = cref.FACTORS


def _engine(make_engine, arrays, **kw):
    e = make_engine(VS, TRUNC, **(kw or SMALL))
    e.import_blocks(*arrays)
    return e, ref.blocks_of(*arrays)


def _check(e, blocks, origin, dims, k, min_weight=1, vs=VS, welded=None):
    v, tri = e.cluster_mesh(origin, dims, k, min_weight)
    w = welded if welded is not None else cref.welded(blocks, origin, dims, vs, min_weight)
    wv, wt = cref.cluster_mesh(blocks, origin, dims, vs, k, min_weight, mesh=w)
    print(f"box {list(origin)} {list(dims)} k {k} min_weight {min_weight}: {len(v)} vertices, {len(tri)} triangles; "
          f"restatement {len(wv)}, {len(wt)}; welded {len(w.vertices)}, {len(w.triangles)}")
    assert tri.dtype == np.int32 and tri.shape == wt.shape and np.array_equal(tri, wt), (origin, dims, k, min_weight)
    assert ref.same_bytes(v, wv), (origin, dims, k, min_weight, len(v), len(wv))
    return v, tri


@pytest.fixture(scope="module")
def sphere():
    return tuple(mref.sphere_blocks(cpu.CENTRE, cpu.RADIUS, cpu.LO, cpu.HI))


# ---- 1. boxes and factors --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", FACTORS)
def test_sphere_through_both_forms(make_engine, sphere, k):
    from ratsdf import devmem
    e, blocks = _engine(make_engine, sphere)
    v, tri = _check(e, blocks, cpu.ORIGIN, cpu.DIMS, k, welded=cpu.sphere_welded())
    assert len(tri) > 50
    cpu.check_invariants(v, tri, cpu.sphere_welded(), k, cpu.CENTRE)         # on the engine's own output
    d_v = devmem.DeviceArray(np.zeros((len(v), 8), dtype=np.int32))
    d_t = devmem.DeviceArray(np.zeros((len(tri), 3), dtype=np.int32))
    d_c = devmem.DeviceArray(np.zeros(2, dtype=np.int64))
    assert e.cluster_mesh_device(cpu.ORIGIN, cpu.DIMS, d_v, len(v), d_t, len(tri), d_c, k) == (len(v), len(tri))
    assert ref.same_bytes(d_v.numpy().reshape(-1).view(np.uint8), v.view(np.uint8))
    assert np.array_equal(d_t.numpy(), tri)


@pytest.mark.parametrize("k", FACTORS)
def test_boxes_that_cut_clusters_and_a_single_layer(make_engine, sphere, k):
    e, blocks = _engine(make_engine, sphere)
    v, tri = _check(e, blocks, [-11, -9, -5], [21, 19, 17], k)              # odd, no multiple of k: cut on both sides
    assert len(tri) > 10
    whole = e.cluster_mesh(cpu.ORIGIN, cpu.DIMS, k)[0]
    assert not set(r.tobytes() for r in v) <= set(r.tobytes() for r in whole)   # a cut cluster averages fewer members
    v, tri = _check(e, blocks, [-13, -12, 3], [26, 26, 1], k)                # one voxel layer
    assert len(v) > 0
    _check(e, blocks, [-12, -5, 2], [7, 9, 3], k)                           # inside one block's reach, off the lattice


@pytest.mark.parametrize("k", FACTORS)
def test_an_absent_block(make_engine, sphere, k):
    """block (-1, -1, 0) of the neighbourhood is missing: the clusters of its upper neighbours lose the members owned
    at their local -1, and the cells that touch it are incomplete"""
    pos = sphere[0]
    keep = ~((pos[:, 0] == -1) & (pos[:, 1] == -1) & (pos[:, 2] == 0))
    assert keep.sum() == len(pos) - 1
    e, blocks = _engine(make_engine, tuple(a[keep] for a in sphere))
    v, tri = _check(e, blocks, cpu.ORIGIN, cpu.DIMS, k)
    assert 0 < len(v) < len(cpu.sphere_mesh(k)[0])


def test_noise_where_duplicates_are_removed(make_engine):
    arrays = cpu.noise_arrays()
    e, blocks = _engine(make_engine, arrays)
    for k in FACTORS:
        assert cref.duplicates_removed(blocks, *cpu.NOISE_BOX, VS, k) > 0
        _check(e, blocks, *cpu.NOISE_BOX, k)
        _check(e, blocks, [-7, -5, 1], [13, 12, 14], k)


def test_ends_of_the_voxel_range(make_engine):
    rng = np.random.default_rng(5)
    noise = lambda x, y, z: rng.uniform(-1, 1, x.shape)
    top = ref.solid((4094, 4095, 4095), (4095, 4095, 4095), noise)
    low = ref.solid((-4096, -4096, -4096), (-4096, -4096, -4095), noise)
    e, blocks = _engine(make_engine, tuple(np.concatenate([a, b]) for a, b in zip(top, low)))
    for k in FACTORS:
        v, tri = _check(e, blocks, [32760, 32760, 32760], [8, 8, 8], k)      # origin + dims == 32768: no such voxel
        assert len(v) > 0
        _check(e, blocks, [32752, 32757, 32761], [16, 11, 7], k)             # two blocks; ends at voxel 32767
        v, tri = _check(e, blocks, [-32768, -32768, -32768], [8, 8, 16], k)
        assert len(v) > 0
        _check(e, blocks, [-32767, -32765, -32768], [5, 4, 13], k)


@pytest.fixture(scope="module")
def random_map():
    rng = np.random.default_rng(11)
    arrays = ref.solid((-2, -1, 0), (0, 1, 2), lambda x, y, z: rng.uniform(-1, 1, x.shape))
    keep = np.flatnonzero(rng.random(27) < 0.7)
    arrays = tuple(a[keep] for a in arrays)
    pos, t, c, p = arrays
    c["weight"] = rng.choice([0, 1, 2, 3] + [200] * 2 + [255] * 10, size=t.shape)
    c["r"], c["g"], c["b"] = (rng.integers(0, 256, t.shape) for _ in range(3))
    p[:] = rng.random(t.shape, dtype=np.float32)
    t[rng.random(t.shape) < 0.03] = -1.0                    # fresh voxels where the weight is 1
    t[rng.random(t.shape) < 0.02] = 0.0                     # f = 0: the lower endpoint
    return arrays


def test_min_weight_and_fresh_voxels(make_engine, random_map):
    e, blocks = _engine(make_engine, random_map)
    box = ([-17, -9, -1], [26, 26, 26])
    n = [len(_check(e, blocks, *box, 4, min_weight=mw)[1]) for mw in (1, 2, 255)]      # triangles
    assert n[0] > n[1] > n[2] > 0
    _check(e, blocks, [-13, -5, 3], [18, 19, 15], 2, min_weight=3)
    _check(e, blocks, [-13, -5, 3], [18, 19, 15], 8, min_weight=2)


def test_empty_box(make_engine, sphere):
    e, blocks = _engine(make_engine, sphere)
    for k in FACTORS:
        v, tri = _check(e, blocks, [500, 500, 500], [20, 9, 40], k)
        assert len(v) == 0 and tri.shape == (0, 3)
    v, tri = _check(e, blocks, [-16, -16, -8], [6, 6, 6], 4)                  # blocks, but no surface
    assert len(v) == 0 and tri.shape == (0, 3)


# ---- 2. the device form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 4])
def test_truncation_in_the_device_form(make_engine, random_map, k):
    import torch
    from ratsdf import devmem
    e, blocks = _engine(make_engine, random_map)
    box = ([-17, -9, -1], [26, 26, 26])
    wv, wt = cref.cluster_mesh(blocks, *box, VS, k)
    nv, nt = len(wv), len(wt)
    assert nv > 100 and nt > 100
    counts = devmem.DeviceArray(np.full(3, -1, dtype=np.int64))
    assert e.cluster_mesh_device(*box, 0, 0, 0, 0, counts, k) == (nv, nt)     # a pure count
    assert counts.numpy().tolist() == [nv, nt, -1]
    # a vertex capacity inside a block's clusters, a triangle capacity inside one first-index run
    run = int(np.flatnonzero((wt[1:, 0] == wt[:-1, 0]) & (np.arange(1, nt) > nt // 2))[0]) + 1
    assert wt[run, 0] == wt[run - 1, 0]
    guard = 0x5A5A5A5A
    for vcap, tcap in ((nv // 2 + 1, run), (nv, nt), (nv // 2 + 1, nt), (nv, run), (0, nt), (nv + 3, nt + 3)):
        d_v = devmem.DeviceArray(np.full((vcap + 4, 8), guard, dtype=np.int32))
        d_t = devmem.DeviceArray(np.full((tcap + 4, 3), guard, dtype=np.int32))
        assert e.cluster_mesh_device(*box, d_v, vcap, d_t, tcap, counts, k) == (nv, nt)
        gv, gt = d_v.numpy(), d_t.numpy()
        kv, kt = min(vcap, nv), min(tcap, nt)
        assert ref.same_bytes(gv[:kv].reshape(-1).view(np.uint8), np.ascontiguousarray(wv[:kv]).view(np.uint8))
        assert np.array_equal(gt[:kt], wt[:kt]), (vcap, tcap)                # indices beyond vcap are kept
        assert np.all(gv[kv:] == guard) and np.all(gt[kt:] == guard), (vcap, tcap)
        if vcap < nv and kt:
            assert gt[:kt].max() >= vcap
    d_v = devmem.DeviceArray(np.full((8, 8), guard, dtype=np.int32))
    d_t = devmem.DeviceArray(np.full((8, 3), guard, dtype=np.int32))
    assert e.cluster_mesh_device(*box, d_v, 0, d_t, 0, counts, k) == (nv, nt)   # capacity 0 with buffers
    assert np.all(d_v.numpy() == guard) and np.all(d_t.numpy() == guard)
    t_v = torch.zeros((nv, 8), dtype=torch.int32, device="cuda")            # torch tensors
    t_t = torch.zeros((nt, 3), dtype=torch.int32, device="cuda")
    t_c = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert e.cluster_mesh_device(*box, t_v, nv, t_t, nt, t_c, k) == (nv, nt)
    assert ref.same_bytes(t_v.cpu().numpy().reshape(-1).view(np.uint8), wv.view(np.uint8))
    assert np.array_equal(t_t.cpu().numpy(), wt)


# ---- 3. awkward values -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _awkward(name, k):
    c = sc.case(name)
    blocks = sc.blocks_of(c)
    return cref.cluster_mesh(blocks, c.origin, c.dims, sc.VS, k, mesh=cref.welded(blocks, c.origin, c.dims, sc.VS))


@pytest.mark.parametrize("name", sc.CASES)
@pytest.mark.parametrize("k", [2, 4])
def test_awkward_values(make_engine, name, k):
    """a float that is NaN in the restatement must be NaN in the engine and vice versa (any payload: a NaN that went
    through arithmetic has no agreed bits); every other word is equal bit for bit.  The NaN count is the
    restatement's own, and zero unless the set plants NaN words (nonfinite: tsdf; probabilities: prob)."""
    c = sc.case(name)
    e = make_engine(sc.VS, sc.TRUNC, **sc.ENGINE)
    e.import_blocks(*c.blocks)
    wv, wt = _awkward(name, k)
    v, tri = e.cluster_mesh(c.origin, c.dims, k)
    nans = cref.nan_count(wv)
    print(f"{name} k {k}: {len(v)} vertices, {len(tri)} triangles; restatement {len(wv)}, {len(wt)}; NaN words "
          f"{cref.nan_count(v)} / {nans}; records differing {cref.differing(v, wv)}")
    assert (nans > 0) == (name in ("nonfinite", "probabilities"))            # the exemption cannot hide a failure
    assert tri.shape == wt.shape and np.array_equal(tri, wt)
    assert cref.nan_count(v) == nans
    assert cref.differing(v, wv) == 0
    if nans == 0:
        assert ref.same_bytes(v, wv)


# ---- 4. after real frames ----------------------------------------------------------------------------------------------
def _wall_frames():
    """the frames of tests/golden/wall_80x60_2cm_3f.npz (make_golden.py's specification)"""
    return [synthetic.frame("wall", i, cam="scannet", scale=0.125, semantic=True, noise=False, holes=False)
            for i in range(3)]


def _integrate(e, frames):
    for f in frames:
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])


def _map_of(e):
    """the map's blocks for the restatement (read back with dump_directory / dump_voxels), and its bounding box"""
    _, b = e.dump_directory()
    pos = np.stack([b["x"], b["y"], b["z"]], axis=1)
    t, c, p = e.dump_voxels(b["idx"])
    lo, hi = pos.astype(int).min(0) * 8, pos.astype(int).max(0) * 8 + 7
    return ref.blocks_of(pos, t, c, p), [int(v) for v in lo], [int(v) for v in hi - lo + 1]


def test_real_frames_and_right_after_a_frame(make_engine):
    from ratsdf import devmem
    frames = _wall_frames()
    host = make_engine(VS, TRUNC)
    _integrate(host, frames)
    blocks, origin, dims = _map_of(host)
    assert max(dims) <= 1024
    wv, wt = _check(host, blocks, origin, dims, 4)
    assert len(wt) > 100
    # right after a frame, without a synchronisation in between: the deferred pool releases come first
    dev = make_engine(VS, TRUNC)
    _integrate(dev, frames[:2])
    f = frames[2]
    bufs = [devmem.DeviceArray(np.ascontiguousarray(f[k])) for k in ("rgb", "depth", "ht", "lt")]
    batch = dev.make_batch([bufs[0].data_ptr()], [bufs[1].data_ptr()], [bufs[2].data_ptr()], [bufs[3].data_ptr()],
                           f["height"], f["width"], 4.0, [f["intrinsics"]], [f["pose"]])
    d_v = devmem.DeviceArray(np.zeros((len(wv), 8), dtype=np.int32))
    d_t = devmem.DeviceArray(np.zeros((len(wt), 3), dtype=np.int32))
    d_c = devmem.DeviceArray(np.zeros(2, dtype=np.int64))
    dev.integrate_device_batch(batch)
    assert dev.cluster_mesh_device(origin, dims, d_v, len(wv), d_t, len(wt), d_c, 4) == (len(wv), len(wt))
    assert ref.same_bytes(d_v.numpy().reshape(-1).view(np.uint8), wv.view(np.uint8))
    assert np.array_equal(d_t.numpy(), wt)


# ---- 5. read-only and errors -------------------------------------------------------------------------------------------
def _snapshot(e, origin, dims):
    ei, blocks = e.dump_directory()
    nf, heap = e.dump_heap()
    t, c, p = e.dump_voxels(blocks["idx"])
    v, tri = e.surface_mesh(origin, dims)
    return ei, blocks, nf, heap[:nf].copy(), t, c, p, v, tri


def test_the_map_is_only_read(make_engine):
    from ratsdf import devmem
    e = make_engine(VS, TRUNC)
    _integrate(e, _wall_frames()[:2])
    _, origin, dims = _map_of(e)
    before = _snapshot(e, origin, dims)
    d_c = devmem.DeviceArray(np.zeros(2, dtype=np.int64))
    for k in FACTORS:
        v, tri = e.cluster_mesh(origin, dims, k)
        assert len(tri) > 0
        assert e.cluster_mesh_device(origin, dims, 0, 0, 0, 0, d_c, k) == (len(v), len(tri))
    e.cluster_mesh(origin, dims, 4, 2)
    after = _snapshot(e, origin, dims)
    for x, y in zip(before, after):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y


def test_sticky_error_is_returned(make_engine):
    import ratsdf
    from ratsdf import devmem
    small = make_engine(VS, TRUNC, block_bits=6)            # 64 blocks: the first frame exhausts the pool
    f = synthetic.frame("room", 0, scale=0.25)
    with pytest.raises(ratsdf.RatsdfError) as ei:
        _integrate(small, [f])
        small.synchronize()
    assert ei.value.status == 3
    with pytest.raises(ratsdf.RatsdfError) as ei:
        small.cluster_mesh([0, 0, 0], [8, 8, 8])
    assert ei.value.status == 3
    d_c = devmem.DeviceArray(np.zeros(2, dtype=np.int64))
    with pytest.raises(ratsdf.RatsdfError) as ei:
        small.cluster_mesh_device([0, 0, 0], [8, 8, 8], 0, 0, 0, 0, d_c)
    assert ei.value.status == 3


def test_bad_arguments(make_engine):
    import ratsdf
    from ratsdf import devmem
    from ratsdf._abi import ClusterMeshParams
    e = make_engine(VS, TRUNC, **SMALL)
    d_v = devmem.DeviceArray(np.zeros((8, 8), dtype=np.int32))
    d_t = devmem.DeviceArray(np.zeros((8, 3), dtype=np.int32))
    d_c = devmem.DeviceArray(np.zeros(3, dtype=np.int64))
    ok_o, ok_d = [0, 0, 0], [4, 4, 4]
    bad = [([0, 0, 0], [0, 4, 4], 4, 1),
           ([0, 0, 0], [4, -1, 4], 4, 1),
           ([0, 0, 0], [4, 4, 1025], 4, 1),
           ([0, 0, 0], [1024, 1024, 129], 4, 1),                # 2^27 + 2^20 voxels
           ([-32769, 0, 0], [4, 4, 4], 4, 1),
           ([0, 32765, 0], [4, 4, 4], 4, 1),                    # the last voxel beyond the int16 range
           (ok_o, ok_d, 4, 0),
           (ok_o, ok_d, 4, 256),
           (ok_o, ok_d, 0, 1),                                  # the factor
           (ok_o, ok_d, 1, 1),
           (ok_o, ok_d, 3, 1),
           (ok_o, ok_d, 16, 1),
           (ok_o, ok_d, -4, 1)]
    for origin, dims, k, mw in bad:
        with pytest.raises(ratsdf.RatsdfError) as ei:
            e.cluster_mesh(origin, dims, k, mw)
        assert ei.value.status == 1, (origin, dims, k, mw)
        with pytest.raises(ratsdf.RatsdfError) as ei:
            e.cluster_mesh_device(origin, dims, d_v, 8, d_t, 8, d_c, k, mw)
        assert ei.value.status == 1, (origin, dims, k, mw)
    fn, fd = e.lib.fn["cluster_mesh"], e.lib.fn["cluster_mesh_device"]
    box = [(C.c_int32 * 3)(*v) for v in (ok_o, ok_d)]
    ok = ClusterMeshParams(1, 4, 0, 0)
    pv, pt, nv, nt = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
    out = (C.byref(pv), C.byref(nv), C.byref(pt), C.byref(nt))
    dev = (d_v.data_ptr(), 8, d_t.data_ptr(), 8, d_c.data_ptr())
    for params in (ClusterMeshParams(1, 4, 1, 0), ClusterMeshParams(1, 4, 0, 1), None):   # flags, reserved, NULL
        ref_ = C.byref(params) if params is not None else None
        assert fn(e._h, *box, ref_, *out) == 1
        assert fd(e._h, *box, ref_, *dev) == 1
    assert fn(e._h, None, box[1], C.byref(ok), *out) == 1                   # NULL origin / dims / outputs / handle
    assert fn(e._h, box[0], None, C.byref(ok), *out) == 1
    for i in range(4):
        assert fn(e._h, *box, C.byref(ok), *[None if j == i else o for j, o in enumerate(out)]) == 1
    assert fn(None, *box, C.byref(ok), *out) == 1
    assert fd(None, *box, C.byref(ok), *dev) == 1
    assert fd(e._h, None, box[1], C.byref(ok), *dev) == 1
    assert fd(e._h, box[0], None, C.byref(ok), *dev) == 1
    assert fd(e._h, *box, C.byref(ok), dev[0], -1, dev[2], 8, dev[4]) == 1  # negative capacities
    assert fd(e._h, *box, C.byref(ok), dev[0], 8, dev[2], -1, dev[4]) == 1
    assert fd(e._h, *box, C.byref(ok), None, 1, dev[2], 8, dev[4]) == 1     # NULL buffers with a capacity
    assert fd(e._h, *box, C.byref(ok), dev[0], 8, None, 1, dev[4]) == 1
    assert fd(e._h, *box, C.byref(ok), dev[0] + 8, 4, dev[2], 8, dev[4]) == 1   # misaligned buffers
    assert fd(e._h, *box, C.byref(ok), dev[0], 8, dev[2] + 2, 4, dev[4]) == 1
    assert fd(e._h, *box, C.byref(ok), dev[0], 8, dev[2], 8, None) == 1     # NULL / misaligned counts
    assert fd(e._h, *box, C.byref(ok), dev[0], 8, dev[2], 8, dev[4] + 4) == 1
    e.synchronize()
    assert (d_v.numpy() == 0).all() and (d_t.numpy() == 0).all() and (d_c.numpy() == 0).all()   # nothing launched
    # the limits themselves are accepted; an empty mesh is two NULLs and two zeros
    for origin, dims in (([-32768, 32767 - 3, 0], [1, 4, 1024]), ([32767, 32767, 32767], [1, 1, 1])):
        for k in FACTORS:
            v, tri = e.cluster_mesh(origin, dims, k, 255)
            assert len(v) == 0 and tri.shape == (0, 3)
    pv.value, pt.value, nv.value, nt.value = 1, 1, 7, 7
    assert fn(e._h, *box, C.byref(ok), *out) == 0
    assert pv.value is None and pt.value is None and nv.value == 0 and nt.value == 0
    assert fd(e._h, *box, C.byref(ok), dev[0], 8, dev[2] + 4, 4, dev[4] + 8) == 0   # 4- and 8-byte alignment suffice
    assert e.cluster_mesh_device(ok_o, ok_d, 0, 0, 0, 0, d_c) == (0, 0)
