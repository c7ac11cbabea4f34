"""The welded surface mesh of the HIP engine (include/ratsdf_surface_mesh.h) against the numpy restatement of its
contract (tests/surface_mesh_ref.py): vertices byte for byte, triangles equal as arrays.  Crafted maps brought in with
import_blocks (spheres across block seams and block 0 / -1, noise with all 256 cases, weights and fresh voxels, the ends
of the grid, a lone block, an empty box, a sparse box of more than one scan tile, chained directories), the capacity
rule of the device form, tiling, the mesh's own properties, a map built from real frames, and the read-only / error
behaviour."""
import ctypes as C

import numpy as np
import pytest

import mesh_cases
import surface_mesh_ref as mref
import surface_ref as ref
from ratsdf import synthetic

pytestmark = pytest.mark.gpu

VS, TRUNC = 0.02, 0.12
SMALL = dict(block_bits=10)        # crafted maps hold a handful of blocks
CENTRE, RADIUS = (3.21, -5.43, 14.69), 9.1
LO, HI = (-2, -3, 0), (2, 1, 3)
ORIGIN, DIMS = [-9, -18, 2], [25, 26, 25]        # not block aligned; blocks -2 .. 1, -3 .. 0, 0 .. 3
SPLIT = [3, -6, 13]


def _engine(make_engine, arrays, **kw):
    e = make_engine(VS, TRUNC, **(kw or SMALL))
    e.import_blocks(*arrays)
    return e, ref.blocks_of(*arrays)


def _check(e, blocks, origin, dims, min_weight=1, vs=VS):
    v, tri = e.surface_mesh(origin, dims, min_weight)
    wv, wt = mref.surface_mesh(blocks, origin, dims, vs, min_weight)
    print(f"box {list(origin)} {list(dims)} min_weight {min_weight}: {len(v)} vertices, {len(tri)} triangles; "
          f"restatement {len(wv)}, {len(wt)}")
    assert tri.dtype == np.int32 and tri.shape == wt.shape and np.array_equal(tri, wt), (origin, dims, min_weight)
    assert ref.same_bytes(v, wv), (origin, dims, min_weight, len(v), len(wv))
    return v, tri


@pytest.fixture(scope="module")
def sphere():
    return tuple(mref.sphere_blocks(CENTRE, RADIUS, LO, HI))


# ---- 1. spheres ------------------------------------------------------------------------------------------------
def test_sphere_across_block_seams_closed_and_oriented(make_engine, sphere):
    e, blocks = _engine(make_engine, sphere)
    v, tri = _check(e, blocks, ORIGIN, DIMS)
    assert len(tri) > 1000
    mref.assert_closed(tri, len(v))                          # the properties, on the engine's own output
    mref.assert_oriented(v, tri, CENTRE, VS)
    points = e.surface_points(ORIGIN, [d + 1 for d in DIMS])
    mref.assert_subsequence(v, points)
    cut = _check(e, blocks, ORIGIN, [8, 26, 25])[0]          # a box that cuts the sphere open
    points = e.surface_points(ORIGIN, [9, 27, 26])
    assert 0 < len(cut) < len(points)
    mref.assert_subsequence(cut, points)


def test_sphere_at_negative_coordinates(make_engine):
    centre = (-1.79, -3.43, -2.31)                           # straddles block 0 / -1 on every axis
    e, blocks = _engine(make_engine, tuple(mref.sphere_blocks(centre, RADIUS, (-2, -3, -2), (1, 1, 1))))
    v, tri = _check(e, blocks, [-14, -17, -15], [25, 27, 26])
    mref.assert_closed(tri, len(v))
    mref.assert_oriented(v, tri, centre, VS)
    # the shell of mesh_cases' kind: voxels more than six from the surface are unobserved
    m = mesh_cases.rc.sphere_shell(centre, RADIUS)
    e, blocks = _engine(make_engine, tuple(m))
    v, tri = _check(e, blocks, [-14, -17, -15], [25, 27, 26])
    mref.assert_closed(tri, len(v))


def test_tiling(make_engine, sphere):
    e, blocks = _engine(make_engine, sphere)
    whole = _check(e, blocks, ORIGIN, DIMS)
    o, d, s = np.array(ORIGIN), np.array(DIMS), np.array(SPLIT)
    rows, seen = [], {}
    for k in range(8):
        up = np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1], dtype=bool)
        v, tri = _check(e, blocks, np.where(up, s, o), np.where(up, o + d - s, s - o))
        assert len(tri) > 0 and len(np.unique(tri)) == len(v)
        rows.append(mref.triangle_rows(v, tri))
        for r in v:                                          # a vertex two boxes share has identical bytes
            key = r["pos"].tobytes()
            assert seen.setdefault(key, r.tobytes()) == r.tobytes()
    rows = np.concatenate(rows)
    rows = rows[np.lexsort(rows.T[::-1])]
    want = mref.triangle_rows(*whole)
    assert rows.shape == want.shape and np.array_equal(rows, want)
    assert len(seen) == len(whole[0])


# ---- 2. noise: all 256 cases -----------------------------------------------------------------------------------
def test_noise_map_with_all_cases(make_engine):
    m = mesh_cases.noise_blocks()                            # (asserts that cells of weight > 10 show every case)
    e, blocks = _engine(make_engine, tuple(m))
    lo = np.array(mesh_cases.NOISE_OFFSET) * 8
    n = np.array(mesh_cases.NOISE_EXTENT) * 8
    v, tri = _check(e, blocks, lo - 1, n + 2, min_weight=11)
    assert len(tri) > 10000
    _check(e, blocks, lo - 1, n + 2, min_weight=1)
    _check(e, blocks, lo + 3, n - 5, min_weight=10)
    # a block whose six neighbours (all 26) are absent
    one = mesh_cases.single_block()
    e, blocks = _engine(make_engine, tuple(one))
    b0 = one.pos[0].astype(int) * 8
    v, tri = _check(e, blocks, b0 - 3, [14, 14, 14], min_weight=11)
    assert len(tri) > 100
    _check(e, blocks, b0, [8, 8, 8], min_weight=11)


# ---- 3. weights and fresh voxels -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_map():
    rng = np.random.default_rng(11)
    arrays = ref.solid((-2, -1, 0), (1, 2, 3), lambda x, y, z: rng.uniform(-1, 1, x.shape))
    keep = np.flatnonzero(rng.random(64) < 0.6)
    arrays = tuple(a[keep] for a in arrays)
    pos, t, c, p = arrays
    c["weight"] = rng.choice([0, 1, 1, 2, 3, 200, 255, 255, 255], size=t.shape)
    p[:] = rng.random(t.shape, dtype=np.float32)
    t[rng.random(t.shape) < 0.03] = -1.0                    # fresh voxels where the weight is 1
    t[rng.random(t.shape) < 0.02] = 0.0                     # triangles of zero area
    t[rng.random(t.shape) < 0.01] = -0.0
    return arrays


def test_min_weight_and_fresh_voxels(make_engine, random_map):
    e, blocks = _engine(make_engine, random_map)
    pos, t, c, p = random_map
    assert ((c["weight"] == 1) & (t == -1.0)).sum() > 50
    box = ([-17, -9, -1], [34, 34, 34])
    n1 = len(_check(e, blocks, *box, min_weight=1)[1])
    n2 = len(_check(e, blocks, *box, min_weight=2)[1])
    n255 = len(_check(e, blocks, *box, min_weight=255)[1])
    assert n1 > n2 > n255 > 0
    _check(e, blocks, [-13, -5, 3], [22, 27, 19], min_weight=3)


# ---- 4. the ends of the grid -----------------------------------------------------------------------------------
def test_ends_of_the_voxel_range(make_engine):
    rng = np.random.default_rng(5)
    noise = lambda x, y, z: rng.uniform(-1, 1, x.shape)
    top = ref.solid((4094, 4095, 4095), (4095, 4095, 4095), noise)
    low = ref.solid((-4096, -4096, -4096), (-4096, -4096, -4095), noise)
    e, blocks = _engine(make_engine, tuple(np.concatenate([a, b]) for a, b in zip(top, low)))
    v, tri = _check(e, blocks, [32760, 32760, 32760], [8, 8, 8])            # origin + dims == 32768: no such voxel
    assert len(tri) > 500
    _check(e, blocks, [32750, 32757, 32767], [18, 11, 1])
    _check(e, blocks, [32752, 32700, 32760], [15, 68, 8])                   # the owners reach 32767 on x: no more
    v, tri = _check(e, blocks, [-32768, -32768, -32768], [8, 8, 8])
    assert len(tri) > 500
    _check(e, blocks, [-32768, -32768, -32768], [1024, 9, 16])


# ---- 5. empty and sparse boxes ---------------------------------------------------------------------------------
def test_empty_box(make_engine, sphere):
    e, blocks = _engine(make_engine, sphere)
    v, tri = _check(e, blocks, [500, 500, 500], [20, 9, 40])
    assert len(v) == 0 and tri.shape == (0, 3)
    v, tri = _check(e, blocks, [-16, -24, 0], [8, 8, 8])                    # blocks, but no surface
    assert len(v) == 0 and tri.shape == (0, 3)


def test_sparse_box_of_more_than_one_scan_tile(make_engine):
    a = mref.sphere_blocks((11.3, 12.2, 10.4), 4.3, (0, 0, 0), (2, 2, 2))
    b = mref.sphere_blocks((123.6, 121.1, 124.7), 5.2, (14, 14, 14), (16, 16, 16))
    e, blocks = _engine(make_engine, tuple(np.concatenate([x, y]) for x, y in zip(a, b)))
    v, tri = _check(e, blocks, [0, 0, 0], [136, 136, 136])                  # 18^3 cells of the owners' block grid
    assert 18 ** 3 > 4096 and len(tri) > 500
    p = v["pos"][tri][:, 0, 0]
    assert (p < 1.0).any() and (p > 2.0).any()                              # both shells
    _check(e, blocks, [1, 2, 3], [20, 20, 20])                              # the workspace stays laid out for 18^3


# ---- 6. chained directories ------------------------------------------------------------------------------------
def test_chained_directories(make_engine):
    """query_cases' tiny_table (200 blocks in 512 buckets: blocks at the end of chains) and known_order (the block
    behind the table-end wrap), loaded with ratsdf_test_allocate as the read-out cases load them; the voxels are noise
    of weights 1 .. 3 with a few unobserved ones (the read-out cases' own values leave no cell complete)"""
    import query_cases as qc
    import readout_cases as rcs
    from kat_cases import ref_hash
    rng = np.random.default_rng(23)
    for name, map_name, origin, dims, _ in rcs.SURFACE_BOXES:
        m = rcs.get_map(map_name)
        pos = m.blocks.pos
        t = rng.uniform(-1, 1, (len(pos), 512)).astype(np.float32)
        c = np.zeros(t.shape, dtype=ref.RGBW)
        c["weight"] = rng.choice([0, 1, 2, 3], p=[0.02, 0.18, 0.4, 0.4], size=t.shape)
        c["r"] = rng.integers(0, 256, t.shape)
        arrays = qc.BlockSet(pos, t, c.view(m.blocks.rgbw.dtype), rng.random(t.shape, dtype=np.float32))
        e = make_engine(rcs.VS, rcs.TRUNC, **m.engine)
        qc.load(e, arrays)
        if map_name == "tiny_table":    # blocks that only a chain walk finds
            ei, bl = e.dump_directory()
            home = np.array([ref_hash(p, m.engine["bucket_bits"]) for p in qc.directory_positions(bl)])
            assert ((ei >> 1) != home).sum() >= 20
        blocks = ref.blocks_of(*arrays)
        for min_weight in (1, 2):
            v, tri = _check(e, blocks, origin, dims, min_weight, vs=rcs.VS)
            assert len(tri) > 50, (name, min_weight)


# ---- 7. the device form ----------------------------------------------------------------------------------------
def test_truncation_in_the_device_form(make_engine, random_map):
    import torch
    from ratsdf import devmem
    e, blocks = _engine(make_engine, random_map)
    box = ([-17, -9, -1], [34, 34, 34])
    wv, wt = mref.surface_mesh(blocks, *box, VS)
    nv, nt = len(wv), len(wt)
    assert nv > 2000 and nt > 2000
    counts = devmem.DeviceArray(np.full(3, -1, dtype=np.int64))
    assert e.surface_mesh_device(*box, 0, 0, 0, 0, counts) == (nv, nt)       # a pure count
    assert counts.numpy().tolist() == [nv, nt, -1]
    guard = 0x5A5A5A5A
    for vcap, tcap in ((nv // 2, nt // 2), (nv, nt), (nv // 2, nt), (nv, nt // 2), (0, nt), (nv + 3, nt + 3)):
        d_v = devmem.DeviceArray(np.full((vcap + 4, 8), guard, dtype=np.int32))
        d_t = devmem.DeviceArray(np.full((tcap + 4, 3), guard, dtype=np.int32))
        assert e.surface_mesh_device(*box, d_v, vcap, d_t, tcap, counts) == (nv, nt)
        gv, gt = d_v.numpy(), d_t.numpy()
        kv, kt = min(vcap, nv), min(tcap, nt)
        assert ref.same_bytes(gv[:kv].reshape(-1).view(np.uint8), np.ascontiguousarray(wv[:kv]).view(np.uint8))
        assert np.array_equal(gt[:kt], wt[:kt]), (vcap, tcap)                # indices beyond vcap are kept
        assert np.all(gv[kv:] == guard) and np.all(gt[kt:] == guard), (vcap, tcap)
        if vcap < nv and kt:
            assert gt[:kt].max() >= vcap
    d_v = devmem.DeviceArray(np.full((8, 8), guard, dtype=np.int32))
    d_t = devmem.DeviceArray(np.full((8, 3), guard, dtype=np.int32))
    assert e.surface_mesh_device(*box, d_v, 0, d_t, 0, counts) == (nv, nt)   # capacity 0 with buffers
    assert np.all(d_v.numpy() == guard) and np.all(d_t.numpy() == guard)
    t_v = torch.zeros((nv, 8), dtype=torch.int32, device="cuda")            # torch tensors
    t_t = torch.zeros((nt, 3), dtype=torch.int32, device="cuda")
    t_c = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert e.surface_mesh_device(*box, t_v, nv, t_t, nt, t_c) == (nv, nt)
    assert ref.same_bytes(t_v.cpu().numpy().reshape(-1).view(np.uint8), wv.view(np.uint8))
    assert np.array_equal(t_t.cpu().numpy(), wt)


# ---- 8. after real frames --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room():
    return synthetic.stream("room", 4, scale=0.25, noise=True, holes=True)


def _integrate(e, frames):
    for f in frames:
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])


def _map_of(e):
    """the map's blocks for the restatement, and its bounding box in voxels"""
    from ratsdf import multi
    _, b = e.dump_directory()
    pos = np.stack([b["x"], b["y"], b["z"]], axis=1)
    lo, hi = pos.astype(int).min(0) * 8, pos.astype(int).max(0) * 8 + 7
    return ref.blocks_of(*multi.export_blocks(e, pos)), [int(v) for v in lo], [int(v) for v in hi - lo + 1]


def test_right_after_an_integrated_frame(make_engine, room):
    from ratsdf import devmem
    host = make_engine(VS, TRUNC)
    _integrate(host, room[:4])
    assert host.last_frame_stats()["deleted_blocks"] > 0
    blocks, origin, dims = _map_of(host)
    wv, wt = _check(host, blocks, origin, dims)
    assert len(wt) > 1000
    # right after a carving frame, without a synchronisation in between: the deferred pool releases come first
    dev = make_engine(VS, TRUNC)
    _integrate(dev, room[:3])
    f = room[3]
    bufs = [devmem.DeviceArray(np.ascontiguousarray(f[k])) for k in ("rgb", "depth", "ht", "lt")]
    batch = dev.make_batch([bufs[0].data_ptr()], [bufs[1].data_ptr()], [bufs[2].data_ptr()], [bufs[3].data_ptr()],
                           f["height"], f["width"], 4.0, [f["intrinsics"]], [f["pose"]])
    d_v = devmem.DeviceArray(np.zeros((len(wv), 8), dtype=np.int32))
    d_t = devmem.DeviceArray(np.zeros((len(wt), 3), dtype=np.int32))
    d_c = devmem.DeviceArray(np.zeros(2, dtype=np.int64))
    dev.integrate_device_batch(batch)
    assert dev.surface_mesh_device(origin, dims, d_v, len(wv), d_t, len(wt), d_c) == (len(wv), len(wt))
    assert ref.same_bytes(d_v.numpy().reshape(-1).view(np.uint8), wv.view(np.uint8))
    assert np.array_equal(d_t.numpy(), wt)


# ---- 9. read-only and errors -----------------------------------------------------------------------------------
def _snapshot(e):
    ei, blocks = e.dump_directory()
    nf, heap = e.dump_heap()
    t, c, p = e.dump_voxels(blocks["idx"])
    return ei, blocks, nf, heap[:nf].copy(), t, c, p


def test_the_map_is_only_read(make_engine, room):
    from ratsdf import devmem
    e = make_engine(VS, TRUNC)
    _integrate(e, room[:2])
    _, origin, dims = _map_of(e)
    before = _snapshot(e)
    v, tri = e.surface_mesh(origin, dims)
    assert len(tri) > 0
    d_c = devmem.DeviceArray(np.zeros(2, dtype=np.int64))
    assert e.surface_mesh_device(origin, dims, 0, 0, 0, 0, d_c) == (len(v), len(tri))
    e.surface_mesh(origin, dims, 2)
    after = _snapshot(e)
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
        small.surface_mesh([0, 0, 0], [8, 8, 8])
    assert ei.value.status == 3
    d_c = devmem.DeviceArray(np.zeros(2, dtype=np.int64))
    with pytest.raises(ratsdf.RatsdfError) as ei:
        small.surface_mesh_device([0, 0, 0], [8, 8, 8], 0, 0, 0, 0, d_c)
    assert ei.value.status == 3


def test_bad_arguments(make_engine):
    import ratsdf
    from ratsdf import devmem
    from ratsdf._abi import SurfaceMeshParams
    e = make_engine(VS, TRUNC, **SMALL)
    d_v = devmem.DeviceArray(np.zeros((8, 8), dtype=np.int32))
    d_t = devmem.DeviceArray(np.zeros((8, 3), dtype=np.int32))
    d_c = devmem.DeviceArray(np.zeros(3, dtype=np.int64))
    ok_o, ok_d = [0, 0, 0], [4, 4, 4]
    bad = [([0, 0, 0], [0, 4, 4], 1),
           ([0, 0, 0], [4, -1, 4], 1),
           ([0, 0, 0], [4, 4, 1025], 1),
           ([0, 0, 0], [1024, 1024, 129], 1),                   # 2^27 + 2^20 voxels
           ([-32769, 0, 0], [4, 4, 4], 1),
           ([0, 32765, 0], [4, 4, 4], 1),                       # the last voxel beyond the int16 range
           ([0, 0, 40000], [4, 4, 4], 1),
           (ok_o, ok_d, 0),
           (ok_o, ok_d, -3),
           (ok_o, ok_d, 256)]
    for origin, dims, mw in bad:
        with pytest.raises(ratsdf.RatsdfError) as ei:
            e.surface_mesh(origin, dims, mw)
        assert ei.value.status == 1, (origin, dims, mw)
        with pytest.raises(ratsdf.RatsdfError) as ei:
            e.surface_mesh_device(origin, dims, d_v, 8, d_t, 8, d_c, mw)
        assert ei.value.status == 1, (origin, dims, mw)
    fn, fd = e.lib.fn["surface_mesh"], e.lib.fn["surface_mesh_device"]
    box = [(C.c_int32 * 3)(*v) for v in (ok_o, ok_d)]
    ok = SurfaceMeshParams(1, 0, 0, 0)
    pv, pt, nv, nt = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
    out = (C.byref(pv), C.byref(nv), C.byref(pt), C.byref(nt))
    dev = (d_v.data_ptr(), 8, d_t.data_ptr(), 8, d_c.data_ptr())
    for params in (SurfaceMeshParams(1, 1, 0, 0), SurfaceMeshParams(1, 0, 1, 0), SurfaceMeshParams(1, 0, 0, 1), None):
        ref_ = C.byref(params) if params is not None else None              # flags, reserved words, NULL params
        assert fn(e._h, *box, ref_, *out) == 1
        assert fd(e._h, *box, ref_, *dev) == 1
    assert fn(e._h, None, box[1], C.byref(ok), *out) == 1                   # NULL origin / dims / outputs / handle
    assert fn(e._h, box[0], None, C.byref(ok), *out) == 1
    for k in range(4):
        assert fn(e._h, *box, C.byref(ok), *[None if i == k else o for i, o in enumerate(out)]) == 1
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
    assert (d_v.numpy() == 0).all() and (d_t.numpy() == 0).all() and (d_c.numpy() == 0).all()   # nothing launched
    # the limits themselves are accepted; an empty mesh is two NULLs and two zeros
    for origin, dims in (([-32768, 32767 - 3, 0], [1, 4, 1024]), ([0, 0, 0], [1024, 1024, 1]),
                         ([32767, 32767, 32767], [1, 1, 1])):
        v, tri = e.surface_mesh(origin, dims, 255)
        assert len(v) == 0 and tri.shape == (0, 3)
    pv.value, pt.value, nv.value, nt.value = 1, 1, 7, 7
    assert fn(e._h, *box, C.byref(ok), *out) == 0
    assert pv.value is None and pt.value is None and nv.value == 0 and nt.value == 0
    assert fd(e._h, *box, C.byref(ok), dev[0], 8, dev[2] + 4, 4, dev[4] + 8) == 0   # 4- and 8-byte alignment suffice
    assert e.surface_mesh_device(ok_o, ok_d, 0, 0, 0, 0, d_c) == (0, 0)
