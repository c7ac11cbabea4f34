"""The oriented surface points of the HIP engine (include/ratsdf_surface.h) against the numpy restatement of their
contract (tests/surface_ref.py), byte for byte: crafted maps brought in with import_blocks (one block, seams between
blocks with and without the neighbour, boxes, filters and ties, a random map), the capacity rule of the device form,
a map built from real frames, and the read-only / error behaviour."""
import ctypes as C

import numpy as np
import pytest

import surface_ref as ref
from ratsdf import synthetic

pytestmark = pytest.mark.gpu

VS, TRUNC = 0.02, 0.12
SMALL = dict(block_bits=10)        # crafted maps hold a handful of blocks


def _engine(make_engine, arrays, **kw):
    """an engine holding the blocks of `arrays` (import_blocks' four arrays), and the restatement's dict of them"""
    e = make_engine(VS, TRUNC, **(kw or SMALL))
    e.import_blocks(*arrays)
    return e, ref.blocks_of(*arrays)


def _check(e, blocks, origin, dims, min_weight=1, min_prob=0.0):
    got = e.surface_points(origin, dims, min_weight, min_prob)
    want = ref.surface_points(blocks, origin, dims, VS, min_weight, min_prob)
    print(f"box {list(origin)} {list(dims)} min_weight {min_weight} min_prob {min_prob}: {len(got)} points, "
          f"restatement {len(want)}")
    assert ref.same_bytes(got, want), (origin, dims, min_weight, min_prob, len(got), len(want))
    return got


def _pick(arrays, keep):
    return tuple(a[keep] for a in arrays)


def _checker(seed, lo=0.05, hi=1.0):
    """a field that changes sign between any two neighbouring voxels, with random magnitudes"""
    rng = np.random.default_rng(seed)
    return lambda x, y, z: np.where((x + y + z) % 2 == 0, 1, -1) * rng.uniform(lo, hi, x.shape)


def _set(arrays, voxel, tsdf=None, weight=None, prob=None):
    """edits one voxel (voxel index) of import_blocks' arrays in place"""
    pos, t, c, p = arrays
    v = np.asarray(voxel)
    i = int(np.flatnonzero(np.all(pos.astype(np.int64) == v >> 3, axis=1))[0])
    k = int((v[0] & 7) + 8 * (v[1] & 7) + 64 * (v[2] & 7))
    if tsdf is not None:
        t[i, k] = tsdf
    if weight is not None:
        c["weight"][i, k] = weight
    if prob is not None:
        p[i, k] = prob


def _at(rec, voxel, axis):
    """the records on edge (voxel, axis): the two other position components are the voxel's, the axis' in [v, v + 1)"""
    v = np.asarray(voxel, dtype=np.float32)
    m = np.ones(len(rec), dtype=bool)
    for b in range(3):
        if b == axis:
            m &= (rec["pos"][:, b] >= v[b] * np.float32(VS)) & (rec["pos"][:, b] < (v[b] + 1) * np.float32(VS))
        else:
            m &= rec["pos"][:, b] == v[b] * np.float32(VS)
    return rec[m]


# ---- 1. one block ----------------------------------------------------------------------------------------------
def test_one_block_plane_and_order(make_engine):
    for axis in range(3):
        e, blocks = _engine(make_engine, ref.solid((0, 0, 0), (0, 0, 0), lambda *g: (g[axis] - 3.25) / 8.0))
        got = _check(e, blocks, [0, 0, 0], [8, 8, 8])
        assert len(got) == 64 and np.all(got["pos"][:, axis] == np.float32(3.25) * np.float32(VS))
        n = np.zeros(3, dtype=np.float32)
        n[axis] = 1
        assert np.all(got["normal"] == n)
    e, blocks = _engine(make_engine, ref.solid((0, 0, 0), (0, 0, 0), _checker(1)))
    got = _check(e, blocks, [0, 0, 0], [8, 8, 8])
    assert len(got) == 3 * 64 * 7            # every edge inside the block, voxel by voxel, axis by axis


# ---- 2. seams --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_seam_owner_at_local_7(make_engine, axis):
    hi = [0, 0, 0]
    hi[axis] = 1
    dims = [8, 8, 8]
    dims[axis] = 16
    arrays = ref.solid((0, 0, 0), hi, lambda *g: (7.5 - g[axis]) / 8.0)
    e, blocks = _engine(make_engine, arrays)
    got = _check(e, blocks, [0, 0, 0], dims)
    assert len(got) == 64 and np.all(got["pos"][:, axis] == np.float32(7.5) * np.float32(VS))
    _check(e, blocks, [0, 0, 0], [8, 8, 8])                     # the upper endpoint outside the box
    # the next block absent: nothing crosses
    e, blocks = _engine(make_engine, _pick(arrays, [0]))
    assert len(_check(e, blocks, [0, 0, 0], dims)) == 0


def test_seams_read_two_voxels_into_the_next_block_and_one_below(make_engine):
    # crossings on every edge: owners at local 6 and 7 (d_a of the upper endpoint reads local 0 and 1 of the next
    # block), at local 0 (d_a of the lower endpoint reads local 7 of the block below)
    arrays = ref.solid((-1, -1, -1), (1, 1, 1), _checker(2))
    e, blocks = _engine(make_engine, arrays)
    got = _check(e, blocks, [-8, -8, -8], [24, 24, 24])
    assert len(got) == 3 * 24 * 24 * 23
    _check(e, blocks, [0, 0, 0], [8, 8, 8])


@pytest.mark.parametrize("missing", range(7))
def test_seams_with_absent_neighbours_fall_back(make_engine, missing):
    # the centre block and its six face neighbours, one of them (or, missing == 6, all of them) left out: one-sided
    # differences, zero differences and no crossing into the absent block
    arrays = ref.solid((-1, -1, -1), (1, 1, 1), _checker(3))
    pos = arrays[0].astype(int)
    face = np.abs(pos).sum(1) == 1
    keep = np.flatnonzero(face | (np.abs(pos).sum(1) == 0))
    faces = np.flatnonzero(face)
    drop = set(faces) if missing == 6 else {faces[missing]}
    e, blocks = _engine(make_engine, _pick(arrays, [i for i in keep if i not in drop]))
    _check(e, blocks, [-8, -8, -8], [24, 24, 24])
    got = _check(e, blocks, [0, 0, 0], [8, 8, 8])
    if missing == 6:
        assert len(got) == 3 * 64 * 7


# ---- 3. boxes --------------------------------------------------------------------------------------------------
def test_boxes(make_engine):
    arrays = ref.solid((-3, -2, -2), (0, 0, 0), _checker(4))
    e, blocks = _engine(make_engine, arrays)
    whole = _check(e, blocks, [-24, -16, -16], [32, 24, 24])               # negative block coordinates
    _check(e, blocks, [-21, -13, -15], [19, 17, 14])                       # not aligned to blocks
    _check(e, blocks, [-30, -20, -20], [45, 33, 31])                       # sticks out of the map
    for dims in ([1, 24, 24], [32, 1, 24], [32, 24, 1], [1, 1, 1]):       # one voxel wide
        _check(e, blocks, [-9, -8, -1], dims)
    # an owner in the box whose neighbour lies outside it: the edge is the owner's
    one = _check(e, blocks, [-9, -9, -9], [1, 1, 1])
    assert len(one) == 3
    # two adjacent boxes tile: no duplicates, no gaps
    for axis, cut in ((0, -9), (1, -8), (2, -3)):
        o2, d1, d2 = [-24, -16, -16], [32, 24, 24], [32, 24, 24]
        d1[axis] = cut - o2[axis]
        d2[axis] -= d1[axis]
        o2[axis] = cut
        parts = np.concatenate([_check(e, blocks, [-24, -16, -16], d1), _check(e, blocks, o2, d2)])
        rows = lambda r: np.ascontiguousarray(r).view(np.uint8).reshape(len(r), 32)
        a, b = rows(parts), rows(whole)
        assert len(np.unique(a, axis=0)) == len(a)
        assert np.array_equal(a[np.lexsort(a.T)], b[np.lexsort(b.T)])
    assert len(_check(e, blocks, [500, 500, 500], [20, 9, 40])) == 0       # no allocated block


def test_ends_of_the_voxel_range(make_engine):
    top = ref.solid((4095, 4095, 4095), (4095, 4095, 4095), _checker(5))
    low = ref.solid((-4096, -4096, -4096), (-4096, -4096, -4096), _checker(6))
    e, blocks = _engine(make_engine, tuple(np.concatenate([a, b]) for a, b in zip(top, low)))
    got = _check(e, blocks, [32760, 32760, 32760], [8, 8, 8])               # voxel 32767 has no upper neighbour
    assert len(got) == 3 * 64 * 7
    _check(e, blocks, [32767, 32767, 32767], [1, 1, 1])
    _check(e, blocks, [32000, 32700, 32760], [768, 68, 8])
    got = _check(e, blocks, [-32768, -32768, -32768], [8, 8, 8])
    assert len(got) == 3 * 64 * 7
    _check(e, blocks, [-32768, -32768, -32768], [1024, 16, 9])


# ---- 4. filters and ties ---------------------------------------------------------------------------------------
def test_filters_and_ties(make_engine):
    arrays = ref.solid((0, 0, 0), (1, 0, 0), lambda x, y, z: np.full(x.shape, 0.5))
    pos, t, c, p = arrays
    p[:] = (0.25 + np.arange(p.size, dtype=np.float32).reshape(p.shape) / np.float32(4096))
    _set(arrays, (2, 1, 1), tsdf=-0.5, weight=2)             # min_weight at, above, below its weight
    _set(arrays, (5, 1, 1), tsdf=-0.5, weight=0)             # never observed
    _set(arrays, (2, 4, 1), tsdf=-1.0, weight=1)             # the fresh voxel next to positive ones
    _set(arrays, (5, 4, 1), tsdf=-1.0, weight=2)             # -1 with another weight is a voxel like any other
    _set(arrays, (2, 1, 4), tsdf=0.0)                        # t0 == 0: f = 0, the lower endpoint
    _set(arrays, (3, 1, 4), tsdf=-0.5)
    _set(arrays, (2, 4, 4), tsdf=-0.0)                       # -0 is not negative
    _set(arrays, (3, 4, 4), tsdf=-0.5)
    _set(arrays, (2, 6, 6), tsdf=0.375)                      # t0 == -t1: f = 0.5, the upper endpoint
    _set(arrays, (3, 6, 6), tsdf=-0.375)
    _set(arrays, (7, 6, 2), tsdf=0.25)                       # the same tie across the seam
    _set(arrays, (8, 6, 2), tsdf=-0.25)
    e, blocks = _engine(make_engine, arrays)
    box = ([0, 0, 0], [16, 8, 8])
    w1 = _check(e, blocks, *box, min_weight=1)
    w2 = _check(e, blocks, *box, min_weight=2)
    w3 = _check(e, blocks, *box, min_weight=3)
    assert len(w1) == len(w2) == len(w3) + 12                # (2,1,1) and (5,4,1): six edges each
    assert len(_at(w1, (1, 4, 1), 0)) == 0 and len(_at(w1, (2, 4, 1), 0)) == 0      # fresh: no point
    assert len(_at(w1, (4, 1, 1), 0)) == 0 and len(_at(w1, (5, 1, 1), 0)) == 0      # weight 0: no point
    assert len(_at(w3, (1, 1, 1), 0)) == 0 and len(_at(w2, (1, 1, 1), 0)) == 1
    r = _at(w1, (2, 1, 4), 0)                                # f = 0
    assert len(r) == 1 and r["pos"][0, 0] == np.float32(2) * np.float32(VS) and r["rgbw"]["r"][0] == 2
    r = _at(w1, (2, 4, 4), 0)                                # t0 = -0.0 against a negative neighbour crosses, f = -0
    assert len(r) == 1 and r["rgbw"]["r"][0] == 2 and r["pos"][0, 0] == np.float32(2) * np.float32(VS)
    assert len(_at(w1, (1, 4, 4), 0)) == 0                   # ... and against the positive one below it does not
    r = _at(w1, (2, 6, 6), 0)                                # f = 0.5
    assert len(r) == 1 and r["pos"][0, 0] == np.float32(2.5) * np.float32(VS) and r["rgbw"]["r"][0] == 3
    r = _at(w1, (7, 6, 2), 0)
    assert len(r) == 1 and r["pos"][0, 0] == np.float32(7.5) * np.float32(VS) and r["rgbw"]["r"][0] == 8
    # min_prob exactly at a point's probability keeps it, the next float above drops it
    pr = np.sort(w1["prob"])[len(w1) // 2]
    at = _check(e, blocks, *box, min_prob=float(pr))
    above = _check(e, blocks, *box, min_prob=float(np.nextafter(pr, np.float32(1))))
    assert (at["prob"] == pr).sum() >= 1 and (above["prob"] == pr).sum() == 0
    assert len(above) == (w1["prob"] > pr).sum() and len(at) == (w1["prob"] >= pr).sum()


# ---- 5. a random map -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_map():
    rng = np.random.default_rng(11)
    arrays = ref.solid((-2, -1, 0), (1, 2, 3), lambda x, y, z: rng.uniform(-1, 1, x.shape))
    arrays = _pick(arrays, np.flatnonzero(rng.random(64) < 0.6))
    pos, t, c, p = arrays
    c["weight"] = rng.choice([0, 1, 1, 2, 3, 200, 255], size=t.shape)
    p[:] = rng.random(t.shape, dtype=np.float32)
    t[rng.random(t.shape) < 0.03] = -1.0                    # fresh voxels where the weight is 1
    t[rng.random(t.shape) < 0.02] = 0.0
    return arrays


def test_random_map(make_engine, random_map):
    e, blocks = _engine(make_engine, random_map)
    assert 24 <= len(blocks) <= 56
    got = _check(e, blocks, [-17, -9, -1], [34, 34, 34])
    assert len(got) > 5000
    _check(e, blocks, [-16, -8, 0], [32, 32, 32], min_weight=2)
    _check(e, blocks, [-13, -5, 3], [22, 27, 19], min_weight=3, min_prob=0.3)
    _check(e, blocks, [-17, -9, -1], [34, 34, 34], min_weight=255, min_prob=0.9)


def test_workspace_grows_then_a_small_box_again(make_engine, random_map):
    # one engine, its workspace laid out for a few cells, then for 17^3 = 4913 (the scan takes two tiles of 4096), then
    # used by boxes far smaller than what it was laid out for.  The map: the random blocks at z 0 .. 3 and a slab of
    # eight at z 14, 15, whose cells of the large box lie beyond 4096 (x fastest: 289 per layer of z, the box starts
    # at block z -1).
    far = ref.solid((3, 2, 14), (4, 3, 15), _checker(12))
    e, blocks = _engine(make_engine, tuple(np.concatenate([a, b]) for a, b in zip(random_map, far)))
    assert len(blocks) <= 64
    small = ([-13, -5, 3], [22, 27, 19])
    first = _check(e, blocks, *small)
    large = _check(e, blocks, [-64, -64, -8], [136, 136, 136])
    in_far = large["pos"][:, 2] >= np.float32(14 * 8) * np.float32(VS)
    assert len(first) > 100 and in_far.sum() > 1000 and (~in_far).sum() > 5000
    assert len(_check(e, blocks, [24, 16, 112], [8, 8, 8])) >= 3 * 64 * 7    # one block of the slab
    assert ref.same_bytes(_check(e, blocks, *small), first)


# ---- 6. capacity -----------------------------------------------------------------------------------------------
def test_capacity(make_engine, random_map):
    import torch
    e, blocks = _engine(make_engine, random_map)
    box = ([-17, -9, -1], [34, 34, 34])
    want = ref.surface_points(blocks, *box, VS)
    total = len(want)
    count = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert e.surface_points_device(*box, 0, 0, count) == total                 # a pure count
    assert count.cpu().tolist() == [total, 0]
    for cap in (1, 777, total - 1, total, total + 5):
        buf = torch.full((cap + 8, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        count.fill_(-1)
        assert e.surface_points_device(*box, buf, cap, count) == total
        assert count.cpu().tolist() == [total, -1]
        got = buf.cpu().numpy()
        n = min(cap, total)
        assert ref.same_bytes(got[:n].reshape(-1).view(np.uint8), np.ascontiguousarray(want[:n]).view(np.uint8))
        assert np.all(got[n:] == 0x5A5A5A5A), cap                             # nothing beyond min(total, capacity)
    buf = torch.full((16, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert e.surface_points_device(*box, buf, 0, count) == total               # capacity 0 with a buffer
    assert np.all(buf.cpu().numpy() == 0x5A5A5A5A)


# ---- 7. after real frames --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room():
    return synthetic.stream("room", 5, scale=0.25, noise=True, holes=True)


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


def test_after_real_frames(make_engine, room):
    import torch
    from ratsdf import devmem
    assert room[0]["depth"].shape == (120, 160)
    host = make_engine(VS, TRUNC)
    _integrate(host, room[:4])
    assert host.last_frame_stats()["deleted_blocks"] > 0
    blocks, origin, dims = _map_of(host)
    want = _check(host, blocks, origin, dims)
    assert len(want) > 1000
    _check(host, blocks, origin, dims, min_weight=2, min_prob=0.5)
    total = len(want)
    t_buf = torch.zeros((total, 8), dtype=torch.int32, device="cuda")
    t_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert host.surface_points_device(origin, dims, t_buf, total, t_cnt) == total
    assert ref.same_bytes(t_buf.cpu().numpy().reshape(-1).view(np.uint8), want.view(np.uint8))
    d_buf = devmem.DeviceArray(np.zeros((total, 8), dtype=np.int32))
    d_cnt = devmem.DeviceArray(np.zeros(1, dtype=np.int64))
    assert host.surface_points_device(origin, dims, d_buf, total, d_cnt) == total
    assert ref.same_bytes(d_buf.numpy().reshape(-1).view(np.uint8), want.view(np.uint8))
    # right after a carving frame, without a synchronisation in between: the deferred pool releases come first
    dev = make_engine(VS, TRUNC)
    _integrate(dev, room[:4])
    f = room[4]
    _integrate(host, [f])
    assert host.last_frame_stats()["deleted_blocks"] > 0
    blocks, origin, dims = _map_of(host)
    want = _check(host, blocks, origin, dims)
    bufs = [devmem.DeviceArray(np.ascontiguousarray(f[k])) for k in ("rgb", "depth", "ht", "lt")]
    batch = dev.make_batch([bufs[0].data_ptr()], [bufs[1].data_ptr()], [bufs[2].data_ptr()], [bufs[3].data_ptr()],
                           f["height"], f["width"], 4.0, [f["intrinsics"]], [f["pose"]])
    d_buf = devmem.DeviceArray(np.zeros((len(want) + 4, 8), dtype=np.int32))
    dev.integrate_device_batch(batch)
    assert dev.surface_points_device(origin, dims, d_buf, len(want) + 4, d_cnt) == len(want)
    assert ref.same_bytes(d_buf.numpy()[:len(want)].reshape(-1).view(np.uint8), want.view(np.uint8))
    assert ref.same_bytes(dev.surface_points(origin, dims), want)


# ---- 8. read-only and errors -----------------------------------------------------------------------------------
def _snapshot(e):
    """directory, free list, voxels, and the directory-delta record since the previous snapshot (rows sorted: the
    log of deleted positions is appended in no fixed order)"""
    from ratsdf import devmem
    ei, blocks = e.dump_directory()
    nf, heap = e.dump_heap()
    t, c, p = e.dump_voxels(blocks["idx"])
    cap = 1 << 15
    payload = devmem.DeviceArray(np.zeros((cap, 3), dtype=np.int32))
    counts = devmem.DeviceArray(np.zeros(2, dtype=np.int32))
    e.export_directory_delta_device(payload.data_ptr(), cap, counts.data_ptr())
    e.synchronize()
    n = counts.numpy()
    rows = payload.numpy()[:min(int(n[0]) + int(n[1] if n[1] != 0x7FFFFFFF else 0), cap)]
    return ei, blocks, nf, heap[:nf].copy(), t, c, p, n, rows[np.lexsort(rows.T)]


def _same(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y


def test_surface_points_are_read_only(make_engine, room):
    from ratsdf import devmem
    d_cnt = devmem.DeviceArray(np.zeros(1, dtype=np.int64))
    snaps = []
    for calls in (True, False):                              # the second engine makes no surface call
        e = make_engine(VS, TRUNC)
        _integrate(e, room[:2])
        _snapshot(e)                                         # (the first delta export switches the record on)
        _integrate(e, room[2:3])
        _, origin, dims = _map_of(e)
        if calls:
            assert len(e.surface_points(origin, dims)) > 0
            assert e.surface_points_device(origin, dims, 0, 0, d_cnt) > 0
        snaps.append(_snapshot(e))
        if calls:
            # ... and with nothing but surface calls in between, the map is the same and the record is empty
            e.surface_points(origin, dims, 2, 0.4)
            e.surface_points_device(origin, dims, 0, 0, d_cnt)
            after = _snapshot(e)
            _same(snaps[0][:7], after[:7])
            assert after[7].tolist() == [0, 0]
    assert snaps[0][7][0] > 0
    _same(snaps[0], snaps[1])


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
        small.surface_points([0, 0, 0], [8, 8, 8])
    assert ei.value.status == 3
    d_cnt = devmem.DeviceArray(np.zeros(1, dtype=np.int64))
    with pytest.raises(ratsdf.RatsdfError) as ei:
        small.surface_points_device([0, 0, 0], [8, 8, 8], 0, 0, d_cnt)
    assert ei.value.status == 3


def test_bad_arguments(make_engine):
    import ratsdf
    from ratsdf import devmem
    from ratsdf._abi import SurfaceParams
    e = make_engine(VS, TRUNC, **SMALL)
    d_buf = devmem.DeviceArray(np.zeros((8, 8), dtype=np.int32))
    d_cnt = devmem.DeviceArray(np.zeros(2, dtype=np.int64))
    ok_o, ok_d = [0, 0, 0], [4, 4, 4]
    bad = [([0, 0, 0], [0, 4, 4], 1, 0.0),
           ([0, 0, 0], [4, -1, 4], 1, 0.0),
           ([0, 0, 0], [4, 4, 1025], 1, 0.0),
           ([0, 0, 0], [1024, 1024, 129], 1, 0.0),              # 2^27 + 2^20 voxels
           ([-32769, 0, 0], [4, 4, 4], 1, 0.0),
           ([0, 32765, 0], [4, 4, 4], 1, 0.0),                  # the last voxel beyond the int16 range
           ([0, 0, 40000], [4, 4, 4], 1, 0.0),
           (ok_o, ok_d, 0, 0.0),
           (ok_o, ok_d, -3, 0.0),
           (ok_o, ok_d, 256, 0.0),
           (ok_o, ok_d, 1, float("nan"))]
    for origin, dims, mw, mp in bad:
        with pytest.raises(ratsdf.RatsdfError) as ei:
            e.surface_points(origin, dims, mw, mp)
        assert ei.value.status == 1, (origin, dims, mw, mp)
        with pytest.raises(ratsdf.RatsdfError) as ei:
            e.surface_points_device(origin, dims, d_buf, 8, d_cnt, mw, mp)
        assert ei.value.status == 1, (origin, dims, mw, mp)
    fn, fd = e.lib.fn["surface_points"], e.lib.fn["surface_points_device"]
    box = [(C.c_int32 * 3)(*v) for v in (ok_o, ok_d)]
    ok = SurfaceParams(1, 0.0, 0, 0)
    p, n = C.c_void_p(), C.c_size_t()
    for params in (SurfaceParams(1, 0.0, 1, 0), SurfaceParams(1, 0.0, 0, 1), None):   # flags, reserved, NULL params
        ref_ = C.byref(params) if params is not None else None
        assert fn(e._h, *box, ref_, C.byref(p), C.byref(n)) == 1
        assert fd(e._h, *box, ref_, d_buf.data_ptr(), 8, d_cnt.data_ptr()) == 1
    assert fn(e._h, None, box[1], C.byref(ok), C.byref(p), C.byref(n)) == 1            # NULL origin / dims / out / n
    assert fn(e._h, box[0], None, C.byref(ok), C.byref(p), C.byref(n)) == 1
    assert fn(e._h, *box, C.byref(ok), None, C.byref(n)) == 1
    assert fn(e._h, *box, C.byref(ok), C.byref(p), None) == 1
    assert fn(None, *box, C.byref(ok), C.byref(p), C.byref(n)) == 1
    assert fd(e._h, *box, C.byref(ok), d_buf.data_ptr(), -1, d_cnt.data_ptr()) == 1    # negative capacity
    assert fd(e._h, *box, C.byref(ok), None, 1, d_cnt.data_ptr()) == 1                 # NULL d_points, capacity > 0
    assert fd(e._h, *box, C.byref(ok), d_buf.data_ptr() + 8, 4, d_cnt.data_ptr()) == 1  # misaligned d_points
    assert fd(e._h, *box, C.byref(ok), d_buf.data_ptr(), 8, None) == 1                 # NULL / misaligned d_count
    assert fd(e._h, *box, C.byref(ok), d_buf.data_ptr(), 8, d_cnt.data_ptr() + 4) == 1
    # the limits themselves are accepted; an empty result is a NULL buffer
    assert len(e.surface_points([-32768, 32767 - 3, 0], [1, 4, 1024])) == 0
    assert len(e.surface_points([0, 0, 0], [1024, 1024, 1], 255, 1.0)) == 0
    assert len(e.surface_points([32767, 32767, 32767], [1, 1, 1])) == 0
    p.value, n.value = 1, 7
    assert fn(e._h, *box, C.byref(ok), C.byref(p), C.byref(n)) == 0 and p.value is None and n.value == 0
    assert e.surface_points_device(ok_o, ok_d, 0, 0, d_cnt) == 0
