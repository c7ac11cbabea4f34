"""The Euclidean signed distance field of the HIP engine (include/ratsdf_esdf.h) against the scipy restatement of its
contract (tests/esdf_ref.py), byte for byte (NaN / inf bits count), with the box's states read from the CPU oracle's map
where one exists."""
import ctypes as C

import numpy as np
import pytest

import esdf_ref as ref
from parity import assert_maps_equal
from ratsdf import synthetic
from ratsdf._abi import RGBW_DTYPE

pytestmark = pytest.mark.gpu

VS, TRUNC = 0.01, 0.06


def _integrate(engines, frames):
    for f in frames:
        for e in engines:
            e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])


def _snapshot(e):
    ei, blocks = e.dump_directory()
    nf, heap = e.dump_heap()
    t, c, p = e.dump_voxels(blocks["idx"])
    return ei, blocks, nf, heap[:nf].copy(), t, c, p


def _same_snapshot(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y


def _check(gpu, src, origin, dims, occupied_below=0.0, unknown_occupied=False):
    """the engine's field and states against the restatement fed by `src`'s map; returns the field"""
    got, st = gpu.esdf(origin, dims, occupied_below, unknown_occupied, with_state=True)
    want_st = ref.box_state(src, origin, dims, occupied_below)
    assert ref.same_bytes(st, want_st), (origin, dims, occupied_below)
    want = ref.esdf(want_st, VS, unknown_occupied)
    assert ref.same_bytes(got, want), (origin, dims, occupied_below, unknown_occupied)
    assert ref.same_bytes(gpu.esdf(origin, dims, occupied_below, unknown_occupied), got)   # without the states
    return got


def _solid_blocks(lo, hi):
    """positions of every block in [lo, hi] (block coordinates, inclusive) and their local voxel coordinates"""
    r = [np.arange(a, b + 1) for a, b in zip(lo, hi)]
    pos = np.stack(np.meshgrid(*r, indexing="ij"), -1).reshape(-1, 3).astype(np.int16)
    loc = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    loc = loc[np.lexsort((loc[:, 0], loc[:, 1], loc[:, 2]))]       # voxel order x + 8y + 64z
    return pos, pos[:, None, :].astype(np.int64) * 8 + loc[None, :, :]


def _import(e, pos, tsdf, weight=3):
    rgbw = np.zeros(tsdf.shape, dtype=RGBW_DTYPE)
    rgbw["weight"] = weight
    e.import_blocks(pos, tsdf.astype(np.float32), rgbw, np.full(tsdf.shape, 0.5, dtype=np.float32))


@pytest.fixture(scope="module")
def churn():
    return synthetic.stream("sphere", 12, scale=0.25, noise=True, holes=True)


@pytest.fixture(scope="module")
def maps(churn):
    import ratsdf
    from oracle_binding import load_oracle
    from ratsdf._abi import Engine
    gpu = ratsdf.TSDFGrid(VS, TRUNC)
    cpu = Engine(load_oracle(), VS, TRUNC, threads=8)
    _integrate([gpu, cpu], churn)
    assert_maps_equal(gpu, cpu)
    yield gpu, cpu
    gpu.close()
    cpu.close()


def test_single_occupied_voxel(make_engine):
    e = make_engine(VS, TRUNC)
    pos, g = _solid_blocks((-3, -2, -1), (1, 2, 0))
    tsdf = np.ones(g.shape[:2], dtype=np.float32)
    c = np.array([-5, 3, -2])
    tsdf[np.all(g == c, axis=-1)] = -0.25
    _import(e, pos, tsdf)
    for origin, dims in (([-24, -16, -8], [40, 40, 16]), ([-13, -5, -7], [21, 19, 13]), ([-5, 3, -2], [1, 1, 1]),
                         ([-30, -20, -12], [64, 52, 20])):
        got = _check(e, e, origin, dims)
        z, y, x = np.meshgrid(*[np.arange(o, o + d) for o, d in zip(origin[::-1], dims[::-1])], indexing="ij")
        d2 = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
        want = np.sqrt(d2.astype(np.float32)) * np.float32(VS)
        inside = d2 == 0
        if inside.any():
            # the obstacle itself: one voxel away from the nearest free one (unless the box is only that voxel)
            want[inside] = -np.inf if got.size == 1 else -(np.sqrt(np.float32(1)) * np.float32(VS))
        assert ref.same_bytes(got, want), (origin, dims)


def test_plane(make_engine):
    e = make_engine(VS, TRUNC)
    pos, g = _solid_blocks((-2, -2, -2), (2, 2, 2))
    tsdf = np.clip((g[..., 2] - 3).astype(np.float32) / np.float32(6), -1, 1)   # occupied at and below z = 3
    _import(e, pos, tsdf)
    for ob in (-0.5, 0.0, 0.5):
        for unk in (False, True):
            got = _check(e, e, [-20, -19, -18], [37, 35, 41], ob, unk)
            assert np.isfinite(got).all()
    got = e.esdf([-16, -16, -16], [32, 32, 32])
    z = np.arange(-16, 16)[:, None, None]
    d = np.where(z <= 3, 4 - z, z - 3).astype(np.float32) * np.float32(VS)   # sqrtf(k^2) is k
    assert ref.same_bytes(got, np.broadcast_to(np.where(z <= 3, -d, d), got.shape).astype(np.float32))


def test_sphere_map_against_the_oracle(maps):
    gpu, cpu = maps
    boxes = [([-72, -56, 112], [152, 112, 48]),        # block-aligned, the whole map
             ([-69, -53, 117], [101, 77, 35]),         # negative unaligned origin, dims not multiples of 8
             ([-5, -3, 100], [8, 16, 64]),
             ([40, 30, 150], [90, 60, 40]),            # sticks out of the map
             ([-1000, 900, -700], [24, 9, 17]),        # no allocated block
             ([-3, -60, 113], [1, 120, 1]),            # a 1 x n x 1 line
             ([-77, 0, 131], [160, 1, 1])]
    for origin, dims in boxes:
        for ob in (-0.5, 0.0, 0.5):
            for unk in (False, True):
                _check(gpu, cpu, origin, dims, ob, unk)
    empty = gpu.esdf([-1000, 900, -700], [24, 9, 17])
    assert np.all(empty == np.inf)
    assert np.all(gpu.esdf([-1000, 900, -700], [24, 9, 17], unknown_occupied=True) == -np.inf)


def test_room_map_against_the_oracle(make_engine, make_oracle):
    gpu, cpu = make_engine(VS, TRUNC), make_oracle(VS, TRUNC, threads=8)
    _integrate([gpu, cpu], synthetic.stream("room", 8, scale=0.25, noise=True, holes=True))
    assert_maps_equal(gpu, cpu)
    for origin, dims in (([-56, -56, 144], [128, 80, 16]), ([-60, -61, 130], [133, 90, 37])):
        for ob in (0.0, 0.5):
            for unk in (False, True):
                _check(gpu, cpu, origin, dims, ob, unk)


def test_large_box(maps):
    gpu, cpu = maps
    origin, dims = [-259, -193, -60], [512, 384, 256]
    got = gpu.esdf(origin, dims, 0.0, True)
    want = ref.esdf(ref.box_state(cpu, origin, dims, 0.0), VS, True)
    assert ref.same_bytes(got, want)
    assert np.isfinite(got).all() and -got.min() > 1.0   # unobserved space far from any free voxel


def test_device_path_into_torch_and_devmem(maps):
    import torch
    from ratsdf import devmem
    gpu, _ = maps
    origin, dims = [-69, -53, 117], [101, 77, 35]
    n = int(np.prod(dims))
    for ob, unk in ((0.0, False), (0.5, True)):
        want, want_st = gpu.esdf(origin, dims, ob, unk, with_state=True)
        t_out = torch.empty(n, dtype=torch.float32, device="cuda")
        t_st = torch.empty(n, dtype=torch.uint8, device="cuda")
        gpu.esdf_device(origin, dims, t_out.data_ptr(), t_st.data_ptr(), ob, unk)
        gpu.synchronize()
        assert ref.same_bytes(t_out.cpu().numpy().reshape(want.shape), want)
        assert ref.same_bytes(t_st.cpu().numpy().reshape(want.shape), want_st)
        d_out = devmem.DeviceArray(np.zeros(n, dtype=np.float32))
        gpu.esdf_device(origin, dims, d_out.data_ptr(), 0, ob, unk)
        gpu.synchronize()
        assert ref.same_bytes(d_out.numpy().reshape(want.shape), want)


def test_device_path_after_a_carving_batch(make_engine, make_oracle, churn):
    from ratsdf import devmem
    oracle = make_oracle(VS, TRUNC, threads=8)
    carve = None
    for i, f in enumerate(churn):
        _integrate([oracle], [f])
        if i >= 2 and oracle.last_frame_stats()["deleted_blocks"] > 0:
            carve = i
            break
    assert carve is not None, "no frame of the stream carves"
    dev, host = make_engine(VS, TRUNC), make_engine(VS, TRUNC)
    _integrate([dev], churn[:carve])
    _integrate([host], churn[:carve + 1])
    f = churn[carve]
    bufs = [devmem.DeviceArray(np.ascontiguousarray(f[k])) for k in ("rgb", "depth", "ht", "lt")]
    origin, dims = [-77, -60, 105], [160, 120, 60]
    n = int(np.prod(dims))
    d_out = devmem.DeviceArray(np.zeros(n, dtype=np.float32))
    d_st = devmem.DeviceArray(np.zeros(n, dtype=np.uint8))
    batch = dev.make_batch([bufs[0].data_ptr()], [bufs[1].data_ptr()], [bufs[2].data_ptr()], [bufs[3].data_ptr()],
                           f["height"], f["width"], 4.0, [f["intrinsics"]], [f["pose"]])
    dev.integrate_device_batch(batch)
    dev.esdf_device(origin, dims, d_out.data_ptr(), d_st.data_ptr())   # no synchronisation in between
    dev.synchronize()
    assert host.last_frame_stats()["deleted_blocks"] > 0
    want, want_st = host.esdf(origin, dims, with_state=True)
    assert ref.same_bytes(d_st.numpy().reshape(want.shape), want_st)
    assert ref.same_bytes(d_out.numpy().reshape(want.shape), want)
    assert ref.same_bytes(want, ref.esdf(ref.box_state(oracle, origin, dims), VS))


def test_esdf_is_read_only(make_engine, make_oracle, churn):
    gpu, cpu = make_engine(VS, TRUNC), make_oracle(VS, TRUNC, threads=8)
    _integrate([gpu, cpu], churn[:6])
    before = _snapshot(gpu)
    gpu.esdf([-80, -64, 100], [170, 130, 70], 0.5, True, with_state=True)
    _same_snapshot(before, _snapshot(gpu))
    _integrate([gpu, cpu], churn[6:10])
    assert_maps_equal(gpu, cpu)


def test_workspace_grows_and_shrinks(maps):
    gpu, cpu = maps
    for origin, dims in (([-8, -8, 120], [16, 16, 16]), ([-72, -56, 100], [160, 120, 72]), ([0, 0, 130], [9, 5, 3]),
                         ([-100, -80, 90], [210, 170, 100]), ([-20, -20, 120], [40, 33, 25])):
        _check(gpu, cpu, origin, dims, 0.0, False)


def test_sticky_error_is_returned(make_engine):
    import ratsdf
    from ratsdf import devmem
    small = make_engine(VS, TRUNC, block_bits=6)   # 64 blocks: the first frame exhausts the pool
    f = synthetic.frame("room", 0, scale=0.25)
    with pytest.raises(ratsdf.RatsdfError) as ei:
        _integrate([small], [f])
        small.synchronize()
    assert ei.value.status == 3
    with pytest.raises(ratsdf.RatsdfError) as ei:
        small.esdf([0, 0, 0], [8, 8, 8])
    assert ei.value.status == 3
    d_out = devmem.DeviceArray(np.zeros(512, dtype=np.float32))
    with pytest.raises(ratsdf.RatsdfError) as ei:
        small.esdf_device([0, 0, 0], [8, 8, 8], d_out.data_ptr())
    assert ei.value.status == 3


def test_bad_arguments(make_engine):
    import ratsdf
    from ratsdf import devmem
    e = make_engine(VS, TRUNC)
    d_out = devmem.DeviceArray(np.zeros(64, dtype=np.float32))
    ok_o, ok_d = [0, 0, 0], [4, 4, 4]
    bad = [([0, 0, 0], [0, 4, 4], 0.0, False),
           ([0, 0, 0], [4, -1, 4], 0.0, False),
           ([0, 0, 0], [4, 4, 1025], 0.0, False),
           ([0, 0, 0], [1024, 1024, 129], 0.0, False),          # 2^27 + 2^20 voxels
           ([-32769, 0, 0], [4, 4, 4], 0.0, False),
           ([0, 32765, 0], [4, 4, 4], 0.0, False),              # the last voxel beyond the int16 range
           ([0, 0, 40000], [4, 4, 4], 0.0, False),
           (ok_o, ok_d, float("nan"), False),
           (ok_o, ok_d, 0.0, 2),                                # an unknown flag bit
           (ok_o, ok_d, 0.0, 3)]
    for origin, dims, ob, flags in bad:
        with pytest.raises(ratsdf.RatsdfError) as ei:
            e.esdf(origin, dims, ob, flags)
        assert ei.value.status == 1, (origin, dims, ob, flags)
        with pytest.raises(ratsdf.RatsdfError) as ei:
            e.esdf_device(origin, dims, d_out.data_ptr(), 0, ob, flags)
        assert ei.value.status == 1, (origin, dims, ob, flags)
    for ptr in (0, d_out.data_ptr() + 4, d_out.data_ptr() + 8):   # NULL and misaligned d_out
        with pytest.raises(ratsdf.RatsdfError) as ei:
            e.esdf_device(ok_o, ok_d, ptr)
        assert ei.value.status == 1
    box = [(C.c_int32 * 3)(*v) for v in (ok_o, ok_d)]                # NULL out through the C entry point
    assert e.lib.fn["esdf"](e._h, *box, C.c_float(0), C.c_uint32(0), None, None) == 1
    assert e.lib.fn["esdf"](e._h, None, box[1], C.c_float(0), C.c_uint32(0), d_out.numpy().ctypes.data, None) == 1
    # the limits themselves are accepted
    e.esdf([-32768, 32767 - 3, 0], [1, 4, 1024])
    e.esdf([0, 0, 0], [1024, 1024, 1], 0.0, True)
    got = e.esdf([32767, 32767, 32767], [1, 1, 1], float("inf"))
    assert got.shape == (1, 1, 1) and got[0, 0, 0] == np.inf
