"""Batched point sampling of the HIP engine (include/ratsdf_sample.h) against the numpy restatement of its contract
(tests/sample_ref.py), with the corners read from the CPU oracle's map: byte for byte."""
import numpy as np
import pytest

import sample_ref as ref
from parity import TOL, assert_maps_equal
from ratsdf import synthetic
from ratsdf._abi import SAMPLE_ALLOCATED, SAMPLE_DTYPE, SAMPLE_NEAREST, SAMPLE_OBSERVED

pytestmark = pytest.mark.gpu

VS, TRUNC = 0.01, 0.06


def _integrate(engines, frames):
    for f in frames:
        for e in engines:
            e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])


def _same(a, b):
    """byte-for-byte equality of two arrays (record fields included: NaN bits count)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _default(n):
    d = np.zeros(n, dtype=SAMPLE_DTYPE)
    d["tsdf"] = ref.QNAN
    d["grad"] = ref.QNAN
    return d


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


def _point_sets(cpu, rng):
    vox = cpu.gather_valid()
    xyz = np.stack([vox["x"], vox["y"], vox["z"]], axis=1).astype(np.float32)
    lo, hi = xyz.min(0) - TRUNC, xyz.max(0) + TRUNC
    vs = np.float32(VS)
    sets = {}
    sets["uniform"] = rng.uniform(lo, hi, size=(80000, 3)).astype(np.float32)
    pick = xyz[rng.integers(0, len(xyz), 60000)]
    sets["jitter"] = (pick + rng.uniform(-VS, VS, size=pick.shape)).astype(np.float32)
    gi = np.round(xyz[rng.integers(0, len(xyz), 20000)] / vs)
    sets["integer"] = (gi.astype(np.float32) * vs).astype(np.float32)
    blk = np.floor(gi[:2000] / 8)
    blk[:200] = -np.abs(blk[:200]) - 1           # negative block coordinates too
    offs = np.array([-1, -0.5, 0, 0.25, 7, 7.5, 8], dtype=np.float32)
    g = blk[:, None, :] * 8 + offs[rng.integers(0, len(offs), size=(2000, 10, 3))]
    sets["block_edges"] = (g.reshape(-1, 3).astype(np.float32) * vs).astype(np.float32)
    half = np.floor(xyz[rng.integers(0, len(xyz), 20000)] / vs) + np.float32(0.5)
    sets["halves"] = (half.astype(np.float32) * vs).astype(np.float32)
    return sets


def test_parity_with_the_restatement(maps):
    gpu, cpu = maps
    _, blocks = cpu.dump_directory()
    tg, cg, pg = gpu.dump_voxels(gpu.dump_directory()[1]["idx"])
    tc, cc, pc = cpu.dump_voxels(blocks["idx"])
    assert np.array_equal(tg.view(np.uint32), tc.view(np.uint32))   # the corners the restatement reads are the engine's
    prob_exact = np.array_equal(pg.view(np.uint32), pc.view(np.uint32))
    sets = _point_sets(cpu, np.random.default_rng(11))
    total = 0
    for name, pts in sets.items():
        got = gpu.sample_points(pts)
        want = ref.sample(pts, VS, ref.oracle_lookup(cpu))
        total += len(pts)
        for f in ("tsdf", "grad", "rgbw", "min_weight", "flags", "reserved"):
            assert _same(got[f], want[f]), (name, f)
        if prob_exact:
            assert np.array_equal(got["prob"].view(np.uint32), want["prob"].view(np.uint32)), name
        else:
            assert np.max(np.abs(got["prob"] - want["prob"])) <= TOL, name
        assert (got["flags"] & SAMPLE_ALLOCATED).sum() > 0, name
    assert total >= 200000


def test_linear_field_and_edge_inputs(make_engine):
    e = make_engine(VS, TRUNC)
    a = np.array([0.011, -0.007, 0.013], dtype=np.float32)
    b = np.float32(0.125)
    pos = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], dtype=np.int16)
    loc = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    loc = loc[np.lexsort((loc[:, 0], loc[:, 1], loc[:, 2]))]       # voxel order x + 8y + 64z
    g = pos[:, None, :].astype(np.float32) * 8 + loc[None, :, :]
    tsdf = (g @ a + b).astype(np.float32)
    rgbw = np.zeros((27, 512), dtype=ref.RGBW_DTYPE)
    rgbw["weight"] = 7
    rgbw["r"] = 40
    prob = np.full((27, 512), 0.75, dtype=np.float32)
    e.import_blocks(pos, tsdf, rgbw, prob)
    rng = np.random.default_rng(3)
    gp = rng.uniform(-8, 14.999, size=(20000, 3)).astype(np.float32)
    pts = (gp * np.float32(VS)).astype(np.float32)
    s = e.sample_points(pts)
    assert np.all(s["flags"] == SAMPLE_ALLOCATED | SAMPLE_OBSERVED | SAMPLE_NEAREST)
    gg = (pts / np.float32(VS)).astype(np.float64)
    assert np.max(np.abs(s["tsdf"] - (gg @ a.astype(np.float64) + float(b)))) <= 1e-5
    assert np.allclose(s["grad"], (a / np.float32(VS))[None, :], rtol=1e-4, atol=0)
    assert np.all(s["min_weight"] == 7) and np.all(s["prob"] == np.float32(0.75)) and np.all(s["rgbw"]["r"] == 40)
    # edge inputs: non-finite, beyond the int16 range, and a point that a plain int16 cast would put into block 0
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [40000, 1, 1], [-40000, 1, 1],
                    [32767.5, 1, 1], [-32768.5, 1, 1], [65536 + 3.25, 1.5, 1.5]], dtype=np.float32) * np.float32(VS)
    bad = bad.astype(np.float32)
    assert e.sample_points((np.array([[3.25, 1.5, 1.5]], dtype=np.float32) * np.float32(VS)).astype(np.float32))[
        "flags"][0] & SAMPLE_ALLOCATED     # the block a wrap-around would alias is there
    got = e.sample_points(bad)
    assert np.array_equal(got.view(np.uint8), _default(len(bad)).view(np.uint8))
    # n = 0 on both entry points
    assert len(e.sample_points(np.zeros((0, 3), dtype=np.float32))) == 0
    e.sample_points_device(0, 0, 0)


def test_empty_map_and_a_large_batch(make_engine, maps):
    e = make_engine(VS, TRUNC)
    rng = np.random.default_rng(4)
    pts = rng.uniform(-2, 2, size=(1000, 3)).astype(np.float32)
    assert np.array_equal(e.sample_points(pts).view(np.uint8), _default(len(pts)).view(np.uint8))
    gpu, cpu = maps
    vox = cpu.gather_valid()
    xyz = np.stack([vox["x"], vox["y"], vox["z"]], axis=1)
    n = 4 * 1024 * 1024 + 13
    big = rng.uniform(xyz.min(0) - TRUNC, xyz.max(0) + TRUNC, size=(n, 3)).astype(np.float32)
    got = gpu.sample_points(big)
    assert len(got) == n
    spot = np.concatenate([rng.integers(0, n, 20000), np.arange(n - 300, n)])
    want = ref.sample(big[spot], VS, ref.oracle_lookup(cpu))
    for f in ("tsdf", "grad", "rgbw", "min_weight", "flags"):
        assert _same(got[spot][f], want[f]), f
    assert np.max(np.abs(got[spot]["prob"] - want["prob"])) <= TOL


def test_device_path_after_a_carving_batch(make_engine, make_oracle, churn):
    import ratsdf
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
    rng = np.random.default_rng(6)
    vox = host.gather_valid()
    xyz = np.stack([vox["x"], vox["y"], vox["z"]], axis=1)
    pts = (xyz[rng.integers(0, len(xyz), 50000)] + rng.uniform(-VS, VS, size=(50000, 3))).astype(np.float32)
    d_pts = devmem.DeviceArray(pts)
    d_out = devmem.DeviceArray(np.zeros(len(pts) * 32, dtype=np.uint8))
    batch = dev.make_batch([bufs[0].data_ptr()], [bufs[1].data_ptr()], [bufs[2].data_ptr()], [bufs[3].data_ptr()],
                           f["height"], f["width"], 4.0, [f["intrinsics"]], [f["pose"]])
    dev.integrate_device_batch(batch)
    dev.sample_points_device(d_pts.data_ptr(), len(pts), d_out.data_ptr())   # no synchronisation in between
    dev.synchronize()
    got = d_out.numpy().view(SAMPLE_DTYPE)
    want = host.sample_points(pts)
    assert host.last_frame_stats()["deleted_blocks"] > 0
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    # argument checks of the device entry point
    with pytest.raises(ratsdf.RatsdfError) as ei:
        dev.sample_points_device(d_pts.data_ptr(), 10, d_out.data_ptr() + 8)
    assert ei.value.status == 1
    with pytest.raises(ratsdf.RatsdfError) as ei:
        dev.sample_points_device(0, 10, d_out.data_ptr())
    assert ei.value.status == 1
    with pytest.raises(ratsdf.RatsdfError) as ei:
        dev.sample_points_device(d_pts.data_ptr(), 1 << 31, d_out.data_ptr())
    assert ei.value.status == 1


def test_sampling_is_read_only(make_engine, make_oracle, churn):
    gpu, cpu = make_engine(VS, TRUNC), make_oracle(VS, TRUNC, threads=8)
    _integrate([gpu, cpu], churn[:6])
    before = _snapshot(gpu)
    rng = np.random.default_rng(8)
    gpu.sample_points(rng.uniform(-1.7, 1.7, size=(300000, 3)).astype(np.float32))
    _same_snapshot(before, _snapshot(gpu))
    _integrate([gpu, cpu], churn[6:10])
    assert_maps_equal(gpu, cpu)


def test_sphere_surface_and_gradient(make_engine):
    e = make_engine(VS, TRUNC)
    _integrate([e], synthetic.stream("sphere", 8, scale=0.25))
    rng = np.random.default_rng(9)
    d = rng.normal(size=(200000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = (1.5 * d).astype(np.float32)
    s = e.sample_points(pts)
    obs = (s["flags"] & SAMPLE_OBSERVED) != 0
    assert obs.sum() > 1000
    # (the map holds projective distances -- along the viewing ray -- so rays that graze the sphere at the edge of a
    # view leave a few samples off; the bulk must sit on the surface and point inward)
    near = np.abs(s["tsdf"][obs] * np.float32(TRUNC)) <= np.float32(VS)
    assert near.mean() >= 0.95, near.mean()
    gr = s["grad"][obs].astype(np.float64)
    gr /= np.linalg.norm(gr, axis=1, keepdims=True)
    cosang = np.sum(gr * -d[obs], axis=1)
    assert (cosang >= np.cos(np.radians(10))).mean() >= 0.95, (cosang >= np.cos(np.radians(10))).mean()


def test_sticky_error_is_returned(make_engine):
    import ratsdf
    from ratsdf import devmem
    small = make_engine(VS, TRUNC, block_bits=6)   # 64 blocks: the first frame exhausts the pool
    f = synthetic.frame("room", 0, scale=0.25)
    with pytest.raises(ratsdf.RatsdfError) as ei:
        _integrate([small], [f])
        small.synchronize()
    assert ei.value.status == 3
    pts = np.zeros((16, 3), dtype=np.float32)
    with pytest.raises(ratsdf.RatsdfError) as ei:
        small.sample_points(pts)
    assert ei.value.status == 3
    d_pts = devmem.DeviceArray(pts)
    d_out = devmem.DeviceArray(np.zeros(16 * 32, dtype=np.uint8))
    with pytest.raises(ratsdf.RatsdfError) as ei:
        small.sample_points_device(d_pts.data_ptr(), 16, d_out.data_ptr())
    assert ei.value.status == 3
