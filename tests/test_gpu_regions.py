"""The connected regions of the HIP engine (include/ratsdf_regions.h) against the scipy restatement of the contract
(tests/regions_ref.py), labels and table byte for byte, with the box's states and probabilities read from the CPU
oracle's map where one exists.  The crafted maps are the smallest at which each phase can go wrong: the local pass
works on 32 x 8 x 4 tiles of the box, the border merge joins them, the table is ordered by a scan."""
import ctypes as C

import numpy as np
import pytest

import regions_ref as ref
from parity import assert_maps_equal
from ratsdf import synthetic
from ratsdf._abi import REGION_DTYPE, RGBW_DTYPE, RegionsParams

pytestmark = pytest.mark.gpu

VS, TRUNC = 0.01, 0.06
U, FR, OC = ref.UNKNOWN, ref.FREE, ref.OCCUPIED
ONLY_FREE, ALL = 1 << FR, 7


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


def _want(src, origin, dims, states, occupied_below=0.0, min_prob=0.0, cache=None):
    """the restatement fed by `src`'s map; cache: a dict that keeps what was read from a map that does not change"""
    key = (tuple(origin), tuple(dims), occupied_below)
    if cache is None or key not in cache:
        read = ref.box_state(src, origin, dims, occupied_below), ref.box_prob(src, origin, dims)
        if cache is None:
            return ref.regions(*read, origin, states, min_prob)
        cache[key] = read
    return ref.regions(*cache[key], origin, states, min_prob)


def _check(gpu, src, origin, dims, states=ONLY_FREE, occupied_below=0.0, min_prob=0.0, cache=None):
    """the engine's labels and table against the restatement fed by `src`'s map; returns them"""
    what = (origin, dims, states, occupied_below, min_prob)
    labels, table = gpu.regions(origin, dims, states, occupied_below, min_prob)
    want_labels, want_table = _want(src, origin, dims, states, occupied_below, min_prob, cache)
    assert table.dtype == REGION_DTYPE == ref.REGION_DTYPE
    assert ref.same_bytes(labels, want_labels), what
    assert ref.same_bytes(table, want_table), what
    assert ref.same_bytes(gpu.regions(origin, dims, states, occupied_below, min_prob, with_labels=False), table), what
    return labels, table


def _craft(e, origin, state, prob=None, outside=FR, absent=None):
    """imports the blocks the box meets so that the box's voxels have `state` (Z, Y, X) and `prob`; voxels of those
    blocks outside the box get `outside`; absent(pos) -> bool array drops blocks"""
    origin = np.asarray(origin, dtype=np.int64)
    dims = np.array(state.shape[::-1], dtype=np.int64)
    r = [np.arange(a, b + 1) for a, b in zip(origin // 8, (origin + dims - 1) // 8)]
    pos = np.stack(np.meshgrid(*r, indexing="ij"), -1).reshape(-1, 3).astype(np.int16)
    if absent is not None:
        pos = pos[~absent(pos)]
    loc = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    loc = loc[np.lexsort((loc[:, 0], loc[:, 1], loc[:, 2]))]       # voxel order x + 8y + 64z
    rel = pos[:, None, :].astype(np.int64) * 8 + loc[None, :, :] - origin
    inside = np.all((rel >= 0) & (rel < dims), axis=-1)
    st = np.full(rel.shape[:2], outside, dtype=np.uint8)
    st[inside] = state[rel[inside][:, 2], rel[inside][:, 1], rel[inside][:, 0]]
    p = np.full(rel.shape[:2], 0.5, dtype=np.float32)
    if prob is not None:
        p[inside] = prob[rel[inside][:, 2], rel[inside][:, 1], rel[inside][:, 0]]
    rgbw = np.zeros(st.shape, dtype=RGBW_DTYPE)
    rgbw["weight"] = np.where(st == U, 0, 3)
    e.import_blocks(pos, np.where(st == OC, -0.25, 0.5).astype(np.float32), rgbw, p)


def _mask_case(e, origin, member, outside=FR):
    """a member mask as FREE voxels among OCCUPIED ones; the labels also against the mask itself"""
    state = np.where(member, FR, OC).astype(np.uint8)
    _craft(e, origin, state, outside=outside)
    labels, table = _check(e, e, list(origin), list(member.shape[::-1]))
    assert ref.same_bytes(labels, ref.regions_of(member, state, origin)[0])
    return labels, table


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


# 1
def test_box_edge_cases(make_engine):
    e = make_engine(VS, TRUNC)
    state = np.full((13, 19, 21), FR, dtype=np.uint8)
    state[3:9, 2:11, 5:17] = OC
    state[0:2, :, :] = U
    _craft(e, [-13, -5, -7], state, absent=lambda pos: pos[:, 0] == 0)
    labels, table = _check(e, e, [-11, -4, -4], [1, 1, 1], ONLY_FREE)             # a member ...
    assert labels.reshape(-1).tolist() == [0] and len(table) == 1
    assert table[0]["voxels"] == 1 and table[0]["faces"] == 0x3F and table[0]["frontier"] == 0
    assert list(table[0]["lo"]) == list(table[0]["hi"]) == [-11, -4, -4]
    labels, table = _check(e, e, [-11, -4, -4], [1, 1, 1], 1 << OC)               # ... and not
    assert labels.reshape(-1).tolist() == [-1] and len(table) == 0
    labels, table = _check(e, e, [-13, -5, -7], [21, 19, 13], ALL)                # every state admitted
    assert len(table) == 1 and np.all(labels == 0)
    assert table[0]["root"] == 0 and table[0]["voxels"] == 21 * 19 * 13 and table[0]["faces"] == 0x3F
    assert list(table[0]["lo"]) == [-13, -5, -7] and list(table[0]["hi"]) == [7, 13, 5]


# 2
def test_checkerboard(make_engine):
    e = make_engine(VS, TRUNC)
    labels, table = _mask_case(e, [0, 0, 0], ref.checkerboard((16, 16, 16)))
    assert len(table) == 2048 and np.all(table["voxels"] == 1) and np.all(np.diff(table["root"]) > 0)
    labels, table = _mask_case(e, [-37, 11, 40], ~ref.checkerboard((5, 11, 35)))   # unaligned, the other colour
    assert len(table) == (5 * 11 * 35) // 2


# 3
def test_serpentine(make_engine):
    e = make_engine(VS, TRUNC)
    for origin, mirrored in (([0, 0, 0], False), ([-45, 200, -3], True)):
        member = ref.serpentine((9, 24, 40), mirrored)
        labels, table = _mask_case(e, origin, member, outside=OC)
        assert len(table) == 1 and table[0]["voxels"] == member.sum()
        assert table[0]["root"] == np.flatnonzero(member.reshape(-1))[0]


# 4
def test_comb(make_engine):
    e = make_engine(VS, TRUNC)
    for origin, member in (([0, 0, 0], ref.comb((3, 7, 30), 1, 3)),                  # both teeth in one tile
                           ([0, 100, 0], ref.comb((6, 21, 70), 2, 17, z=5)),         # in different tiles
                           ([-70, -100, -9], ref.comb((9, 21, 100), 17, 2, z=4))):
        labels, table = _mask_case(e, origin, member, outside=OC)
        assert len(table) == 1 and table[0]["voxels"] == member.sum()


# 5
def test_diagonal_and_box_face_contact(make_engine):
    e = make_engine(VS, TRUNC)
    diag = np.zeros((8, 16, 66), dtype=bool)
    for k in range(8):
        diag[k, k, k] = True                                   # corners, inside a tile and across z tile faces
        diag[k, 15 - k, 28 + k] = True                         # corners across the x = 31 | 32 tile face
        diag[0, 4 + k, 40 + k] = True                          # edges across the y = 7 | 8 tile face
        diag[k, 2, 50 + k] = True                              # edges across z tile faces
    labels, table = _mask_case(e, [-3, 5, 9], diag, outside=OC)
    assert len(table) == diag.sum() and np.all(table["voxels"] == 1)
    # a C whose back lies outside the box: the arms are joined in the map, not in the box
    world = np.zeros((3, 9, 20), dtype=bool)
    world[1, 2, :] = world[1, 6, :] = True
    world[1, 2:7, 0] = True
    state = np.where(world, FR, OC).astype(np.uint8)
    _craft(e, [100, 100, 100], state, outside=OC)
    _, whole = _check(e, e, [100, 100, 100], [20, 9, 3])
    assert len(whole) == 1
    _, cut = _check(e, e, [101, 100, 100], [19, 9, 3])
    assert len(cut) == 2 and cut["voxels"].tolist() == [19, 19] and cut["faces"].tolist() == [3, 3]


# 6
def test_unaligned_origin_absent_blocks_and_every_mask(make_engine):
    e = make_engine(VS, TRUNC)
    rng = np.random.default_rng(5)
    state = rng.integers(0, 3, size=(23, 29, 37)).astype(np.uint8)
    state[:, 10:20, :] = np.where(rng.random((23, 10, 37)) < 0.8, U, state[:, 10:20, :])
    prob = rng.random(state.shape).astype(np.float32)
    origin = [-45, -11, -3]
    _craft(e, origin, state, prob, outside=U, absent=lambda pos: (pos[:, 0] + pos[:, 1] + pos[:, 2]) % 3 == 0)
    got = ref.box_state(e, origin, [37, 29, 23])
    assert (got == U).sum() > (state == U).sum() and (got[got != U] == state[got != U]).all()
    labels, table = _check(e, e, origin, [37, 29, 23], 1 << U)
    assert table["voxels"].max() > 512                          # absent blocks and weight-0 voxels in one region
    _check(e, e, origin, [37, 29, 23], (1 << FR) | (1 << U))
    for states in range(1, 8):
        _check(e, e, [-41, -9, -1], [30, 21, 17], states, min_prob=0.25)


# 7
def test_min_prob(make_engine):
    e = make_engine(VS, TRUNC)
    thr = np.float32(0.7)
    below, tiny = np.nextafter(thr, np.float32(0)), np.float32(1e-45)
    state = np.array([FR, FR, FR, OC, OC, U, FR, U], dtype=np.uint8).reshape(1, 1, 8)
    prob = np.array([thr, below, np.nan, thr, below, np.nan, 1.0, 0.9], dtype=np.float32).reshape(1, 1, 8)
    _craft(e, [3, 5, 7], state, prob, outside=OC)
    assert ref.same_bytes(ref.box_prob(e, [3, 5, 7], [8, 1, 1]), prob)
    labels, _ = _check(e, e, [3, 5, 7], [8, 1, 1], ALL, min_prob=float(thr))
    assert labels.reshape(-1).tolist() == [0, -1, 2, 2, -1, -1, 6, -1]     # at the threshold: kept; NaN: kept
    labels, _ = _check(e, e, [3, 5, 7], [8, 1, 1], ALL, min_prob=0.0)
    assert labels.reshape(-1).tolist() == [0] * 8                          # an UNKNOWN voxel is kept at 0 ...
    labels, _ = _check(e, e, [3, 5, 7], [8, 1, 1], ALL, min_prob=float(tiny))
    assert labels.reshape(-1).tolist() == [0] * 5 + [-1, 6, -1]            # ... and dropped just above it
    _check(e, e, [3, 5, 7], [8, 1, 1], ALL, min_prob=float("inf"))
    _check(e, e, [3, 5, 7], [8, 1, 1], ALL, min_prob=float("-inf"))


# 8
def test_frontier(make_engine):
    e = make_engine(VS, TRUNC)
    state = np.full((5, 5, 5), OC, dtype=np.uint8)
    state[2, 2, 2] = FR
    state[2, 2, 3] = state[2, 3, 2] = state[3, 2, 2] = U       # three unknown neighbours
    state[0, 0, 0] = FR
    state[0, 0, 1] = U
    _craft(e, [8, 8, 8], state, outside=U)
    _, table = _check(e, e, [8, 8, 8], [5, 5, 5])
    assert table["frontier"].tolist() == [1, 1] and table["voxels"].tolist() == [1, 1]
    _, table = _check(e, e, [10, 10, 10], [1, 1, 1])           # its unknown neighbours are outside the box
    assert table["frontier"].tolist() == [0]
    _, table = _check(e, e, [7, 7, 7], [2, 2, 2])              # (8, 8, 8) with the block's unknown outside around it
    assert table["frontier"].tolist() == [1]
    _, table = _check(e, e, [8, 8, 8], [5, 5, 5], ALL)
    assert len(table) == 1 and table["frontier"][0] == ref.unknown_neighbour(state).sum()


# 9
@pytest.mark.parametrize("density", [0.2, 0.31, 0.5, 0.8])
def test_random_masks(make_engine, density):
    e = make_engine(VS, TRUNC)
    member = ref.random_mask((23, 29, 37), density, seed=int(density * 100))
    _mask_case(e, [-19, 3, -12], member)


# 10
BOXES = [([-72, -56, 112], [152, 112, 48]),        # block-aligned, the whole map
         ([-69, -53, 117], [101, 77, 35]),         # negative unaligned origin, dims not multiples of 8
         ([-5, -3, 100], [8, 16, 64]),
         ([40, 30, 150], [90, 60, 40]),            # sticks out of the map
         ([-1000, 900, -700], [24, 9, 17]),        # no allocated block
         ([-3, -60, 113], [1, 120, 1]),            # a 1 x n x 1 line
         ([-77, 0, 131], [160, 1, 1])]


def test_sphere_map_against_the_oracle(maps):
    gpu, cpu = maps
    combos = ((ONLY_FREE, 0.0, 0.0), (1 << OC, 0.0, 0.5), (ALL, 0.0, 0.0), (1 << U, 0.0, 0.0), (1 << OC, 0.5, 0.0),
              ((1 << FR) | (1 << U), -0.5, 0.0))
    cache = {}
    for k, (origin, dims) in enumerate(BOXES):
        for states, ob, mp in combos[:3] if k < 2 else combos:     # (the two large boxes: one threshold)
            _check(gpu, cpu, origin, dims, states, ob, mp, cache)
    labels, table = gpu.regions([-1000, 900, -700], [24, 9, 17])
    assert len(table) == 0 and np.all(labels == -1)
    _, table = gpu.regions([-1000, 900, -700], [24, 9, 17], 1 << U)
    assert len(table) == 1 and table[0]["voxels"] == table[0]["frontier"] == 24 * 9 * 17


def test_workspace_grows_then_a_small_box_again(maps):
    gpu, cpu = maps
    _check(gpu, cpu, [-8, -8, 120], [16, 16, 16])
    _check(gpu, cpu, [-131, -97, 70], [256, 192, 128], ONLY_FREE)
    _check(gpu, cpu, [0, 0, 130], [9, 5, 3], ALL)
    _check(gpu, cpu, [-20, -20, 120], [40, 33, 25])


# 11
def test_device_path_into_torch_and_devmem(maps):
    import torch
    from ratsdf import devmem
    gpu, _ = maps
    origin, dims = [-72, -56, 112], [152, 112, 48]
    n = int(np.prod(dims))
    for states, mp in ((1 << OC, 0.0), (1 << OC, 0.5), (ALL, 0.0)):
        want_labels, want = gpu.regions(origin, dims, states, 0.0, mp)
        total = len(want)
        assert total > 8 or (states == ALL and total == 1)         # (one region: the cut below is a capacity of 0)
        t_lab = torch.empty(n, dtype=torch.int32, device="cuda")
        t_reg = torch.full((total + 3, 32), 0xAB, dtype=torch.uint8, device="cuda")
        t_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        assert gpu.regions_device(origin, dims, t_lab, t_reg, total + 3, t_cnt, states, 0.0, mp) == total
        assert ref.same_bytes(t_lab.cpu().numpy().reshape(want_labels.shape), want_labels)
        got = t_reg.cpu().numpy()
        assert ref.same_bytes(got[:total].reshape(-1).view(REGION_DTYPE), want) and np.all(got[total:] == 0xAB)
        # a capacity below the total: the prefix, the rest untouched, the true total; no labels asked for
        d_reg = devmem.DeviceArray(np.full((total, 32), 0xCD, dtype=np.uint8))
        d_cnt = devmem.DeviceArray(np.zeros(1, dtype=np.int64))
        cut = total // 2
        assert gpu.regions_device(origin, dims, 0, d_reg, cut, d_cnt, states, 0.0, mp) == total
        got = d_reg.numpy()
        assert ref.same_bytes(got[:cut].reshape(-1).view(REGION_DTYPE), want[:cut]) and np.all(got[cut:] == 0xCD)
        # the pure count
        d_cnt = devmem.DeviceArray(np.full(1, -1, dtype=np.int64))
        d_lab = devmem.DeviceArray(np.zeros(n, dtype=np.int32))
        assert gpu.regions_device(origin, dims, d_lab, 0, 0, d_cnt, states, 0.0, mp) == total
        assert ref.same_bytes(d_lab.numpy().reshape(want_labels.shape), want_labels)


def test_esdf_and_regions_back_to_back(maps):
    from ratsdf import devmem
    gpu, _ = maps
    origin, dims = [-69, -53, 117], [101, 77, 35]
    n = int(np.prod(dims))
    want_field, want_state = gpu.esdf(origin, dims, with_state=True)
    want_labels, want = gpu.regions(origin, dims, ALL)
    d_out = devmem.DeviceArray(np.zeros(n, dtype=np.float32))
    d_st = devmem.DeviceArray(np.zeros(n, dtype=np.uint8))
    d_lab = devmem.DeviceArray(np.zeros(n, dtype=np.int32))
    d_reg = devmem.DeviceArray(np.zeros((len(want) + 1, 32), dtype=np.uint8))
    d_cnt = devmem.DeviceArray(np.zeros(2, dtype=np.int64))
    params = RegionsParams(0.0, 0.0, ALL, 0)
    box = [(C.c_int32 * 3)(*v) for v in (origin, dims)]
    gpu.esdf_device(origin, dims, d_out.data_ptr(), 0)
    assert gpu.lib.fn["regions_device"](gpu._h, *box, C.byref(params), d_lab.data_ptr(), d_reg.data_ptr(),
                                        len(want) + 1, d_cnt.data_ptr()) == 0
    gpu.esdf_device(origin, dims, d_out.data_ptr(), d_st.data_ptr())          # no synchronisation in between
    assert gpu.lib.fn["regions_device"](gpu._h, *box, C.byref(params), None, None, 0, d_cnt.data_ptr() + 8) == 0
    gpu.synchronize()
    assert ref.same_bytes(d_out.numpy().reshape(want_field.shape), want_field)
    assert ref.same_bytes(d_st.numpy().reshape(want_state.shape), want_state)
    assert ref.same_bytes(d_lab.numpy().reshape(want_labels.shape), want_labels)
    assert ref.same_bytes(d_reg.numpy()[:len(want)].reshape(-1).view(REGION_DTYPE), want)
    assert d_cnt.numpy().tolist() == [len(want), len(want)]


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
    dev = make_engine(VS, TRUNC)
    _integrate([dev], churn[:carve])
    f = churn[carve]
    bufs = [devmem.DeviceArray(np.ascontiguousarray(f[k])) for k in ("rgb", "depth", "ht", "lt")]
    origin, dims = [-77, -60, 105], [160, 120, 60]
    n = int(np.prod(dims))
    want_labels, want = _want(oracle, origin, dims, ONLY_FREE)
    d_lab = devmem.DeviceArray(np.zeros(n, dtype=np.int32))
    d_reg = devmem.DeviceArray(np.zeros((len(want), 32), dtype=np.uint8))
    d_cnt = devmem.DeviceArray(np.zeros(1, dtype=np.int64))
    batch = dev.make_batch([bufs[0].data_ptr()], [bufs[1].data_ptr()], [bufs[2].data_ptr()], [bufs[3].data_ptr()],
                           f["height"], f["width"], 4.0, [f["intrinsics"]], [f["pose"]])
    dev.integrate_device_batch(batch)
    total = dev.regions_device(origin, dims, d_lab, d_reg, len(want), d_cnt)   # no synchronisation in between
    assert dev.last_frame_stats()["deleted_blocks"] > 0
    assert total == len(want) > 0
    assert ref.same_bytes(d_lab.numpy().reshape(want_labels.shape), want_labels)
    assert ref.same_bytes(d_reg.numpy().reshape(-1).view(REGION_DTYPE), want)


# 12
def test_two_calls_give_identical_bytes(maps):
    gpu, _ = maps
    for states in (ONLY_FREE, ALL, 1 << OC):
        a = gpu.regions([-72, -56, 112], [152, 112, 48], states)
        b = gpu.regions([-72, -56, 112], [152, 112, 48], states)
        assert ref.same_bytes(a[0], b[0]) and ref.same_bytes(a[1], b[1])


# 13
def test_regions_are_read_only(make_engine, make_oracle, churn):
    gpu, cpu = make_engine(VS, TRUNC), make_oracle(VS, TRUNC, threads=8)
    _integrate([gpu, cpu], churn[:6])
    before = _snapshot(gpu)
    gpu.regions([-80, -64, 100], [170, 130, 70], ALL, 0.5, 0.25)
    _same_snapshot(before, _snapshot(gpu))
    _integrate([gpu, cpu], churn[6:10])
    assert_maps_equal(gpu, cpu)


# 14
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
        small.regions([0, 0, 0], [8, 8, 8])
    assert ei.value.status == 3
    d_cnt = devmem.DeviceArray(np.zeros(1, dtype=np.int64))
    with pytest.raises(ratsdf.RatsdfError) as ei:
        small.regions_device([0, 0, 0], [8, 8, 8], 0, 0, 0, d_cnt)
    assert ei.value.status == 3


def test_bad_arguments(make_engine):
    from ratsdf import devmem
    e = make_engine(VS, TRUNC)
    d_lab = devmem.DeviceArray(np.zeros(64, dtype=np.int32))
    d_reg = devmem.DeviceArray(np.full((32, 32), 0x5A, dtype=np.uint8))
    d_cnt = devmem.DeviceArray(np.full(2, -7, dtype=np.int64))
    labels = np.full(64, -9, dtype=np.int32)
    host, device = e.lib.fn["regions"], e.lib.fn["regions_device"]
    vec = lambda v: (C.c_int32 * 3)(*v) if v is not None else None   # noqa: E731
    ok_o, ok_d = [0, 0, 0], [4, 4, 4]

    def call_host(origin=ok_o, dims=ok_d, params=(0.0, 0.0, 1, 0), lab=labels.ctypes.data, out=True, n=True):
        p, m = C.c_void_p(), C.c_size_t()
        st = host(e._h, vec(origin), vec(dims), C.byref(RegionsParams(*params)) if params else None, lab,
                  C.byref(p) if out else None, C.byref(m) if n else None)
        assert st != 0 or (e._take(p, m.value, REGION_DTYPE) is not None)
        return st

    def call_device(origin=ok_o, dims=ok_d, params=(0.0, 0.0, 1, 0), lab=d_lab.data_ptr(), reg=d_reg.data_ptr(),
                    capacity=32, cnt=d_cnt.data_ptr()):
        return device(e._h, vec(origin), vec(dims), C.byref(RegionsParams(*params)) if params else None, lab or None,
                      reg or None, capacity, cnt or None)

    assert call_host() == 0 and call_device() == 0
    e.synchronize()
    boxes = [([0, 0, 0], [0, 4, 4]), ([0, 0, 0], [4, -1, 4]), ([0, 0, 0], [4, 4, 1025]),
             ([0, 0, 0], [1024, 1024, 129]),                    # 2^27 + 2^20 voxels
             ([-32769, 0, 0], [4, 4, 4]), ([0, 32765, 0], [4, 4, 4]), ([0, 0, 40000], [4, 4, 4]),
             (None, ok_d), (ok_o, None)]
    d_cnt_before = d_cnt.numpy().copy()
    for origin, dims in boxes:
        assert call_host(origin, dims) == 1, (origin, dims)
        assert call_device(origin, dims) == 1, (origin, dims)
    nan = float("nan")
    for params in (None, (nan, 0.0, 1, 0), (0.0, nan, 1, 0), (0.0, 0.0, 0, 0), (0.0, 0.0, 8, 0), (0.0, 0.0, 1 << 31, 0),
                   (0.0, 0.0, 1, 1), (0.0, 0.0, 1, 2), (0.0, 0.0, 1, 1 << 31)):
        assert call_host(params=params) == 1, params
        assert call_device(params=params) == 1, params
    assert call_host(out=False) == 1 and call_host(n=False) == 1
    assert call_device(capacity=-1) == 1
    assert call_device(reg=0, capacity=1) == 1                  # no table buffer, but a capacity
    assert call_device(cnt=0) == 1
    assert call_device(lab=d_lab.data_ptr() + 4) == 1           # misaligned pointers
    assert call_device(reg=d_reg.data_ptr() + 8) == 1
    assert call_device(cnt=d_cnt.data_ptr() + 4) == 1
    e.synchronize()
    assert np.array_equal(d_cnt.numpy(), d_cnt_before)          # nothing was launched
    # the limits themselves are accepted
    labels_, table = e.regions([-32768, 32767 - 3, 0], [1, 4, 1024], ALL)
    assert len(table) == 1 and table[0]["voxels"] == 4096 and list(table[0]["lo"]) == [-32768, 32764, 0]
    assert list(table[0]["hi"]) == [-32768, 32767, 1023]
    table = e.regions([0, 0, 0], [1024, 1024, 1], 1 << U, with_labels=False)
    assert len(table) == 1 and table[0]["voxels"] == 1 << 20 and table[0]["frontier"] == 1 << 20
    labels_, table = e.regions([32767, 32767, 32767], [1, 1, 1], ALL, float("inf"), float("inf"))
    assert labels_.shape == (1, 1, 1) and len(table) == 0      # UNKNOWN: p = 0 < inf
    assert call_host(lab=None) == 0 and call_device(lab=0) == 0 and call_device(reg=0, capacity=0) == 0
