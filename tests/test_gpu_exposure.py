"""The exposure of surface points to lamps on the HIP engine (ratsdf_exposure*, include/ratsdf_surface.h) against the
restatement of the contract (tests/exposure_ref.py): dose, mask, lamp table and summary byte for byte, with the box's
states read from the map the case crafted (or from the CPU oracle's map where frames built it).  The crafted cases are
the smallest at which each part can go wrong: the walk's ties, the 4 x 4 x 4 bricks of the blocking bitmap and their
padding at the box's faces, the packing of (point, lamp) pairs into waves, the ordered sum.

Not compared: what a sum delivers once it has met a NaN (the header leaves that NaN's payload open); no case here
produces one but by copying a prior dose through."""
import ctypes as C

import numpy as np
import pytest

import exposure_ref as ref
from parity import assert_maps_equal
from ratsdf import devmem, synthetic
from ratsdf._abi import (EXPOSURE_SUMMARY_DTYPE, LAMP_DTYPE, LAMP_RECORD_DTYPE, SURFACE_DTYPE, ExposureParams)
from test_gpu_regions import _craft, _integrate, _same_snapshot, _snapshot

pytestmark = pytest.mark.gpu

VS, TRUNC = 0.01, 0.06
F = np.float32
U, FR, OC = ref.UNKNOWN, ref.FREE, ref.OCCUPIED


def _points(vox, normal, prob=0.5):
    """surface points at the centres of the voxels `vox` (absolute indices; the start voxel is one `normal` on)"""
    vox = np.asarray(vox, dtype=F).reshape(-1, 3)
    p = np.zeros(len(vox), dtype=SURFACE_DTYPE)
    p["pos"] = vox * F(VS)
    p["normal"] = np.broadcast_to(np.asarray(normal, dtype=F), vox.shape)
    p["prob"] = prob
    return p


def _lamps(vox, power=1.0):
    vox = np.asarray(vox, dtype=F).reshape(-1, 3)
    l = np.zeros(len(vox), dtype=LAMP_DTYPE)
    l["pos"] = vox * F(VS)
    l["power"] = power
    return l


def _check(gpu, origin, dims, points, lamps, src=None, state=None, dose=None, occupied_below=0.0, **kw):
    """the engine's four outputs against the restatement fed by `src`'s map (the engine's own by default); returns
    (dose, mask, table, summary)"""
    what = (origin, dims, len(points), len(lamps), kw)
    if state is None:
        state = ref.box_state(src or gpu, origin, dims, occupied_below)
    want = ref.exposure(state, origin, VS, points, lamps, dose=dose, **kw)
    got = gpu.exposure(origin, dims, points, lamps, occupied_below=occupied_below, dose=dose, with_mask=True, **kw)
    assert got[2].dtype == LAMP_RECORD_DTYPE == ref.LAMP_RECORD_DTYPE
    assert got[3].dtype == EXPOSURE_SUMMARY_DTYPE == ref.SUMMARY_DTYPE
    assert ref.same_bytes(got[1], want[1]), (what, np.flatnonzero(got[1] != want[1])[:5])
    assert ref.same_bytes(got[0], want[0]), (what, np.flatnonzero(got[0].view(np.uint32) != want[0].view(np.uint32))[:5])
    assert ref.same_bytes(got[2], want[2]), (what, got[2], want[2])
    assert got[3].tobytes() == want[3].tobytes(), (what, got[3], want[3])
    return got


def _room(e, origin, shape, occupied=()):
    """crafts a box of FREE voxels whose z = 0 layer is an OCCUPIED floor, plus the `occupied` voxels (box-relative
    x, y, z); returns the state"""
    state = np.full(shape, FR, dtype=np.uint8)
    state[0] = OC
    for x, y, z in occupied:
        state[z, y, x] = OC
    _craft(e, origin, state)
    return state


def _at(origin, v):
    return [origin[0] + v[0], origin[1] + v[1], origin[2] + v[2]]


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
def test_open_box(make_engine):
    """a floor slab that runs on beyond the box on every side, so that the box's surface points are the slab's top
    alone; one lamp overhead lights them all"""
    e = make_engine(VS, TRUNC)
    state = np.full((16, 24, 24), FR, dtype=np.uint8)
    state[:6] = OC                                                  # up to z = -3
    _craft(e, [-16, 0, -8], state)
    origin, dims = [-13, 5, -3], [20, 12, 9]
    points = e.surface_points(origin, dims)
    assert len(points) == 20 * 12 and np.all(points["normal"] == np.array([0, 0, 1], dtype=F))
    lamps = _lamps([[-3, 11, 4]], 2.5)
    dose, mask, table, summary = _check(e, origin, dims, points, lamps)
    assert np.all(mask == 1) and np.all(dose > 0) and summary["points_lit"] == summary["lit_pairs"] == 240
    assert table[0].tolist() == (1, 240, 240, 0) and summary["points_outside"] == 0
    under = np.argmin(np.abs(points["pos"][:, 0] + 3 * VS) + np.abs(points["pos"][:, 1] - 11 * VS))
    r = 4 * VS - points["pos"][under, 2]
    assert abs(dose[under] - 2.5 / (4 * np.pi * r * r)) < 1e-3 * dose[under] and dose[under] == dose.max()
    _check(e, origin, dims, points, lamps, min_irradiance=float(np.median(dose)), p_cutoff=0.75)
    _check(e, [-3, 11, -2], [1, 1, 7], points, lamps)               # a one-column box: nearly every point OUTSIDE


# 2
def test_pillar_and_hole(make_engine):
    e = make_engine(VS, TRUNC)
    origin, dims = [0, 0, 0], [24, 16, 12]
    wall = [(16, y, z) for y in range(16) for z in range(1, 12) if (y, z) != (8, 3)]
    _room(e, origin, (16, 16, 24), [(8, 4, z) for z in range(1, 7)] + wall)
    lamps = _lamps([[4, 8, 3]])
    behind_pillar = _points([[12, 0, 0]], [0, 0, 1])                # the walk (12, 0, 1) -> (4, 8, 3) meets (8, 4, 2)
    beside_pillar = _points([[12, 3, 0]], [0, 0, 1])
    through_hole = _points([[21, 8, 3]], [-1, 0, 0])                # straight along x through (16, 8, 3)
    at_the_wall = _points([[21, 9, 3]], [-1, 0, 0])                 # y steps half way: meets the wall at (16, 9, 3)
    points = np.concatenate([behind_pillar, beside_pillar, through_hole, at_the_wall])
    _, mask, table, summary = _check(e, origin, dims, points, lamps)
    assert mask.tolist() == [0, 1, 1, 0] and table[0]["lit"] == 2 and summary["points_lit"] == 2
    floor = e.surface_points(origin, dims)
    assert len(floor) > 300
    _, mask, _, _ = _check(e, origin, dims, floor, lamps)
    assert 0 < np.count_nonzero(mask) < len(floor)                  # the pillar and the wall cast shadows


# 3
def test_staircase_wall(make_engine):
    """a diagonal wall one voxel thick, its voxels touching by edges only: a 6-connected walk cannot slip through"""
    e = make_engine(VS, TRUNC)
    origin, dims = [3, -5, 2], [16, 16, 4]
    state = np.full((4, 16, 16), FR, dtype=np.uint8)
    for k in range(16):
        state[:, k, k] = OC
    _craft(e, origin, state)
    n = np.array([1, -1, 0], dtype=F) / F(np.sqrt(2.0))
    above = [(x, y, z) for x in range(0, 12) for y in range(x + 3, 16) for z in (1, 2)]      # y > x: beyond the wall
    points = _points([_at(origin, v) for v in above], n)
    below = _lamps([_at(origin, v) for v in [(5, 0, 1), (9, 2, 2), (15, 6, 0), (12, 9, 3), (15, 13, 1)]])
    _, mask, table, _ = _check(e, origin, dims, points, below)
    assert np.all(mask == 0) and np.all(table["accepted"] == 1)
    same_side = _lamps([_at(origin, v) for v in [(5, 0, 1), (2, 14, 1)]])
    _, mask, _, _ = _check(e, origin, dims, points, same_side)
    assert np.all((mask & 1) == 0) and np.any(mask & 2)
    assert np.any(ref.exposure(state, origin, VS, points, below, wrong="bresenham")[1] != 0)  # what it guards against


# 4
@pytest.mark.parametrize("step", [(5, 5, 0), (4, 4, 4), (6, 3, 0)])
def test_tie_cases(make_engine, step):
    e = make_engine(VS, TRUNC)
    origin, dims = [-2, 3, -1], [12, 8, 8]
    a = np.array([1, 1, 1])
    b = a + np.array(step)
    cells = ref.walk(a, b)
    other = ref.walk(a, b, ties_highest=True)
    back = ref.walk(b, a)
    assert len(cells) == sum(step) + 1 and cells[0] == tuple(a) and cells[-1] == tuple(b)
    forward = (_points([_at(origin, a - [1, 0, 0])], [1, 0, 0]), _lamps([_at(origin, b)]))
    backward = (_points([_at(origin, b + [1, 0, 0])], [-1, 0, 0]), _lamps([_at(origin, a)]))
    blockers = [None, cells[1], cells[len(cells) // 2], back[1], back[len(back) // 2]]
    blockers += [v for v in other if v not in cells][:2] + [v for v in cells if v not in other][:2]
    for blocker in blockers:
        state = np.full((8, 8, 12), FR, dtype=np.uint8)
        if blocker is not None:
            state[blocker[2], blocker[1], blocker[0]] = OC
        _craft(e, origin, state)
        for (points, lamps), path in ((forward, cells), (backward, back)):
            _, mask, _, _ = _check(e, origin, dims, points, lamps, state=state)
            assert mask[0] == (0 if blocker in path else 1), (step, blocker)


# 5
@pytest.mark.parametrize("n_lamps", [0, 1, 3, 33, 64])
def test_packing_edges(make_engine, n_lamps):
    e = make_engine(VS, TRUNC)
    origin, dims = [0, 0, 0], [16, 8, 8]
    _room(e, origin, (8, 8, 16), [(5, 3, z) for z in range(1, 5)] + [(11, y, 3) for y in range(8)])
    rng = np.random.default_rng(n_lamps)
    at = np.stack([rng.integers(0, 16, n_lamps), rng.integers(0, 8, n_lamps), rng.integers(1, 8, n_lamps)], 1)
    at[:1] = (0, 0, 0)                                               # the first lamp sits in the floor: not accepted
    at[1:2] = (1, 1, 5)
    lamps = _lamps(at, rng.uniform(0.5, 2.0, n_lamps).astype(F))
    state = ref.box_state(e, origin, dims)
    for n_points in (0, 1, 63, 64, 65, 77):                          # 77: no multiple of 1, 2, 4, ... 64 points a wave
        floor = np.stack([rng.integers(0, 16, n_points), rng.integers(0, 8, n_points), np.zeros(n_points, int)], 1)
        points = _points(floor, [0, 0, 1], rng.uniform(0, 1, n_points).astype(F))
        _, mask, table, summary = _check(e, origin, dims, points, lamps, state=state, min_irradiance=20.0)
        if n_lamps >= 1:
            assert table["accepted"][0] == 0 and np.all((mask & 1) == 0)
        if n_lamps >= 3 and n_points >= 63:
            assert summary["lit_pairs"] > n_points // 2 and table["accepted"][1] == 1
            assert table["lit"].sum() <= summary["lit_pairs"]


# 6
def test_longest_walk(make_engine):
    e = make_engine(VS, TRUNC)
    origin, dims = [-512, 0, 0], [1024, 8, 8]
    near = [(0, y, z) for y, z in ((3, 3), (0, 0), (7, 7), (0, 7), (7, 0))]          # the start voxels
    far = [(1023, y, z) for y, z in ((3, 3), (0, 0), (7, 7))]
    ends = [(1023, 3, 3), (0, 4, 4)]
    walks = {(s, L): ref.walk(s, L) for s in near + far for L in ends}
    assert len(walks[(0, 0, 7), (1023, 3, 3)]) == 1023 + 3 + 4 + 1
    blocker = [v for v in walks[(0, 0, 7), (1023, 3, 3)] if v[0] == 300][0]
    state = np.full((8, 8, 1024), FR, dtype=np.uint8)
    state[blocker[2], blocker[1], blocker[0]] = OC
    _craft(e, origin, state)
    points = np.concatenate([_points([_at(origin, (x - 1, y, z)) for x, y, z in near], [1, 0, 0]),
                             _points([_at(origin, (x + 1, y, z)) for x, y, z in far], [-1, 0, 0])])
    lamps = _lamps([_at(origin, L) for L in ends], 1000.0)
    _, mask, _, summary = _check(e, origin, dims, points, lamps, state=state)
    expected = [sum((blocker not in walks[s, L]) << k for k, L in enumerate(ends)) for s in near + far]
    assert mask.tolist() == expected and 0 < expected.count(3) < len(expected) and (expected[3] & 1) == 0
    origin, dims = [5, 5, -100], [1, 1, 300]
    for blocker in (None, 137):
        state = np.full((300, 1, 1), FR, dtype=np.uint8)
        if blocker:
            state[blocker] = OC
        _craft(e, origin, state)
        points = np.concatenate([_points([[5, 5, -101]], [0, 0, 1]), _points([[5, 5, 200]], [0, 0, -1])])
        lamps = _lamps([[5, 5, 199], [5, 5, -100]], 50.0)
        _, mask, _, _ = _check(e, origin, dims, points, lamps, state=state)
        assert mask.tolist() == ([2, 1] if blocker else [3, 3])     # each still sees the lamp in its own voxel


def _random_case(origin, dims, seed, n_points=150, n_lamps=12, density=0.04):
    rng = np.random.default_rng(seed)
    X, Y, Z = dims
    state = np.where(rng.random((Z, Y, X)) < density, OC, FR).astype(np.uint8)
    lo, hi = np.array(origin) - 2, np.array(origin) + np.array(dims) + 2    # some beyond every face
    points = np.zeros(n_points, dtype=SURFACE_DTYPE)
    points["pos"] = (rng.integers(lo, hi, (n_points, 3)) + rng.uniform(-0.5, 0.5, (n_points, 3))).astype(F) * F(VS)
    n = rng.normal(size=(n_points, 3))
    points["normal"] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
    points["prob"] = rng.uniform(0, 1, n_points).astype(F)
    lamps = np.zeros(n_lamps, dtype=LAMP_DTYPE)
    lamps["pos"] = (rng.integers(lo, hi, (n_lamps, 3)) + rng.uniform(-0.5, 0.5, (n_lamps, 3))).astype(F) * F(VS)
    lamps["power"] = rng.uniform(0.1, 3.0, n_lamps).astype(F)
    return state, points, lamps


# 7
@pytest.mark.parametrize("origin, dims", [([-32768, 32755, -7], [13, 13, 10]), ([32761, -32768, 32762], [7, 5, 6]),
                                          ([-3, 2, 1], [9, 1, 1]), ([1, -2, 3], [5, 6, 7])])
def test_box_faces(make_engine, origin, dims):
    """start voxels and lamps beyond every face, lamps in OCCUPIED voxels; dims that are no multiples of 4 and origins
    that are no multiples of 8, at both ends of the grid: the padding of the edge bricks"""
    e = make_engine(VS, TRUNC)
    state, points, lamps = _random_case(origin, dims, seed=sum(dims))
    _craft(e, origin, state, outside=OC)
    occupied = np.argwhere(state == OC)[:2]
    lamps[:len(occupied)]["pos"] = (occupied[:, ::-1] + np.array(origin)).astype(F) * F(VS)
    z, y, x = np.argwhere(state == FR)[0]
    inside = np.array(origin) + [x, y, z]
    lamps[2]["pos"] = inside.astype(F) * F(VS)                        # one in a FREE voxel, one beyond the box
    lamps[3]["pos"] = (np.array(origin) + [dims[0], 0, 0]).astype(F) * F(VS)
    points[0]["pos"], points[0]["normal"] = inside.astype(F) * F(VS), (0, 0, 0)     # start voxel: its own
    points[1]["pos"], points[1]["normal"] = inside.astype(F) * F(VS), (-dims[0], 0, 0)
    _, mask, table, summary = _check(e, origin, dims, points, lamps, state=state)
    assert summary["points_outside"] >= 1 and 1 <= summary["lamps_accepted"] < len(lamps)
    assert np.all(table["accepted"][:len(occupied)] == 0) and table["accepted"][2:4].tolist() == [1, 0]
    if np.prod(dims) > 1000:
        assert summary["lit_pairs"] > 0
    _check(e, origin, dims, points, lamps, max_range=5 * VS, p_cutoff=0.3, min_irradiance=100.0)


# 8
def test_unknown_space(make_engine):
    e = make_engine(VS, TRUNC)
    origin, dims = [0, 8, -8], [24, 8, 8]
    state = np.full((8, 8, 24), FR, dtype=np.uint8)
    _craft(e, origin, state, absent=lambda pos: pos[:, 0] == 1)      # the middle block of three is not in the map
    points = _points([[21, 8 + y, -8 + z] for y in range(8) for z in range(8)], [-1, 0, 0])
    lamps = _lamps([[2, 12, -4], [12, 12, -4]])                       # the second one sits in UNKNOWN space
    state = ref.box_state(e, origin, dims)
    assert np.all(state[:, :, 8:16] == U) and np.all(state[:, :, :8] == FR)
    _, mask, table, _ = _check(e, origin, dims, points, lamps, state=state)
    assert np.all(mask == 3) and table["accepted"].tolist() == [1, 1]
    _, mask, table, summary = _check(e, origin, dims, points, lamps, state=state, unknown_occupied=True)
    assert np.all(mask == 0) and table["accepted"].tolist() == [1, 0] and summary["lamps_accepted"] == 1
    _check(e, [-1000, 900, -700], [24, 9, 17], points, lamps)         # no allocated block at all
    _check(e, [-1000, 900, -700], [24, 9, 17], points, lamps, unknown_occupied=True)


# 9
def test_accumulate(make_engine):
    e = make_engine(VS, TRUNC)
    origin, dims = [0, 0, 0], [16, 16, 12]
    state = _room(e, origin, (16, 16, 16), [(8, 8, z) for z in range(1, 6)])[:12]
    rng = np.random.default_rng(9)
    lamps = _lamps(np.stack([rng.integers(0, 16, 70), rng.integers(0, 16, 70), rng.integers(2, 12, 70)], 1),
                   rng.uniform(0.5, 2.0, 70).astype(F))
    points = e.surface_points(origin, dims)[:90]
    first = _check(e, origin, dims, points, lamps[:64], state=state)
    second = _check(e, origin, dims, points, lamps[64:], state=state, dose=first[0])
    sequential = np.zeros(len(points), dtype=F)
    for k in range(70):                                               # one restated sum, lamp by lamp
        sequential = ref.exposure(state, origin, VS, points, lamps[k:k + 1], dose=sequential)[0]
    assert ref.same_bytes(second[0], sequential) and first[3]["lit_pairs"] + second[3]["lit_pairs"] > 1000
    # a prior dose with awkward words: kept bit for bit where nothing is visible, summed on top elsewhere
    words = np.array([0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x7FC12345, 0x0DA24260, 0x40400000, 0x807FFFFF],
                     dtype=np.uint32).view(F)
    pts = np.concatenate([_points([[3, 3, 0]] * 8, [0, 0, 1]), _points([[3, 3, 0]] * 8, [0, 0, -1])])
    pts = pts[[0, 8, 1, 2, 3, 12, 5, 6, 7, 9, 10, 11]]                # the NaN word only with a point that faces away
    prior = words[[0, 0, 1, 2, 3, 4, 5, 6, 7, 1, 2, 3]]
    dose, mask, _, _ = _check(e, origin, dims, pts, _lamps([[3, 3, 6], [10, 3, 4], [3, 12, 8]]), state=state, dose=prior)
    dark = mask == 0
    assert dark.tolist() == [False, True, False, False, False, True, False, False, False, True, True, True]
    assert np.array_equal(dose.view(np.uint32)[dark], prior.view(np.uint32)[dark])
    assert dose[0] > 0 and np.signbit(dose[1]) and dose[3] == np.inf and dose[4] == -np.inf


# 10
def test_awkward_floats(make_engine):
    e = make_engine(VS, TRUNC)
    origin, dims = [-8, -8, -8], [24, 16, 16]
    state = np.full((16, 16, 24), FR, dtype=np.uint8)
    _craft(e, origin, state)
    base = _points([[0, 0, 0]], [0, 0, 1])[0]
    rows = []
    for pos, normal in [((0.0, 0.0, 0.0), (0, 0, 0)),                               # a zero normal
                        ((np.nan, 0.0, 0.0), (0, 0, 1)), ((0.0, np.inf, 0.0), (0, 0, 1)),
                        ((0.0, 0.0, -np.inf), (0, 0, 1)), ((1e-40, -1e-42, 1e-45), (0, 0, 1)),
                        ((0.0, 0.0, 0.0), (np.nan, 0, 1)), ((0.0, 0.0, 0.0), (0, 0, 1)),
                        ((0.03, 0.02, 0.05), (0, 0, 1)),                              # lamp 1 sits exactly here
                        ((0.03, 0.02, 0.0625), (0, 0, 1)),                            # lamp 2 at its height: c == 0
                        ((0.0, 0.0, 0.0), (1, 0, 0)),                                 # lamp 3: r2 == max_range^2 exactly
                        ((0.0, 0.0, 0.0), (3.0, -2.5, 0.25))]:                        # no unit normal: two voxels off
        p = base.copy()
        p["pos"], p["normal"] = pos, normal
        rows.append(p)
    points = np.array(rows, dtype=SURFACE_DTYPE)
    lamps = np.zeros(9, dtype=LAMP_DTYPE)
    lamps["pos"] = [(0.02, 0.01, 0.06), (0.03, 0.02, 0.05), (0.05, 0.05, 0.0625), (0.0625, 0.0, 0.0),
                    (0.01, 0.0, 0.03), (0.0, 0.01, 0.03), (np.nan, 0.0, 0.03), (0.0, np.inf, 0.03), (1e-41, 0.0, 0.04)]
    lamps["power"] = [1.0, 1.0, 1.0, 1.0, 0.0, np.inf, 1.0, 1.0, 1e-38]
    for max_range in (np.inf, 0.0625, float(np.nextafter(F(0.0625), F(0))), 0.0, 1e30, 1e-30):
        dose, mask, table, _ = _check(e, origin, dims, points, lamps, state=state, max_range=max_range)
        assert table["accepted"].tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 1]
        assert not np.any(np.isnan(dose))
        assert mask[0] == 0 and not mask[7] & 2 and not mask[8] & 4
        if max_range == np.inf:
            assert mask[6] & 16 and mask[6] & 32 and dose[6] == np.inf and mask[9] & 8
        if max_range == 0.0625:
            assert mask[9] & 8 and not mask[6] & 1                    # at the range exactly: in; lamp 0 is farther
        if max_range in (0.0, 1e-30) or max_range < 0.0625 and max_range > 0.06:
            assert not mask[9] & 8
    _check(e, origin, dims, points, lamps, state=state, min_irradiance=-np.inf, p_cutoff=np.inf)
    _check(e, origin, dims, points, lamps, state=state, min_irradiance=np.inf, p_cutoff=-np.inf)
    # a map whose every voxel is OCCUPIED below a threshold of +inf, FREE above one of -inf
    _check(e, origin, dims, points, lamps, occupied_below=np.inf)
    _check(e, origin, dims, points, lamps, occupied_below=-np.inf)


# 11
def test_sphere_map_against_the_oracle(maps):
    gpu, cpu = maps
    origin, dims = [-48, -32, 112], [96, 64, 48]
    state = ref.box_state(cpu, origin, dims)
    points = gpu.surface_points(origin, dims)[:2000]
    assert len(points) == 2000
    rng = np.random.default_rng(11)
    free = np.argwhere(state == FR)
    lamps = _lamps([_at(origin, v[::-1]) for v in free[rng.integers(0, len(free), 16)]], 10.0)
    for unknown_occupied in (False, True):
        _, mask, table, summary = _check(gpu, origin, dims, points, lamps, state=state,
                                         unknown_occupied=unknown_occupied, min_irradiance=5.0)
        assert np.all(table["accepted"] == 1)
        if not unknown_occupied:
            assert summary["points_lit"] > 0 and table["lit"].sum() <= summary["lit_pairs"]


def _device_buffers(n_points, n_lamps, prior=None):
    dose = np.full(n_points + 8, -7.0, dtype=F)
    if prior is not None:
        dose[:n_points] = prior
    return (devmem.DeviceArray(dose), devmem.DeviceArray(np.full(n_points + 8, 0xABABABABABABABAB, dtype=np.uint64)),
            devmem.DeviceArray(np.full((n_lamps + 2, 4), 0x6C6C6C6C, dtype=np.uint32)),
            devmem.DeviceArray(np.full(8 + 4, 0xEFEFEFEF, dtype=np.uint32)))


def _device_result(n_points, n_lamps, d_dose, d_mask, d_table, d_sum):
    dose, mask, table, summary = d_dose.numpy(), d_mask.numpy(), d_table.numpy(), d_sum.numpy()
    assert np.all(dose[n_points:] == -7.0) and np.all(mask[n_points:] == 0xABABABABABABABAB)
    assert np.all(table[n_lamps:] == 0x6C6C6C6C) and np.all(summary[8:] == 0xEFEFEFEF)
    return (dose[:n_points], mask[:n_points], table[:n_lamps].reshape(-1).view(LAMP_RECORD_DTYPE),
            summary[:8].view(EXPOSURE_SUMMARY_DTYPE)[0])


def _same(got, want):
    assert ref.same_bytes(got[0], want[0]) and ref.same_bytes(got[1], want[1]) and ref.same_bytes(got[2], want[2])
    assert got[3].tobytes() == want[3].tobytes()


# 12
def test_device_form(make_engine):
    import torch
    e = make_engine(VS, TRUNC)
    origin, dims = [-13, 5, -3], [20, 12, 9]
    state, points, lamps = _random_case(origin, dims, seed=12, n_points=333, n_lamps=21)
    state[0] = OC
    _craft(e, origin, state)
    floor = e.surface_points(origin, dims)
    points = np.concatenate([points, floor])
    n, m = len(points), len(lamps)
    want = _check(e, origin, dims, points, lamps, state=state, min_irradiance=30.0)
    assert want[3]["lit_pairs"] > 500 and want[3]["points_outside"] > 0
    d_points, d_lamps = devmem.DeviceArray(points), devmem.DeviceArray(lamps)
    # into devmem buffers, twice: identical bytes, nothing beyond the ends, OUTSIDE points keep what the buffer held
    for _ in range(2):
        bufs = _device_buffers(n, m)
        s = e.exposure_device(origin, dims, d_points, n, d_lamps, m, *bufs, min_irradiance=30.0)
        got = _device_result(n, m, *bufs)
        outside = (got[1] == 0) & (got[0] == -7.0)
        assert outside.sum() == want[3]["points_outside"] and s.tobytes() == want[3].tobytes()
        _same((np.where(outside, F(0), got[0]),) + got[1:], want)
    # into torch tensors, without a mask and without a table, on top of a prior dose
    prior = np.random.default_rng(3).uniform(0, 50, n).astype(F)
    want2 = ref.exposure(state, origin, VS, points, lamps, dose=prior)
    t_points = torch.from_numpy(points.view(np.uint8).reshape(n, 32)).cuda()
    t_lamps = torch.from_numpy(lamps.view(F).reshape(m, 4)).cuda()
    t_dose = torch.from_numpy(prior.copy()).cuda()
    t_sum = torch.full((8,), -3, dtype=torch.int32, device="cuda")
    s = e.exposure_device(origin, dims, t_points, n, t_lamps, m, t_dose, None, None, t_sum, accumulate=True)
    assert ref.same_bytes(t_dose.cpu().numpy(), want2[0]) and s["lit_pairs"] == want2[3]["lit_pairs"]
    # the points never leave the device
    got = e.surface_exposure(origin, dims, lamps, min_irradiance=30.0)
    assert ref.same_bytes(got[0], floor)
    _same(got[1:], ref.exposure(state, origin, VS, floor, lamps, min_irradiance=30.0))
    # the workspace grows, then serves a smaller box from the larger buffer
    big_o, big_d = [-20, 0, -8], [40, 24, 24]
    for o, d in ((big_o, big_d), (origin, dims), ([-13, 5, -3], [3, 2, 2])):
        _check(e, o, d, points, lamps)
    # ESDF, regions and exposure back to back on the stream, no synchronisation in between
    other_o, other_d = [-12, 6, -2], [17, 9, 6]
    want_field, want_state = e.esdf(other_o, other_d, with_state=True)
    want_labels, want_table = e.regions(other_o, other_d, 7)
    k = 17 * 9 * 6
    d_out, d_st = devmem.DeviceArray(np.zeros(k, dtype=F)), devmem.DeviceArray(np.zeros(k, dtype=np.uint8))
    d_lab = devmem.DeviceArray(np.zeros(k, dtype=np.int32))
    d_reg = devmem.DeviceArray(np.zeros((len(want_table) + 1, 32), dtype=np.uint8))
    d_cnt = devmem.DeviceArray(np.zeros(1, dtype=np.int64))
    from ratsdf._abi import RegionsParams
    box = [(C.c_int32 * 3)(*v) for v in (origin, dims)]
    other = [(C.c_int32 * 3)(*v) for v in (other_o, other_d)]
    bufs = _device_buffers(n, m)
    params = ExposureParams(0.0, float("inf"), 30.0, 0.5, 0, (C.c_uint32 * 3)(0, 0, 0))
    e.esdf_device(other_o, other_d, d_out.data_ptr(), d_st.data_ptr())
    assert e.lib.fn["exposure_device"](e._h, *box, C.byref(params), d_points.data_ptr(), n, d_lamps.data_ptr(), m,
                                       *(b.data_ptr() for b in bufs)) == 0
    assert e.lib.fn["regions_device"](e._h, *other, C.byref(RegionsParams(0.0, 0.0, 7, 0)), d_lab.data_ptr(),
                                      d_reg.data_ptr(), len(want_table) + 1, d_cnt.data_ptr()) == 0
    e.synchronize()
    got = _device_result(n, m, *bufs)
    _same((np.where(got[0] == -7.0, F(0), got[0]),) + got[1:], want)
    assert ref.same_bytes(d_out.numpy().reshape(want_field.shape), want_field)
    assert ref.same_bytes(d_st.numpy().reshape(want_state.shape), want_state)
    assert ref.same_bytes(d_lab.numpy().reshape(want_labels.shape), want_labels)
    assert ref.same_bytes(d_reg.numpy()[:len(want_table)].reshape(-1).view(want_table.dtype), want_table)


def test_after_a_carving_batch(make_engine, make_oracle, churn):
    """the call applies the last frame's deferred pool releases first: right after a batch that carved blocks away the
    states are those of the map the batch left"""
    gpu, cpu = make_engine(VS, TRUNC), make_oracle(VS, TRUNC, threads=8)
    _integrate([gpu, cpu], churn[:8])
    origin, dims = [-48, -32, 112], [96, 64, 48]
    points = gpu.surface_points(origin, dims)[:500]
    _integrate([gpu, cpu], churn[8:12])
    lamps = _lamps([_at(origin, v) for v in [(10, 10, 4), (80, 50, 6), (48, 32, 2)]], 5.0)
    got = gpu.exposure(origin, dims, points, lamps, with_mask=True)
    _same(got, ref.exposure(ref.box_state(cpu, origin, dims), origin, VS, points, lamps))
    assert_maps_equal(gpu, cpu)


# 13
def test_the_map_is_only_read(make_engine, make_oracle, churn):
    gpu, cpu = make_engine(VS, TRUNC), make_oracle(VS, TRUNC, threads=8)
    _integrate([gpu, cpu], churn[:6])
    before = _snapshot(gpu)
    origin, dims = [-48, -32, 112], [96, 64, 48]
    points = gpu.surface_points(origin, dims)[:300]
    lamps = _lamps([_at(origin, v) for v in [(10, 10, 4), (80, 50, 6)]])
    _, _, _, summary = gpu.exposure(origin, dims, points, lamps, with_mask=True)
    gpu.surface_exposure(origin, dims, lamps, unknown_occupied=True)
    assert summary["lamps_accepted"] >= 1
    _same_snapshot(before, _snapshot(gpu))
    _integrate([gpu, cpu], churn[6:10])
    assert_maps_equal(gpu, cpu)


def test_sticky_error_is_returned(make_engine):
    import ratsdf
    small = make_engine(VS, TRUNC, block_bits=6)   # 64 blocks: the first frame exhausts the pool
    f = synthetic.frame("room", 0, scale=0.25)
    with pytest.raises(ratsdf.RatsdfError) as ei:
        _integrate([small], [f])
        small.synchronize()
    assert ei.value.status == 3
    points, lamps = _points([[1, 1, 1]], [0, 0, 1]), _lamps([[1, 1, 5]])
    with pytest.raises(ratsdf.RatsdfError) as ei:
        small.exposure([0, 0, 0], [8, 8, 8], points, lamps)
    assert ei.value.status == 3
    bufs = _device_buffers(1, 1)
    with pytest.raises(ratsdf.RatsdfError) as ei:
        small.exposure_device([0, 0, 0], [8, 8, 8], devmem.DeviceArray(points), 1, devmem.DeviceArray(lamps), 1, *bufs)
    assert ei.value.status == 3


def test_refusals(make_engine):
    e = make_engine(VS, TRUNC)
    _craft(e, [0, 0, 0], np.full((4, 4, 4), FR, dtype=np.uint8))
    host, device = e.lib.fn["exposure"], e.lib.fn["exposure_device"]
    vec = lambda v: (C.c_int32 * 3)(*v) if v is not None else None   # noqa: E731
    ok_o, ok_d = [0, 0, 0], [4, 4, 4]
    ok_params = (0.0, float("inf"), 0.0, 0.5, 0, (0, 0, 0))
    points, lamps = _points([[1, 1, 0], [2, 2, 0]], [0, 0, 1]), _lamps([[1, 1, 3], [2, 2, 2], [3, 0, 3]])
    dose = np.full(4, 0x5A5A5A5A, dtype=np.uint32)
    mask = np.full(4, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    table = np.full(16, 0x5A5A5A5A, dtype=np.uint32)
    summary = np.full(8, 0x5A5A5A5A, dtype=np.uint32)
    d_points, d_lamps = devmem.DeviceArray(np.concatenate([points, points])), devmem.DeviceArray(np.concatenate([lamps, lamps]))
    d_dose = devmem.DeviceArray(np.full(4, 0x6B6B6B6B, dtype=np.uint32))
    d_mask = devmem.DeviceArray(np.full(4, 0x6B6B6B6B6B6B6B6B, dtype=np.uint64))
    d_table = devmem.DeviceArray(np.full(24, 0x6B6B6B6B, dtype=np.uint32))
    d_sum = devmem.DeviceArray(np.full(12, 0x6B6B6B6B, dtype=np.uint32))

    def par(p):
        return C.byref(ExposureParams(*p[:5], (C.c_uint32 * 3)(*p[5]))) if p else None

    def call_host(origin=ok_o, dims=ok_d, params=ok_params, p=points.ctypes.data, n=2, l=lamps.ctypes.data, m=3,
                  d=dose.ctypes.data, k=mask.ctypes.data, t=table.ctypes.data, s=summary.ctypes.data):
        return host(e._h, vec(origin), vec(dims), par(params), p or None, n, l or None, m, d or None, k or None,
                    t or None, s or None)

    def call_device(origin=ok_o, dims=ok_d, params=ok_params, p=d_points.data_ptr(), n=2, l=d_lamps.data_ptr(), m=3,
                    d=d_dose.data_ptr(), k=d_mask.data_ptr(), t=d_table.data_ptr(), s=d_sum.data_ptr()):
        return device(e._h, vec(origin), vec(dims), par(params), p or None, n, l or None, m, d or None, k or None,
                      t or None, s or None)

    refused = 0

    def both(**kw):
        nonlocal refused
        assert call_host(**kw) == 1, kw
        assert call_device(**kw) == 1, kw
        refused += 1

    for origin, dims in [([0, 0, 0], [0, 4, 4]), ([0, 0, 0], [4, -1, 4]), ([0, 0, 0], [4, 4, 1025]),
                         ([0, 0, 0], [1024, 1024, 129]), ([-32769, 0, 0], [4, 4, 4]), ([0, 32765, 0], [4, 4, 4]),
                         ([0, 0, 40000], [4, 4, 4]), (None, ok_d), (ok_o, None)]:
        both(origin=origin, dims=dims)
    nan, inf = float("nan"), float("inf")
    for params in (None, (nan, inf, 0.0, 0.5, 0, (0, 0, 0)), (0.0, nan, 0.0, 0.5, 0, (0, 0, 0)),
                   (0.0, -1.0, 0.0, 0.5, 0, (0, 0, 0)), (0.0, -inf, 0.0, 0.5, 0, (0, 0, 0)),
                   (0.0, inf, nan, 0.5, 0, (0, 0, 0)), (0.0, inf, 0.0, nan, 0, (0, 0, 0)),
                   (0.0, inf, 0.0, 0.5, 4, (0, 0, 0)), (0.0, inf, 0.0, 0.5, 1 << 31, (0, 0, 0)),
                   (0.0, inf, 0.0, 0.5, 0, (1, 0, 0)), (0.0, inf, 0.0, 0.5, 0, (0, 0, 7))):
        both(params=params)
    both(n=-1)
    both(n=(1 << 24) + 1)
    both(m=-1)
    both(m=65)
    both(p=0, n=1)
    both(l=0, m=1)
    both(d=0)
    both(s=0)
    for kw in (dict(p=d_points.data_ptr() + 8), dict(l=d_lamps.data_ptr() + 4), dict(t=d_table.data_ptr() + 8),
               dict(k=d_mask.data_ptr() + 4), dict(s=d_sum.data_ptr() + 4), dict(d=d_dose.data_ptr() + 2)):
        assert call_device(**kw) == 1, kw                             # misaligned
    e.synchronize()
    assert refused == 28
    assert np.all(dose == 0x5A5A5A5A) and np.all(mask == 0x5A5A5A5A5A5A5A5A) and np.all(table == 0x5A5A5A5A)
    assert np.all(summary == 0x5A5A5A5A)
    assert np.all(d_dose.numpy() == 0x6B6B6B6B) and np.all(d_mask.numpy() == 0x6B6B6B6B6B6B6B6B)
    assert np.all(d_table.numpy() == 0x6B6B6B6B) and np.all(d_sum.numpy() == 0x6B6B6B6B)
    # what is allowed
    assert call_host() == 0 and mask[:2].tolist() == [7, 7] and np.all(mask[2:] == 0x5A5A5A5A5A5A5A5A)
    assert summary.view(EXPOSURE_SUMMARY_DTYPE)[0]["lit_pairs"] == 6 and np.all(table[12:] == 0x5A5A5A5A)
    assert call_host(k=0) == 0 and call_host(t=0) == 0 and call_host(p=0, n=0) == 0 and call_host(l=0, m=0) == 0
    assert call_host(params=(0.0, 0.0, 0.0, 0.5, 3, (0, 0, 0))) == 0 and call_host(params=(0.0, -0.0, 0.0, 0.5, 0, (0, 0, 0))) == 0
    assert call_device() == 0 and call_device(k=0, t=0) == 0 and call_device(p=0, n=0) == 0
    assert call_device(l=0, m=0) == 0 and call_device(d=d_dose.data_ptr() + 4, k=d_mask.data_ptr() + 8, n=1) == 0
    assert call_device(p=d_points.data_ptr() + 32, l=d_lamps.data_ptr() + 16, t=d_table.data_ptr() + 16) == 0
    e.synchronize()
    assert d_sum.numpy()[:8].view(EXPOSURE_SUMMARY_DTYPE)[0]["lit_pairs"] == 6 and np.all(d_sum.numpy()[8:] == 0x6B6B6B6B)
    # the limit itself: 64 lamps on one point
    many = _lamps([[x % 4, x // 4 % 4, 1 + x // 16] for x in range(48)] + [[1, 1, 3]] * 16)
    _, m64, t64, s64 = e.exposure(ok_o, ok_d, points[:1], many, with_mask=True)
    assert s64["lamps_accepted"] == 64 and m64[0] == np.uint64(0xFFFFFFFFFFFFFFFF) and np.all(t64["lit"] == 1)
