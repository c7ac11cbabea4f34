"""The numpy restatement of the point-sampling contract (tests/sample_ref.py) checked on its own: no GPU, no engine."""
import numpy as np

import sample_ref as ref
from ratsdf._abi import SAMPLE_ALLOCATED, SAMPLE_NEAREST, SAMPLE_OBSERVED

VS = np.float32(0.01)


def _field(lo, hi, fn, weight=5):
    """every voxel of the box [lo, hi] (voxel coordinates) holding tsdf fn(x, y, z)"""
    vox = {}
    for x in range(lo[0], hi[0] + 1):
        for y in range(lo[1], hi[1] + 1):
            for z in range(lo[2], hi[2] + 1):
                vox[(x, y, z)] = (np.float32(fn(x, y, z)), (x & 255, y & 255, z & 255, weight),
                                  np.float32(((x * 7 + y * 3 + z) % 10) / 10))
    return vox


def _linear():
    a = np.array([0.011, -0.007, 0.013], dtype=np.float32)
    b = np.float32(0.25)
    return a, b, _field((-10, -10, -10), (10, 10, 10), lambda x, y, z: a[0] * x + a[1] * y + a[2] * z + b)


def test_linear_field_and_exact_gradient():
    a, b, vox = _linear()
    rng = np.random.default_rng(1)
    g = rng.uniform(-9.5, 9.5, size=(2000, 3)).astype(np.float32)
    p = (g * VS).astype(np.float32)
    s = ref.sample(p, VS, ref.dict_lookup(vox))
    assert np.all(s["flags"] == SAMPLE_ALLOCATED | SAMPLE_OBSERVED | SAMPLE_NEAREST)
    gg = (p / VS).astype(np.float64)
    want = gg @ a.astype(np.float64) + float(b)
    assert np.max(np.abs(s["tsdf"] - want)) < 1e-5
    assert np.allclose(s["grad"], (a / VS)[None, :], rtol=1e-4, atol=0)
    assert np.all(s["min_weight"] == 5) and np.all(s["reserved"] == 0)


def test_integer_points_return_the_voxel_itself():
    _, _, vox = _linear()
    vs = np.float32(2.0 ** -6)   # p / vs exactly integral
    g = np.array([[x, y, z] for x in (-4, 0, 3) for y in (-1, 2) for z in (-3, 5)], dtype=np.float32)
    p = (g * vs).astype(np.float32)
    assert np.array_equal(p / vs, g)
    s = ref.sample(p, vs, ref.dict_lookup(vox))
    for i, k in enumerate(map(tuple, g.astype(int).tolist())):
        assert s["tsdf"][i] == vox[k][0]
        assert s["prob"][i] == vox[k][2]
        assert tuple(s["rgbw"][i]) == vox[k][1]


def test_nearest_voxel_is_a_corner():
    _, _, vox = _linear()
    rng = np.random.default_rng(2)
    g = rng.uniform(-8, 8, size=(3000, 3)).astype(np.float32)
    g[:500] = np.floor(g[:500]) + np.float32(0.5)   # halves: away from zero
    p = (g * VS).astype(np.float32)
    s = ref.sample(p, VS, ref.dict_lookup(vox))
    gg = p / VS
    near = ref.round_half_away(gg)
    fl = np.floor(gg)
    assert np.all((near == fl) | (near == fl + 1))
    for i in range(0, 3000, 7):
        k = tuple(int(v) for v in near[i])
        assert s["prob"][i] == vox[k][2] and tuple(s["rgbw"][i]) == vox[k][1]
    # half away from zero on both sides of 0
    assert list(ref.round_half_away(np.array([-2.5, -0.5, 0.5, 2.5, -0.49999997], dtype=np.float32))) == [-3, -1, 1, 3, 0]


def test_nan_and_int16_range_rules():
    _, _, vox = _linear()
    # a block at the top of the int16 range, and its image under a plain (int16_t) cast of 32768 + 5
    vox.update(_field((32760, 0, 0), (32767, 1, 1), lambda x, y, z: 0.5))
    vox.update(_field((-32768, 0, 0), (-32760, 1, 1), lambda x, y, z: -0.5))
    pts = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf],
                    [32767.5, 0.2, 0.2],        # corner x = 32768: outside
                    [32773.2, 0.2, 0.2],        # would wrap onto x = -32763 under an int16 cast
                    [-32768.5, 0.2, 0.2],       # corner x = -32769: outside
                    [32766.5, 0.2, 0.2],        # last cell inside
                    [-32768.0, 0.2, 0.2]], dtype=np.float32) * VS
    pts = pts.astype(np.float32)
    s = ref.sample(pts, VS, ref.dict_lookup(vox))
    default = np.zeros(1, dtype=s.dtype)
    default["tsdf"] = ref.QNAN
    default["grad"] = ref.QNAN
    for i in range(6):
        assert ref.same_bytes(s[i:i + 1], default), i
    assert s["flags"][6] & SAMPLE_ALLOCATED and s["tsdf"][6] == np.float32(0.5)
    assert s["flags"][7] & SAMPLE_ALLOCATED and s["tsdf"][7] == np.float32(-0.5)
    # unallocated corners: NaN bits exactly, min_weight 0; nearest voxel present -> NEAREST only
    half = _field((0, 0, 0), (0, 3, 3), lambda x, y, z: 0.1)
    s = ref.sample(np.array([[0.2, 1.2, 1.2]], dtype=np.float32) * VS, VS, ref.dict_lookup(half))
    assert s["flags"][0] == SAMPLE_NEAREST and s["min_weight"][0] == 0
    assert s["tsdf"].view(np.uint32)[0] == 0x7FC00000 and np.all(s["grad"].view(np.uint32) == 0x7FC00000)


def test_mirrored_pairing_differs_off_the_cell_centre():
    """RetrieveTSDF's corner / weight pairing reproduces the linear field only at cell centres; at an integer point it
    returns the voxel one step up every axis"""
    a, b, vox = _linear()
    look = ref.dict_lookup(vox)
    g = np.array([[1.25, -2.75, 3.1], [0.5, 0.5, 0.5], [2.0, 3.0, -1.0]], dtype=np.float32)
    l = np.floor(g).astype(np.int64)

    def corner(i, j, k):
        return look(l + np.array([i, j, k]))[1]

    mirrored = ref.mirrored_tsdf(g, corner)
    s = ref.sample((g * VS).astype(np.float32), VS, look)
    want = g.astype(np.float64) @ a.astype(np.float64) + float(b)
    assert abs(s["tsdf"][0] - want[0]) < 1e-5
    assert abs(mirrored[0] - want[0]) > 1e-3     # off the centre: mirrored
    assert abs(mirrored[1] - want[1]) < 1e-5     # cell centre: the same
    assert mirrored[2] == look(l[2:3] + 1)[1][0]  # integer point: the neighbour at +1
    assert s["tsdf"][2] == look(l[2:3])[1][0]     # ... the point query: the voxel itself
