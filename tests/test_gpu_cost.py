"""The cost-to-go field of the HIP engine (include/ratsdf_cost.h) against the restatement of the contract
(tests/cost_ref.py): cost, next and summary byte for byte, with the box's states read from the CPU oracle's map where one
exists.  The crafted maps are the smallest at which each phase can go wrong: the relaxation works on 32 x 8 x 4 tiles of
the box and hands changes from tile to tile between launches.

The summary's `rounds` is the one field the contract does not define for the host form (how many rounds it took depends
on what a tile saw of its neighbours in the same round): it is checked to be a positive count and otherwise taken from
the engine."""
import ctypes as C

import numpy as np
import pytest

import cost_ref as ref
from parity import assert_maps_equal
from ratsdf import synthetic
from ratsdf._abi import COST_SUMMARY_DTYPE, CostParams
from test_gpu_regions import _craft, _integrate, _same_snapshot, _snapshot

pytestmark = pytest.mark.gpu

VS, TRUNC = 0.01, 0.06
U, FR, OC = ref.UNKNOWN, ref.FREE, ref.OCCUPIED
NONE = ref.NONE


def _want(state, origin, goals, clearance=0.0, unknown_occupied=False, through_unknown=False, faces_only=False):
    trav = ref.traversable(state, VS, clearance, unknown_occupied, through_unknown)
    idx = ref.accept(goals, origin, trav)
    cost = ref.exact(trav, idx, faces_only)
    return trav, idx, cost, ref.next_of(cost, trav, faces_only), ref.summary_of(cost, trav)


def _check(gpu, src, origin, dims, goals, clearance=0.0, occupied_below=0.0, state=None, **flags):
    """the engine's cost, next and summary against the restatement fed by `src`'s map; returns (cost, next, summary,
    trav)"""
    what = (origin, dims, clearance, flags)
    if state is None:
        state = ref.box_state(src, origin, dims, occupied_below)
    trav, idx, want, want_next, want_sum = _want(state, origin, goals, clearance, **flags)
    cost, nxt, summary = gpu.cost_to_go(origin, dims, goals, clearance, occupied_below, with_next=True, **flags)
    assert summary.dtype == COST_SUMMARY_DTYPE == ref.SUMMARY_DTYPE
    assert ref.same_bytes(cost, want), what
    assert ref.same_bytes(nxt, want_next), what
    assert summary["rounds"] >= 1 and summary["pending"] == 0, what
    want_sum["rounds"] = summary["rounds"]
    assert summary.tobytes() == want_sum.tobytes(), (what, summary, want_sum)
    only_cost, s2 = gpu.cost_to_go(origin, dims, goals, clearance, occupied_below, **flags)
    assert ref.same_bytes(only_cost, cost) and s2["reached"] == summary["reached"], what
    return cost, nxt, summary, trav


def _mask_case(e, origin, free, goals, **kw):
    """a mask as FREE voxels among OCCUPIED ones (and OCCUPIED around the box)"""
    state = np.where(free, FR, OC).astype(np.uint8)
    _craft(e, origin, state, outside=OC)
    return _check(e, e, list(origin), list(free.shape[::-1]), goals, **kw)


def _at(origin, x, y, z):
    return [origin[0] + x, origin[1] + y, origin[2] + z]


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
    e = make_engine(VS, TRUNC)
    origin, dims = [-13, 5, -3], [20, 12, 9]
    _craft(e, origin, np.full((9, 12, 20), FR, dtype=np.uint8))
    cost, nxt, summary, _ = _check(e, e, origin, dims, [_at(origin, 7, 5, 3)])
    assert ref.same_bytes(cost, ref.closed_form((9, 12, 20), (7, 5, 3)))
    assert summary["goals"] == 1 and summary["reached"] == summary["traversable"] == 20 * 12 * 9
    cost, _, _, _ = _check(e, e, origin, dims, [_at(origin, 7, 5, 3)], faces_only=True)
    z, y, x = np.indices((9, 12, 20))
    assert np.array_equal(cost, 10 * (abs(x - 7) + abs(y - 5) + abs(z - 3)))
    _check(e, e, [-11, 6, -1], [1, 1, 1], [[-11, 6, -1]])                      # one voxel, its own goal


# 2
@pytest.mark.parametrize("faces_only", [False, True])
def test_tile_seams(make_engine, faces_only):
    """70 x 20 x 9 crosses tile borders in x at 32 and 64, in y at 8 and 16, in z at 4 and 8"""
    e = make_engine(VS, TRUNC)
    for origin, mirrored in (([0, 0, 0], False), ([-45, 200, -3], True)):
        free = ref.serpentine((9, 20, 70), mirrored)
        start = _at(origin, 69, 19, 8) if mirrored else _at(origin, 0, 0, 0)
        cost, _, summary, _ = _mask_case(e, origin, free, [start], faces_only=faces_only)
        assert summary["reached"] == free.sum()
        if faces_only:
            assert summary["max_cost"] == 10 * (free.sum() - 1)   # the path is a chain of face moves
    for origin, shape, y0, y1, z in (([0, 100, 0], (6, 21, 70), 2, 17, 5), ([-70, -100, -9], (9, 21, 100), 17, 2, 4)):
        free = ref.comb(shape, y0, y1, z=z)                        # the goal at the free end of one tooth
        cost, _, summary, _ = _mask_case(e, origin, free, [_at(origin, 0, y0, z)], faces_only=faces_only)
        assert summary["reached"] == free.sum()
        if faces_only:
            assert cost[z, y1, 0] == 10 * (2 * (shape[2] - 1) + abs(y1 - y0))


# 2b
@pytest.mark.parametrize("faces_only", [False, True])
def test_goal_on_a_tile_face(make_engine, faces_only):
    """a goal's word is lowered before round 0, so nobody sees it fall: where the goal is the only voxel through which a
    path crosses a tile face (edge, corner), the tile on the other side must be marked for it.  One-voxel-wide
    corridors across the seams x = 31 | 32, y = 7 | 8 and z = 3 | 4, a diagonal through the corner of eight tiles, and
    a box one voxel thick, with the goal on either side of the seam; the host form and the device form without
    CONTINUE"""
    from ratsdf import devmem
    e = make_engine(VS, TRUNC)
    cases = []
    for axis, shape in ((0, (3, 3, 40)), (1, (3, 12, 3)), (2, (7, 3, 3))):      # corridors along x, y, z
        free = np.zeros(shape, dtype=bool)
        line = [1, 1, 1]
        line[2 - axis] = slice(None)
        free[tuple(line)] = True
        seam = (31, 7, 3)[axis]
        for at in (seam, seam + 1):
            goal = [1, 1, 1]
            goal[axis] = at
            cases.append((free, goal))
    diag = np.zeros((8, 12, 36), dtype=bool)
    for k in range(8):
        diag[k, 4 + k, 28 + k] = True                              # (31, 7, 3) and (32, 8, 4) meet in a corner only
    cases += [(diag, [31, 7, 3]), (diag, [32, 8, 4])]
    thin = np.ones((1, 1, 64), dtype=bool)
    cases += [(thin, [31, 0, 0]), (thin, [32, 0, 0])]
    for k, (free, goal) in enumerate(cases):
        origin = [-5 + 64 * k, 11, -2]                             # (unaligned to blocks; tiles start at the box's origin)
        dims = list(free.shape[::-1])
        cost, _, summary, trav = _mask_case(e, origin, free, [_at(origin, *goal)], faces_only=faces_only)
        if free is not diag:
            assert summary["reached"] == free.sum(), (free.shape, goal)       # both sides of the seam
        elif not faces_only:
            assert summary["reached"] == 8 and summary["max_cost"] == 17 * max(goal[2], 7 - goal[2])
        n = free.size
        d_goals = devmem.DeviceArray(np.array([_at(origin, *goal)], dtype=np.int32))
        d_cost, d_next, d_sum = _device_buffers(n)
        s = e.cost_to_go_device(origin, dims, d_goals, 1, d_cost, d_next, d_sum, rounds=8, faces_only=faces_only)
        assert s["pending"] == 0 and s["reached"] == summary["reached"], (free.shape, goal)
        assert ref.same_bytes(d_cost.numpy()[:n].reshape(cost.shape), cost), (free.shape, goal)


# 3
def test_goals(make_engine):
    e = make_engine(VS, TRUNC)
    origin, dims = [3, -20, 40], [45, 19, 11]
    state = np.full((11, 19, 45), FR, dtype=np.uint8)
    state[:, :, 20] = OC                                           # a wall: two rooms
    state[2:9, 5:12, 30:38] = OC
    _craft(e, origin, state)
    inside = [_at(origin, 2, 3, 4), _at(origin, 44, 18, 10), _at(origin, 10, 10, 0)]
    cost, _, summary, _ = _check(e, e, origin, dims, inside)
    assert summary["goals"] == 3
    _check(e, e, origin, dims, inside + inside[:2] + inside)       # duplicates
    outside = [_at(origin, -1, 3, 4), _at(origin, 45, 0, 0), _at(origin, 0, 19, 0), _at(origin, 0, 0, -1),
               [2 ** 31 - 1, 0, 0], [-2 ** 31, -2 ** 31, -2 ** 31]]
    cost, _, summary, _ = _check(e, e, origin, dims, outside + inside[:1])
    assert summary["goals"] == 1 and np.all(cost[:, :, 21:] == NONE)          # the other room is not reached
    walled = [_at(origin, 20, 3, 3), _at(origin, 33, 8, 5)]                    # on OCCUPIED voxels
    eroded = [_at(origin, 19, 3, 3)]                                           # FREE, but next to the wall
    cost, _, summary, _ = _check(e, e, origin, dims, walled + eroded + inside[:1], clearance=1.5 * VS)
    assert summary["goals"] == 1
    for goals in ([], outside, walled, np.zeros((0, 3), dtype=np.int32)):
        cost, nxt, summary, _ = _check(e, e, origin, dims, goals)
        assert np.all(cost == NONE) and np.all(nxt == ref.NO_STEP)
        assert summary["goals"] == summary["reached"] == summary["max_cost"] == 0 and summary["traversable"] > 0


# 4
def test_clearance(make_engine):
    e = make_engine(VS, TRUNC)
    origin, dims = [-21, 9, 3], [40, 24, 12]
    state = np.full((12, 24, 40), FR, dtype=np.uint8)
    for x, y in ((6, 5), (11, 16), (30, 8), (34, 19)):
        state[:, y, x] = OC                                        # pillars
    state[:, :, 20] = OC
    state[:, 10:14, 20] = FR                                       # a wall with a door four voxels wide
    _craft(e, origin, state, outside=OC)                           # OCCUPIED one voxel outside the box: not seen
    goal = [_at(origin, 2, 2, 2)]
    two = float(np.float32(2) * np.float32(VS))
    reached = []
    for clearance in (0.0, VS, two, 2.5 * VS):
        cost, _, summary, trav = _check(e, e, origin, dims, goal, clearance=clearance)
        reached.append(int(summary["reached"]))
        assert trav[0, 0, 0] and trav[11, 23, 39]                  # the box's faces are not eroded from outside
        if clearance == two:
            assert trav[5, 11, 20] and trav[5, 12, 20] and not trav[5, 10, 20]    # exactly at the clearance: kept
            assert cost[5, 12, 25] != NONE
        if clearance == 2.5 * VS:
            assert not trav[:, :, 20].any()                        # the door is closed ...
            assert trav[5, 12, 30] and np.all(cost[:, :, 21:] == NONE)           # ... the far room a pocket
    # (every voxel outside O is at least one voxel from it: a clearance of vs erodes nothing)
    assert reached[0] == reached[1] > reached[2] > reached[3] > 0
    _check(e, e, origin, dims, goal, clearance=-1.0)
    _check(e, e, origin, dims, goal, clearance=float("inf"))       # nothing is that far from an obstacle
    _check(e, e, origin, dims, goal, clearance=two, faces_only=True)


# 5
def test_unknown_space(make_engine):
    e = make_engine(VS, TRUNC)
    rng = np.random.default_rng(11)
    origin, dims = [-45, -11, -3], [37, 29, 23]
    state = np.where(rng.random((23, 29, 37)) < 0.12, OC, FR).astype(np.uint8)
    state[:, 12:17, :] = np.where(rng.random((23, 5, 37)) < 0.7, U, state[:, 12:17, :])
    _craft(e, origin, state, outside=U, absent=lambda pos: (pos[:, 0] + pos[:, 1] + pos[:, 2]) % 4 == 0)
    got = ref.box_state(e, origin, dims)
    assert (got == U).sum() > (state == U).sum()                   # absent blocks and zero-weight voxels
    free = np.argwhere(got == FR)
    goals = [_at(origin, int(x), int(y), int(z)) for z, y, x in free[[0, len(free) // 2, -1]]]
    cost, _, plain, trav = _check(e, e, origin, dims, goals, state=got)
    assert not trav[got == U].any() and np.all(cost[got == U] == NONE)
    _, _, through, trav = _check(e, e, origin, dims, goals, state=got, through_unknown=True)
    assert trav[got == U].all() and through["reached"] > plain["reached"]
    _, _, eroded, trav = _check(e, e, origin, dims, goals, state=got, unknown_occupied=True, clearance=1.5 * VS)
    _, _, kept, _ = _check(e, e, origin, dims, goals, state=got, clearance=1.5 * VS)
    assert eroded["traversable"] < kept["traversable"]


# 6
@pytest.mark.parametrize("density", [0.3, 0.6, 0.9])
def test_random_density_and_descent(make_engine, density):
    import ratsdf
    e = make_engine(VS, TRUNC)
    origin = [-19, 3, -12]
    free = ref.random_mask((11, 19, 45), density, seed=int(density * 100))
    at = np.argwhere(free)
    goals = [_at(origin, int(x), int(y), int(z)) for z, y, x in at[[1, len(at) // 2, -2]]]
    cost, nxt, summary, _ = _mask_case(e, origin, free, goals)
    _mask_case(e, origin, free, goals, faces_only=True)
    assert summary["goals"] == 3
    for z, y, x in np.argwhere(cost != NONE):
        path = ratsdf.descend(nxt, origin, _at(origin, int(x), int(y), int(z)))
        end = path[-1] - origin
        assert cost[end[2], end[1], end[0]] == 0 and ref.path_weight(path) == cost[z, y, x]
    for z, y, x in np.argwhere(cost == NONE)[:5]:
        assert len(ratsdf.descend(nxt, origin, _at(origin, int(x), int(y), int(z)))) == 1


# 7
def test_ends_of_the_grid(make_engine):
    e = make_engine(VS, TRUNC)
    for origin in ([-32768, -32768, -32768], [32767 - 8, 32767 - 4, 32767 - 5]):
        free = ref.random_mask((6, 5, 9), 0.8, seed=7)
        at = np.argwhere(free)
        z, y, x = at[len(at) // 2]
        _, _, summary, _ = _mask_case(e, origin, free, [_at(origin, int(x), int(y), int(z))])
        assert summary["reached"] > 1


# 8
def test_sphere_map_against_the_oracle(maps):
    gpu, cpu = maps
    origin, dims = [-48, -32, 112], [96, 64, 48]
    state = ref.box_state(cpu, origin, dims)
    free = np.argwhere(state == FR)
    assert len(free) > 1000
    goals = [_at(origin, int(x), int(y), int(z)) for z, y, x in free[[0, len(free) // 3, 2 * len(free) // 3]]]
    for clearance in (0.0, 3 * VS):
        _, _, summary, _ = _check(gpu, cpu, origin, dims, goals, clearance=clearance, state=state)
        if clearance == 0.0:
            assert summary["goals"] == 3 and summary["reached"] > 1000
    _check(gpu, cpu, [-1000, 900, -700], [24, 9, 17], [[-990, 903, -690]])     # no allocated block: nothing to walk on
    _, _, summary, _ = _check(gpu, cpu, [-1000, 900, -700], [24, 9, 17], [[-990, 903, -690]], through_unknown=True)
    assert summary["reached"] == 24 * 9 * 17


def _device_buffers(n):
    from ratsdf import devmem
    return (devmem.DeviceArray(np.full(n + 64, 0xABABABAB, dtype=np.uint32)),
            devmem.DeviceArray(np.full(n + 64, 0xCD, dtype=np.uint8)),
            devmem.DeviceArray(np.full(8 + 8, 0xEFEFEFEF, dtype=np.uint32)))


# 9
def test_device_form_bounded_rounds(make_engine):
    from ratsdf import devmem
    e = make_engine(VS, TRUNC)
    origin, dims = [0, 0, 0], [70, 20, 9]
    n = 70 * 20 * 9
    free = ref.serpentine((9, 20, 70))
    state = np.where(free, FR, OC).astype(np.uint8)
    _craft(e, origin, state, outside=OC)
    host_cost, host_next, host_sum = e.cost_to_go(origin, dims, [[0, 0, 0]], with_next=True)
    trav, idx, want, want_next, _ = _want(state, origin, [[0, 0, 0]])
    assert ref.same_bytes(host_cost, want)
    d_goals = devmem.DeviceArray(np.array([[0, 0, 0]], dtype=np.int32))
    d_cost, d_next, d_sum = _device_buffers(n)
    s = e.cost_to_go_device(origin, dims, d_goals, 1, d_cost, d_next, d_sum, rounds=1)
    assert s["pending"] > 0 and s["rounds"] == 1 and s["goals"] == 1 and s["traversable"] == free.sum()
    cost = d_cost.numpy()[:n].reshape(want.shape)
    assert 1 < s["reached"] == (cost != NONE).sum() < free.sum()
    assert ref.unconverged_ok(cost, want, trav, idx)
    assert ref.same_bytes(d_next.numpy()[:n].reshape(want.shape), ref.next_of(cost, trav))
    calls = 0
    while s["pending"] != 0:
        calls += 1
        assert calls <= 4                                          # a condition: 114 rounds suffice tile by tile
        s = e.cost_to_go_device(origin, dims, d_goals, 1, d_cost, d_next, d_sum, rounds=64, resume=True)
        assert s["rounds"] == 64
        assert ref.unconverged_ok(d_cost.numpy()[:n].reshape(want.shape), want, trav, idx)
    assert ref.same_bytes(d_cost.numpy()[:n].reshape(want.shape), host_cost)
    assert ref.same_bytes(d_next.numpy()[:n].reshape(want.shape), host_next)
    got = d_sum.numpy()[:8].view(COST_SUMMARY_DTYPE)[0].copy()
    got["rounds"] = host_sum["rounds"]
    assert got.tobytes() == host_sum.tobytes()
    assert np.all(d_cost.numpy()[n:] == 0xABABABAB) and np.all(d_next.numpy()[n:] == 0xCD)
    assert np.all(d_sum.numpy()[8:] == 0xEFEFEFEF)
    # continuing a converged field changes nothing; a buffer that is no field of this engine gives no fault
    s = e.cost_to_go_device(origin, dims, d_goals, 1, d_cost, 0, d_sum, rounds=2, resume=True)
    assert s["pending"] == 0 and ref.same_bytes(d_cost.numpy()[:n].reshape(want.shape), host_cost)
    junk = devmem.DeviceArray(np.random.default_rng(1).integers(0, 2 ** 32, size=n, dtype=np.uint32))
    s = e.cost_to_go_device(origin, dims, d_goals, 1, junk, 0, d_sum, rounds=3, resume=True)
    assert np.all(junk.numpy().reshape(want.shape)[~trav] == NONE)


# 10
def test_device_form_full_convergence_and_neighbours_in_the_queue(make_engine):
    """rounds = 4096 on the open 20 x 12 x 9 box of test 1, here with a tenth of its voxels OCCUPIED at random (so that
    the ESDF and the regions queued in front of it have something to tell apart), behind an esdf_device and a
    regions_device of another box"""
    import torch
    from ratsdf import devmem
    e = make_engine(VS, TRUNC)
    origin, dims = [-13, 5, -3], [20, 12, 9]
    n = 20 * 12 * 9
    rng = np.random.default_rng(2)
    _craft(e, origin, np.where(rng.random((9, 12, 20)) < 0.1, OC, FR).astype(np.uint8))
    goals = np.array([_at(origin, 7, 5, 3), _at(origin, 19, 11, 8)], dtype=np.int32)
    want_cost, want_next, want_sum = e.cost_to_go(origin, dims, goals, with_next=True)
    assert want_sum["reached"] > n // 2
    other_o, other_d = [-12, 6, -2], [17, 9, 6]
    want_field, want_state = e.esdf(other_o, other_d, with_state=True)
    want_labels, want_table = e.regions(other_o, other_d, 7)
    m = 17 * 9 * 6
    t_goals = torch.from_numpy(goals).cuda()
    t_cost = torch.full((n + 16,), -2, dtype=torch.int32, device="cuda")
    t_next = torch.full((n + 16,), 0x77, dtype=torch.uint8, device="cuda")
    t_sum = torch.full((16,), -3, dtype=torch.int32, device="cuda")
    d_out = devmem.DeviceArray(np.zeros(m, dtype=np.float32))
    d_st = devmem.DeviceArray(np.zeros(m, dtype=np.uint8))
    d_lab = devmem.DeviceArray(np.zeros(m, dtype=np.int32))
    d_reg = devmem.DeviceArray(np.zeros((len(want_table) + 1, 32), dtype=np.uint8))
    d_cnt = devmem.DeviceArray(np.zeros(1, dtype=np.int64))
    from ratsdf._abi import RegionsParams
    box = [(C.c_int32 * 3)(*v) for v in (origin, dims)]
    other = [(C.c_int32 * 3)(*v) for v in (other_o, other_d)]
    e.esdf_device(other_o, other_d, d_out.data_ptr(), d_st.data_ptr())         # no synchronisation in between
    assert e.lib.fn["regions_device"](e._h, *other, C.byref(RegionsParams(0.0, 0.0, 7, 0)), d_lab.data_ptr(),
                                      d_reg.data_ptr(), len(want_table) + 1, d_cnt.data_ptr()) == 0
    assert e.lib.fn["cost_to_go_device"](e._h, *box, C.byref(CostParams(0.0, 0.0, 0, 4096)), t_goals.data_ptr(), 2,
                                         t_cost.data_ptr(), t_next.data_ptr(), t_sum.data_ptr()) == 0
    e.synchronize()
    got = t_sum.cpu().numpy()[:8].view(COST_SUMMARY_DTYPE)[0].copy()
    assert got["pending"] == 0 and got["rounds"] == 4096
    got["rounds"] = want_sum["rounds"]
    assert got.tobytes() == want_sum.tobytes()
    assert ref.same_bytes(t_cost.cpu().numpy()[:n].view(np.uint32).reshape(want_cost.shape), want_cost)
    assert ref.same_bytes(t_next.cpu().numpy()[:n].reshape(want_next.shape), want_next)
    assert np.all(t_cost.cpu().numpy()[n:] == -2) and np.all(t_next.cpu().numpy()[n:] == 0x77)
    assert np.all(t_sum.cpu().numpy()[8:] == -3)
    assert ref.same_bytes(d_out.numpy().reshape(want_field.shape), want_field)
    assert ref.same_bytes(d_st.numpy().reshape(want_state.shape), want_state)
    assert ref.same_bytes(d_lab.numpy().reshape(want_labels.shape), want_labels)
    assert ref.same_bytes(d_reg.numpy()[:len(want_table)].reshape(-1).view(want_table.dtype), want_table)
    # the binding's form, into torch tensors
    s = e.cost_to_go_device(origin, dims, t_goals, 2, t_cost, None, t_sum, rounds=40)
    assert s["pending"] == 0 and s["reached"] == want_sum["reached"]


# 11
def test_the_map_is_only_read(make_engine, make_oracle, churn):
    gpu, cpu = make_engine(VS, TRUNC), make_oracle(VS, TRUNC, threads=8)
    _integrate([gpu, cpu], churn[:6])
    before = _snapshot(gpu)
    origin, dims = [-48, -32, 112], [96, 64, 48]
    state = ref.box_state(gpu, origin, dims)
    z, y, x = np.argwhere(state == FR)[0]
    cost, nxt, summary = gpu.cost_to_go(origin, dims, [_at(origin, int(x), int(y), int(z))], clearance=VS,
                                        with_next=True)
    assert summary["goals"] <= 1
    _same_snapshot(before, _snapshot(gpu))
    _integrate([gpu, cpu], churn[6:10])
    assert_maps_equal(gpu, cpu)


# 12
def test_sticky_error_is_returned(make_engine):
    import ratsdf
    small = make_engine(VS, TRUNC, block_bits=6)   # 64 blocks: the first frame exhausts the pool
    f = synthetic.frame("room", 0, scale=0.25)
    with pytest.raises(ratsdf.RatsdfError) as ei:
        _integrate([small], [f])
        small.synchronize()
    assert ei.value.status == 3
    with pytest.raises(ratsdf.RatsdfError) as ei:
        small.cost_to_go([0, 0, 0], [8, 8, 8], [[1, 1, 1]])
    assert ei.value.status == 3
    d_cost, d_next, d_sum = _device_buffers(512)
    with pytest.raises(ratsdf.RatsdfError) as ei:
        small.cost_to_go_device([0, 0, 0], [8, 8, 8], 0, 0, d_cost, 0, d_sum, rounds=1)
    assert ei.value.status == 3


# 13
def test_refusals(make_engine):
    from ratsdf import devmem
    e = make_engine(VS, TRUNC)
    _craft(e, [0, 0, 0], np.full((4, 4, 4), FR, dtype=np.uint8))
    host, device = e.lib.fn["cost_to_go"], e.lib.fn["cost_to_go_device"]
    vec = lambda v: (C.c_int32 * 3)(*v) if v is not None else None   # noqa: E731
    ok_o, ok_d = [0, 0, 0], [4, 4, 4]
    goals = np.array([[1, 1, 1], [2, 2, 2]], dtype=np.int32)
    cost = np.full(64, 0x5A5A5A5A, dtype=np.uint32)
    nxt = np.full(64, 0x5A, dtype=np.uint8)
    summary = np.full(8, 0x5A5A5A5A, dtype=np.uint32)
    d_goals = devmem.DeviceArray(np.concatenate([goals.reshape(-1), np.zeros(10, dtype=np.int32)]))
    d_cost = devmem.DeviceArray(np.full(64 + 4, 0x6B6B6B6B, dtype=np.uint32))
    d_next = devmem.DeviceArray(np.full(64 + 16, 0x6B, dtype=np.uint8))
    d_sum = devmem.DeviceArray(np.full(8 + 2, 0x6B6B6B6B, dtype=np.uint32))

    def call_host(origin=ok_o, dims=ok_d, params=(0.0, 0.0, 0, 0), g=goals.ctypes.data, ng=2, c=cost.ctypes.data,
                  nx=nxt.ctypes.data, s=summary.ctypes.data):
        return host(e._h, vec(origin), vec(dims), C.byref(CostParams(*params)) if params else None, g or None, ng,
                    c or None, nx or None, s or None)

    def call_device(origin=ok_o, dims=ok_d, params=(0.0, 0.0, 0, 3), g=d_goals.data_ptr(), ng=2, c=d_cost.data_ptr(),
                    nx=d_next.data_ptr(), s=d_sum.data_ptr()):
        return device(e._h, vec(origin), vec(dims), C.byref(CostParams(*params)) if params else None, g or None, ng,
                      c or None, nx or None, s or None)

    refused = 0

    def both(**kw):
        nonlocal refused
        assert call_host(**kw) == 1, kw
        if "params" in kw and kw["params"] is not None:
            kw = dict(kw, params=kw["params"][:3] + (3,))
        assert call_device(**kw) == 1, kw
        refused += 1

    for origin, dims in [([0, 0, 0], [0, 4, 4]), ([0, 0, 0], [4, -1, 4]), ([0, 0, 0], [4, 4, 1025]),
                         ([0, 0, 0], [1024, 1024, 129]), ([-32769, 0, 0], [4, 4, 4]), ([0, 32765, 0], [4, 4, 4]),
                         ([0, 0, 40000], [4, 4, 4]), (None, ok_d), (ok_o, None)]:
        both(origin=origin, dims=dims)
    nan = float("nan")
    for params in (None, (nan, 0.0, 0, 0), (0.0, nan, 0, 0), (0.0, 0.0, 16, 0), (0.0, 0.0, 1 << 31, 0),
                   (0.0, 0.0, 3, 0), (0.0, 0.0, 7, 0)):          # unknown bits; UNKNOWN_OCCUPIED with THROUGH_UNKNOWN
        both(params=params)
    both(ng=-1)
    both(ng=(1 << 20) + 1)
    both(g=0, ng=1)
    both(c=0)
    both(s=0)
    assert call_host(params=(0.0, 0.0, 0, 1)) == 1 and call_host(params=(0.0, 0.0, 0, -1)) == 1     # rounds, host form
    assert call_host(params=(0.0, 0.0, 8, 0)) == 1                                                   # CONTINUE, host form
    for rounds in (0, -1, 4097, 1 << 30):
        assert call_device(params=(0.0, 0.0, 0, rounds)) == 1, rounds
    assert call_device(c=d_cost.data_ptr() + 4) == 1 and call_device(g=d_goals.data_ptr() + 8) == 1  # misaligned
    assert call_device(s=d_sum.data_ptr() + 4) == 1
    e.synchronize()
    assert refused == 21
    assert np.all(cost == 0x5A5A5A5A) and np.all(nxt == 0x5A) and np.all(summary == 0x5A5A5A5A)
    assert np.all(d_cost.numpy() == 0x6B6B6B6B) and np.all(d_next.numpy() == 0x6B) and np.all(d_sum.numpy() == 0x6B6B6B6B)
    # what is allowed
    assert call_host() == 0 and cost[1 + 4 * (1 + 4 * 1)] == 0 and nxt[0] == 26 and summary[0] == 2
    assert call_host(nx=0) == 0 and call_host(g=0, ng=0) == 0
    assert call_device() == 0 and call_device(nx=0) == 0 and call_device(g=0, ng=0) == 0
    assert call_device(params=(0.0, 0.0, 8 | 4, 4096)) == 0 and call_device(nx=d_next.data_ptr() + 1, ng=1) == 0
    e.synchronize()
    assert d_sum.numpy()[:8].view(COST_SUMMARY_DTYPE)[0]["goals"] == 1
    # the limits themselves
    c, s = e.cost_to_go([-32768, 32767 - 3, 0], [1, 4, 1024], [[-32768, 32767, 1023]], through_unknown=True)
    assert s["reached"] == 4096 and c[0, 0, 0] == 10 * (1023 - 3) + 14 * 3
    many = np.tile(np.array([[1, 1, 1]], dtype=np.int32), (1 << 20, 1))
    c, s = e.cost_to_go(ok_o, ok_d, many)
    assert s["goals"] == 1 and s["reached"] == 64
