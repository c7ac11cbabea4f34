"""The restatement of the regions contract (tests/regions_ref.py) against the plain breadth-first flood fill, and the
properties the contract states (no GPU needed)."""
import numpy as np
import pytest

import regions_ref as ref

SHAPE = (21, 19, 13)          # (Z, Y, X): a 13 x 19 x 21 box


def _crafted():
    yield "checkerboard", ref.checkerboard((16, 16, 16))
    yield "serpentine", ref.serpentine((9, 24, 40))
    yield "serpentine mirrored", ref.serpentine((9, 24, 40), mirrored=True)
    yield "comb in a tile", ref.comb((3, 9, 30), 1, 3)
    yield "comb across tiles", ref.comb((3, 21, 70), 2, 17)
    diag = np.zeros((6, 12, 40), dtype=bool)
    for k in range(6):
        diag[k, k, k] = diag[k, 11 - k, 30 + k] = True         # corners only
        diag[0, k, 20 + k] = True                              # edges only
    yield "diagonal", diag
    yield "full", np.ones(SHAPE, dtype=bool)
    yield "empty", np.zeros(SHAPE, dtype=bool)
    yield "one voxel", np.ones((1, 1, 1), dtype=bool)


def _state(member):
    return np.where(member, ref.FREE, ref.OCCUPIED).astype(np.uint8)


def _check(member, state=None, origin=(0, 0, 0)):
    state = _state(member) if state is None else state
    labels, table = ref.regions_of(member, state, origin)
    want = ref.flood_fill(member)
    assert ref.same_bytes(labels, want)
    Z, Y, X = member.shape
    roots = np.unique(want[want >= 0])
    assert np.array_equal(table["root"], roots) and np.all(table["reserved"] == 0)
    nb = ref.unknown_neighbour(state)
    for r in table:                                            # the table by its definition, region by region
        zz, yy, xx = np.nonzero(want == r["root"])
        assert r["voxels"] == len(xx) and r["root"] == (xx + X * (yy + Y * zz)).min()
        assert r["frontier"] == int(nb[want == r["root"]].sum())
        lo = [xx.min(), yy.min(), zz.min()]
        hi = [xx.max(), yy.max(), zz.max()]
        assert list(r["lo"]) == [a + o for a, o in zip(lo, origin)] and list(r["hi"]) == [a + o for a, o in zip(hi, origin)]
        faces = sum((lo[a] == 0) << (2 * a) | (hi[a] == n - 1) << (2 * a + 1) for a, n in enumerate((X, Y, Z)))
        assert r["faces"] == faces
    return labels, table


@pytest.mark.parametrize("density", [0.2, 0.31, 0.5, 0.8])
def test_random_masks_equal_the_flood_fill(density):
    member = ref.random_mask(SHAPE, density, seed=int(density * 100))
    state = _state(member)
    state[ref.random_mask(SHAPE, 0.3, seed=7) & ~member] = ref.UNKNOWN
    _check(member, state, origin=(-13, 5, -700))


@pytest.mark.parametrize("name,member", list(_crafted()), ids=[n for n, _ in _crafted()])
def test_crafted_shapes_equal_the_flood_fill(name, member):
    labels, table = _check(member)
    if name == "checkerboard":
        assert len(table) == member.size // 2 and np.all(table["voxels"] == 1)
    if name.startswith("serpentine") or name.startswith("comb") or name in ("full", "one voxel"):
        assert len(table) == 1 and table["voxels"][0] == member.sum()
    if name == "diagonal":
        assert len(table) == member.sum()                      # edge and corner contact joins nothing
    if name == "full":
        assert table["root"][0] == 0 and table["faces"][0] == 0x3F
    if name == "empty":
        assert len(table) == 0 and np.all(labels == -1)


def test_a_small_checkerboard_gives_32_singletons():
    labels, table = ref.regions_of(ref.checkerboard((4, 4, 4)), _state(ref.checkerboard((4, 4, 4))), (0, 0, 0))
    assert len(table) == 32 and np.all(table["voxels"] == 1) and len(np.unique(table["root"])) == 32
    assert np.array_equal(np.sort(labels[labels >= 0]), table["root"])


def test_members_follow_the_header():
    state = np.array([ref.UNKNOWN, ref.FREE, ref.OCCUPIED, ref.FREE, ref.OCCUPIED, ref.UNKNOWN], dtype=np.uint8)
    state = state.reshape(1, 1, 6)
    tiny = np.float32(1e-45)                                   # the smallest positive float
    below = np.nextafter(np.float32(0.5), np.float32(0))
    prob = np.array([0.9, 0.5, below, np.nan, 0.0, np.nan], dtype=np.float32).reshape(1, 1, 6)
    assert ref.members(state, prob, 7, 0.0).all()
    assert ref.members(state, prob, 7, 0.5).reshape(-1).tolist() == [False, True, False, True, False, False]
    assert ref.members(state, prob, 7, tiny).reshape(-1).tolist() == [False, True, True, True, False, False]
    assert ref.members(state, prob, 1, 0.0).reshape(-1).tolist() == [True, False, False, False, False, True]
    assert ref.members(state, prob, 6, 0.0).reshape(-1).tolist() == [False, True, True, True, True, False]


def test_frontier_counts_a_member_once_and_only_inside_the_box():
    state = np.full((3, 3, 3), ref.UNKNOWN, dtype=np.uint8)
    state[1, 1, 1] = ref.FREE                                   # six unknown neighbours
    labels, table = ref.regions(state, np.zeros(state.shape, np.float32), (0, 0, 0), 1 << ref.FREE)
    assert len(table) == 1 and table["frontier"][0] == 1 and table["voxels"][0] == 1
    one = np.full((1, 1, 1), ref.FREE, dtype=np.uint8)          # the same voxel alone in its box: nothing to count
    assert ref.regions(one, np.zeros(one.shape, np.float32), (1, 1, 1), 2)[1]["frontier"][0] == 0
    # an unknown neighbour counts whether or not it is a member itself
    labels, table = ref.regions(state, np.zeros(state.shape, np.float32), (0, 0, 0), 3)
    assert len(table) == 1 and table["voxels"][0] == 27 and table["frontier"][0] == 27
