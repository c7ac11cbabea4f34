"""numpy / scipy restatement of the regions contract of include/ratsdf_regions.h (test infrastructure).

`box_state` is esdf_ref's; `box_prob(engine, origin, dims)` reads the probability words of the box the same way, through
dump_directory / dump_voxels (0 where no block is allocated).  `regions(state, prob, origin, states, min_prob)` turns
them into the labels and the table: scipy.ndimage.label with its default structure (6-connected in 3-D), the root of a
component as ndimage.minimum of the linear index, the rest in numpy.  `flood_fill` is the plain breadth-first
definition the restatement is checked against.  Arrays are (dims[2], dims[1], dims[0]): x fastest, as the engine writes
them.  The crafted member masks of the tests (serpentine, comb, ...) live here too, for both test files."""
from collections import deque

import numpy as np
from scipy import ndimage

from esdf_ref import FREE, OCCUPIED, UNKNOWN, box_state, same_bytes  # noqa: F401  (re-exported)

F = np.float32
REGION_DTYPE = np.dtype([("root", "<i4"), ("voxels", "<i4"), ("frontier", "<i4"), ("faces", "<u4"),
                         ("lo", "<i2", (3,)), ("hi", "<i2", (3,)), ("reserved", "<u4")])
assert REGION_DTYPE.itemsize == 32


def box_prob(engine, origin, dims):
    ox, oy, oz = (int(v) for v in origin)
    X, Y, Z = (int(v) for v in dims)
    prob = np.zeros((Z, Y, X), dtype=np.float32)
    _, blocks = engine.dump_directory()
    blocks = blocks[(blocks["idx"] >= 0) & (blocks["idx"] < (1 << engine.block_bits))]  # pending entries: absent
    pos = np.stack([blocks["x"], blocks["y"], blocks["z"]], axis=1).astype(np.int64)
    lo = np.array([ox, oy, oz]) // 8
    hi = np.array([ox + X - 1, oy + Y - 1, oz + Z - 1]) // 8
    sel = np.all((pos >= lo) & (pos <= hi), axis=1)
    blocks, pos = blocks[sel], pos[sel]
    if len(blocks) == 0:
        return prob
    _, _, p = engine.dump_voxels(blocks["idx"])
    p = np.asarray(p, dtype=np.float32).reshape(-1, 8, 8, 8)     # [block][z][y][x]: voxel x + 8y + 64z
    for i in range(len(blocks)):
        g0 = pos[i] * 8 - np.array([ox, oy, oz])
        a = np.maximum(g0, 0)
        b = np.minimum(g0 + 8, [X, Y, Z])
        prob[a[2]:b[2], a[1]:b[1], a[0]:b[0]] = p[i, a[2] - g0[2]:b[2] - g0[2], a[1] - g0[1]:b[1] - g0[1],
                                                  a[0] - g0[0]:b[0] - g0[0]]
    return prob


def members(state, prob, states, min_prob=0.0):
    """member(v) of the header: the mask admits the state, and not p(v) < min_prob with p = 0 for UNKNOWN voxels"""
    p = np.where(state == UNKNOWN, F(0), np.asarray(prob, dtype=np.float32))
    with np.errstate(invalid="ignore"):
        return (((int(states) >> state.astype(np.int64)) & 1) != 0) & ~(p < F(min_prob))


def unknown_neighbour(state):
    """voxels with at least one face neighbour inside the box whose state is UNKNOWN"""
    u = state == UNKNOWN
    nb = np.zeros(state.shape, dtype=bool)
    nb[1:] |= u[:-1]
    nb[:-1] |= u[1:]
    nb[:, 1:] |= u[:, :-1]
    nb[:, :-1] |= u[:, 1:]
    nb[:, :, 1:] |= u[:, :, :-1]
    nb[:, :, :-1] |= u[:, :, 1:]
    return nb


def table_of(labels, state, origin):
    """the table from root labels (-1: non-member): everything but the grouping itself"""
    Z, Y, X = labels.shape
    roots = np.unique(labels[labels >= 0])                        # ascending
    out = np.zeros(len(roots), dtype=REGION_DTYPE)
    if len(roots) == 0:
        return out
    rank = np.searchsorted(roots, labels[labels >= 0])
    z, y, x = (c[labels >= 0] for c in np.indices(labels.shape))
    out["root"] = roots
    out["voxels"] = np.bincount(rank, minlength=len(roots))
    out["frontier"] = np.bincount(rank[unknown_neighbour(state)[labels >= 0]], minlength=len(roots))
    faces = np.zeros(len(roots), dtype=np.uint32)
    for a, (c, n) in enumerate(((x, X), (y, Y), (z, Z))):
        lo = np.asarray(ndimage.minimum(c, rank, index=np.arange(len(roots)))).astype(np.int64)
        hi = np.asarray(ndimage.maximum(c, rank, index=np.arange(len(roots)))).astype(np.int64)
        out["lo"][:, a] = lo + int(origin[a])
        out["hi"][:, a] = hi + int(origin[a])
        faces |= np.isin(np.arange(len(roots)), rank[c == 0]).astype(np.uint32) << np.uint32(2 * a)
        faces |= np.isin(np.arange(len(roots)), rank[c == n - 1]).astype(np.uint32) << np.uint32(2 * a + 1)
    out["faces"] = faces
    return out


def regions_of(member, state, origin):
    """(labels, table) of a member mask"""
    lab, k = ndimage.label(member)                                # default structure: face adjacency
    index = np.arange(member.size, dtype=np.int64).reshape(member.shape)
    labels = np.full(member.shape, -1, dtype=np.int32)
    if k:
        roots = np.asarray(ndimage.minimum(index, lab, index=np.arange(1, k + 1))).astype(np.int64)
        assert len(np.unique(roots)) == k                         # one distinct root per component
        labels[member] = roots[lab[member] - 1]
    return labels, table_of(labels, state, origin)


def regions(state, prob, origin, states, min_prob=0.0):
    return regions_of(members(state, prob, states, min_prob), state, origin)


def flood_fill(member):
    """labels by the definition: breadth-first over face neighbours inside the box, voxels visited in index order, so a
    region is found from its smallest index"""
    Z, Y, X = member.shape
    labels = np.full(member.shape, -1, dtype=np.int32)
    flat_m, flat_l = member.reshape(-1), labels.reshape(-1)
    for i in range(member.size):
        if not flat_m[i] or flat_l[i] >= 0:
            continue
        flat_l[i] = i
        todo = deque([i])
        while todo:
            j = todo.popleft()
            x, y, z = j % X, j // X % Y, j // (X * Y)
            for ok, k in ((x > 0, j - 1), (x + 1 < X, j + 1), (y > 0, j - X), (y + 1 < Y, j + X),
                          (z > 0, j - X * Y), (z + 1 < Z, j + X * Y)):
                if ok and flat_m[k] and flat_l[k] < 0:
                    flat_l[k] = i
                    todo.append(k)
    return labels


# ---- crafted member masks, (Z, Y, X) ----
def random_mask(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def checkerboard(shape):
    z, y, x = np.indices(shape)
    return (x + y + z) % 2 == 0


def serpentine(shape, mirrored=False):
    """a one-voxel-wide path through the box: every other row (in y) of every other plane (in z) is full, a row is
    joined to the next at alternating ends in x, a plane to the next at alternating ends of the path, through one
    voxel of the row or plane in between.  One region whose only connection runs the whole length.  Mirrored in all
    three axes the path's far end becomes the first voxel."""
    Z, Y, X = shape
    plane = np.zeros((Y, X), dtype=bool)
    rows = list(range(0, Y, 2))
    for k, y in enumerate(rows):
        plane[y, :] = True
        if k + 1 < len(rows):
            plane[y + 1, X - 1 if k % 2 == 0 else 0] = True
    far = (rows[-1], X - 1 if (len(rows) - 1) % 2 == 0 else 0)    # where the path ends in a plane; it starts at (0, 0)
    m = np.zeros(shape, dtype=bool)
    for z in range(0, Z, 2):
        m[z] = plane
        if z + 1 < Z:
            m[(z + 1,) + (far if (z // 2) % 2 == 0 else (0, 0))] = True
    return m[::-1, ::-1, ::-1].copy() if mirrored else m


def comb(shape, y0, y1, z=0):
    """two teeth along x in rows y0 and y1 of plane z, joined only at the far end (x = X - 1)"""
    Z, Y, X = shape
    m = np.zeros(shape, dtype=bool)
    m[z, y0, :] = True
    m[z, y1, :] = True
    m[z, min(y0, y1):max(y0, y1) + 1, X - 1] = True
    return m
