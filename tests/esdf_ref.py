"""numpy / scipy restatement of the ESDF contract of include/ratsdf_esdf.h (test infrastructure).

`box_state(engine, origin, dims, occupied_below)` reads the box's voxel states out of any engine's map through
dump_directory / dump_voxels (the HIP engine's or the CPU oracle's); `esdf(state, vs, unknown_occupied)` turns them into
the field: the integer squared distances come from scipy.ndimage.distance_transform_edt (d2 = rint(d * d), exact while
d2 < 2^24), the rest is the header's fp32 formula.  `brute_d2` is the O(n^2) definition the restatement is checked
against.  Arrays are (dims[2], dims[1], dims[0]): x fastest, as the engine writes them."""
import numpy as np
from scipy import ndimage

UNKNOWN, FREE, OCCUPIED = 0, 1, 2
F = np.float32


def box_state(engine, origin, dims, occupied_below=0.0):
    ox, oy, oz = (int(v) for v in origin)
    X, Y, Z = (int(v) for v in dims)
    state = np.zeros((Z, Y, X), dtype=np.uint8)
    _, blocks = engine.dump_directory()
    blocks = blocks[(blocks["idx"] >= 0) & (blocks["idx"] < (1 << engine.block_bits))]  # pending entries: absent
    pos = np.stack([blocks["x"], blocks["y"], blocks["z"]], axis=1).astype(np.int64)
    lo = np.array([ox, oy, oz]) // 8
    hi = np.array([ox + X - 1, oy + Y - 1, oz + Z - 1]) // 8
    sel = np.all((pos >= lo) & (pos <= hi), axis=1)
    blocks, pos = blocks[sel], pos[sel]
    if len(blocks) == 0:
        return state
    t, c, _ = engine.dump_voxels(blocks["idx"])
    t = t.reshape(-1, 8, 8, 8)                       # [block][z][y][x]: voxel x + 8y + 64z
    w = c["weight"].reshape(-1, 8, 8, 8)
    s = np.where(w == 0, UNKNOWN, np.where(t <= F(occupied_below), OCCUPIED, FREE)).astype(np.uint8)
    for i in range(len(blocks)):
        g0 = pos[i] * 8 - np.array([ox, oy, oz])     # box coordinates of the block's voxel (0, 0, 0)
        a = np.maximum(g0, 0)
        b = np.minimum(g0 + 8, [X, Y, Z])
        state[a[2]:b[2], a[1]:b[1], a[0]:b[0]] = s[i, a[2] - g0[2]:b[2] - g0[2], a[1] - g0[1]:b[1] - g0[1],
                                                   a[0] - g0[0]:b[0] - g0[0]]
    return state


def obstacles(state, unknown_occupied=False):
    o = state == OCCUPIED
    return o | (state == UNKNOWN) if unknown_occupied else o


def edt_d2(targets):
    """squared distance (int64) of every voxel to the nearest True voxel of `targets`; None when there is none"""
    if not targets.any():
        return None
    d = ndimage.distance_transform_edt(~targets)
    return np.rint(d * d).astype(np.int64)


def brute_d2(targets):
    """the same by its definition, O(n^2): for small boxes"""
    if not targets.any():
        return None
    Z, Y, X = targets.shape
    grid = np.stack(np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij"), -1).reshape(-1, 3)
    t = grid[targets.reshape(-1)]
    d = ((grid[:, None, :] - t[None, :, :]) ** 2).sum(-1).min(1)
    return d.reshape(targets.shape).astype(np.int64)


def field(o, vs, d2_fn=edt_d2):
    """the contract's fp32 field from the obstacle mask o"""
    vs = F(vs)
    out = np.empty(o.shape, dtype=np.float32)
    d_o, d_c = d2_fn(o), d2_fn(~o)
    out[~o] = F(np.inf) if d_o is None else np.sqrt(d_o[~o].astype(np.float32)) * vs
    out[o] = F(-np.inf) if d_c is None else -(np.sqrt(d_c[o].astype(np.float32)) * vs)
    return out


def esdf(state, vs, unknown_occupied=False, d2_fn=edt_d2):
    return field(obstacles(state, unknown_occupied), vs, d2_fn)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
