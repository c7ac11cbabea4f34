"""numpy / scipy restatement of the cost-to-go contract of include/ratsdf_cost.h (test infrastructure).

`box_state` and the ESDF are esdf_ref's.  `traversable` builds the mask of the header, `accept` filters the goals,
`exact` is the cost field (a heap Dijkstra over the moves for small boxes, scipy.sparse.csgraph.dijkstra over the move
graph otherwise: both are here, and a test holds them to each other), `next_of(cost, trav)` the direction bytes from a
cost field, `summary_of` the summary record, `unconverged_ok` the three properties the header promises of a field whose
rounds ran out.  Arrays are (dims[2], dims[1], dims[0]): x fastest, as the engine writes them.  The crafted masks are
regions_ref's (serpentine, comb, random_mask)."""
import heapq

import numpy as np
from scipy import sparse
from scipy.sparse import csgraph

import esdf_ref
from esdf_ref import FREE, OCCUPIED, UNKNOWN, box_state, same_bytes  # noqa: F401  (re-exported)
from regions_ref import comb, random_mask, serpentine  # noqa: F401  (re-exported)

F = np.float32
NONE = 0xFFFFFFFF
AT_GOAL, NO_STEP = 255, 254
WEIGHTS = (0, 10, 14, 17)                 # by the number of axes a move changes
SUMMARY_DTYPE = np.dtype([("goals", "<i4"), ("traversable", "<i4"), ("reached", "<i4"), ("max_cost", "<u4"),
                          ("pending", "<i4"), ("rounds", "<i4"), ("reserved", "<u4", (2,))])
assert SUMMARY_DTYPE.itemsize == 32


def moves(faces_only=False, weights=WEIGHTS):
    """(code, dx, dy, dz, w) of every move, ascending in the direction code (dx + 1) + 3 (dy + 1) + 9 (dz + 1)"""
    out = []
    for code in range(27):
        dx, dy, dz = code % 3 - 1, code // 3 % 3 - 1, code // 9 - 1
        k = (dx != 0) + (dy != 0) + (dz != 0)
        if k == 0 or (faces_only and k != 1):
            continue
        out.append((code, dx, dy, dz, weights[k]))
    return out


def traversable(state, vs, clearance=0.0, unknown_occupied=False, through_unknown=False, field=None):
    """traversable(v) of the header; field: the ESDF to use instead of esdf_ref's (the wrong variants of the tests)"""
    if field is None:
        field = esdf_ref.esdf(state, vs, unknown_occupied)
    o = esdf_ref.obstacles(state, unknown_occupied)
    kind = (state == FREE) | ((state == UNKNOWN) & bool(through_unknown))
    with np.errstate(invalid="ignore"):
        return ~o & kind & ~(field.astype(np.float32) < F(clearance))


def accept(goals, origin, trav):
    """flat box indices of the accepted goals: inside the box, traversable, each once, ascending"""
    Z, Y, X = trav.shape
    g = np.asarray(goals, dtype=np.int64).reshape(-1, 3) - np.asarray(origin, dtype=np.int64)
    inside = np.all((g >= 0) & (g < [X, Y, Z]), axis=1)
    g = g[inside]
    idx = g[:, 0] + X * (g[:, 1] + Y * g[:, 2])
    return np.unique(idx[trav.reshape(-1)[idx]])


def shifted(a, dx, dy, dz, fill):
    """b[z, y, x] = a[z + dz, y + dy, x + dx], `fill` where that leaves the box"""
    Z, Y, X = a.shape
    b = np.full(a.shape, fill, dtype=a.dtype)
    dst = tuple(slice(max(0, -d), n - max(0, d)) for d, n in ((dz, Z), (dy, Y), (dx, X)))
    src = tuple(slice(max(0, d), n - max(0, -d)) for d, n in ((dz, Z), (dy, Y), (dx, X)))
    b[dst] = a[src]
    return b


def dijkstra_heap(trav, goal_idx, faces_only=False, weights=WEIGHTS):
    """the exact cost by the textbook algorithm (pure Python: small boxes)"""
    Z, Y, X = trav.shape
    t = trav.reshape(-1)
    cost = np.full(trav.size, NONE, dtype=np.uint32)
    dist = {}
    heap = [(0, int(i)) for i in goal_idx]
    for _, i in heap:
        dist[i] = 0
    heapq.heapify(heap)
    mv = moves(faces_only, weights)
    while heap:
        d, i = heapq.heappop(heap)
        if d > dist[i]:
            continue
        x, y, z = i % X, i // X % Y, i // (X * Y)
        for _, dx, dy, dz, w in mv:
            ux, uy, uz = x + dx, y + dy, z + dz
            if not (0 <= ux < X and 0 <= uy < Y and 0 <= uz < Z):
                continue
            j = ux + X * (uy + Y * uz)
            if t[j] and d + w < dist.get(j, 1 << 62):
                dist[j] = d + w
                heapq.heappush(heap, (d + w, j))
    for i, d in dist.items():
        cost[i] = d
    return cost.reshape(trav.shape)


def dijkstra_scipy(trav, goal_idx, faces_only=False, weights=WEIGHTS):
    """the exact cost over the sparse move graph (boxes up to 96 x 64 x 48 in about a second)"""
    cost = np.full(trav.size, NONE, dtype=np.uint32)
    if len(goal_idx) == 0:
        return cost.reshape(trav.shape)
    index = np.arange(trav.size, dtype=np.int64).reshape(trav.shape)
    rows, cols, vals = [], [], []
    for code, dx, dy, dz, w in moves(faces_only, weights):
        if code > 13:                                    # each undirected move once
            continue
        both = trav & shifted(trav, dx, dy, dz, False)
        rows.append(index[both])
        cols.append(shifted(index, dx, dy, dz, -1)[both])
        vals.append(np.full(int(both.sum()), float(w)))
    g = sparse.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                          shape=(trav.size, trav.size))
    d = csgraph.dijkstra(g, directed=False, indices=np.asarray(goal_idx), min_only=True)
    ok = np.isfinite(d)
    cost[ok] = np.rint(d[ok]).astype(np.uint32)          # (integers below 2^32: exact in float64)
    return cost.reshape(trav.shape)


def exact(trav, goal_idx, faces_only=False):
    return (dijkstra_heap if trav.size <= 4096 else dijkstra_scipy)(trav, goal_idx, faces_only)


def closed_form(shape, goal, weights=WEIGHTS):
    """the cost in an all-traversable box with one goal (box coordinates x, y, z): 10 (a - b) + 14 (b - c) + 17 c for the
    sorted offsets a >= b >= c"""
    z, y, x = np.indices(shape)
    off = np.sort(np.stack([np.abs(x - goal[0]), np.abs(y - goal[1]), np.abs(z - goal[2])], -1), axis=-1)
    c, b, a = off[..., 0], off[..., 1], off[..., 2]
    return (weights[1] * (a - b) + weights[2] * (b - c) + weights[3] * c).astype(np.uint32)


def best_move(cost, faces_only=False, weights=WEIGHTS, largest_code=False):
    """per voxel: min over moves to neighbours inside the box with a finite cost of cost[u] + w (2^62: no such move),
    and the code that attains it -- the smallest among equals (largest_code: the wrong variant)"""
    c = cost.astype(np.int64)
    best = np.full(cost.shape, 1 << 62, dtype=np.int64)
    code_of = np.full(cost.shape, NO_STEP, dtype=np.uint8)
    for code, dx, dy, dz, w in moves(faces_only, weights):
        u = shifted(c, dx, dy, dz, NONE)
        s = np.where(u == NONE, 1 << 62, u + w)
        better = (s <= best) & (s < (1 << 62)) if largest_code else s < best
        best = np.where(better, s, best)
        code_of = np.where(better, code, code_of).astype(np.uint8)
    return best, code_of


def next_of(cost, trav, faces_only=False, largest_code=False):
    """the direction bytes of a cost field.  (A finite cost sits on a traversable voxel only: trav is the check.)"""
    assert not np.any((cost != NONE) & ~trav)
    _, code = best_move(cost, faces_only, largest_code=largest_code)
    return np.where(cost == NONE, NO_STEP, np.where(cost == 0, AT_GOAL, code)).astype(np.uint8)


def summary_of(cost, trav, pending=0, rounds=0):
    s = np.zeros(1, dtype=SUMMARY_DTYPE)[0]
    finite = cost != NONE
    s["goals"] = int((cost == 0).sum())
    s["traversable"] = int(trav.sum())
    s["reached"] = int(finite.sum())
    s["max_cost"] = int(cost[finite].max()) if finite.any() else 0
    s["pending"] = pending
    s["rounds"] = rounds
    return s


def unconverged_ok(cost, want, trav, goal_idx, faces_only=False):
    """the header's three properties of a field whose rounds ran out; want: the exact cost"""
    flat = cost.reshape(-1)
    at_goal = np.zeros(cost.size, dtype=bool)
    at_goal[goal_idx] = True
    upper = np.all(cost.astype(np.int64) >= want.astype(np.int64))           # NONE is the largest value
    fixed = np.all(flat[at_goal] == 0) and np.all(cost[~trav] == NONE) and not np.any(flat[~at_goal] == 0)
    best, _ = best_move(cost, faces_only)
    inner = (cost != NONE) & ~at_goal.reshape(cost.shape)
    accounted = np.all(best[inner] <= cost[inner].astype(np.int64))
    return bool(upper and fixed and accounted)


def relax_once(trav, goal_idx, faces_only=False):
    """ONE Jacobi round from the seed (goals 0, the rest NONE): what a wrong engine that stops early would give"""
    cost = np.full(trav.size, NONE, dtype=np.uint32)
    cost[goal_idx] = 0
    cost = cost.reshape(trav.shape)
    best, _ = best_move(cost, faces_only)
    return np.where(trav & (best < cost.astype(np.int64)), best, cost).astype(np.uint32)


def path_weight(path):
    """summed weights of a voxel path [k, 3]"""
    steps = np.abs(np.diff(np.asarray(path, dtype=np.int64), axis=0))
    assert steps.max(initial=0) <= 1
    return int(np.take(WEIGHTS, (steps != 0).sum(axis=1)).sum())
