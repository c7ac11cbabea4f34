"""numpy restatement of the exposure contract of include/ratsdf_surface.h (test infrastructure).

`exposure(state, origin, vs, points, lamps, ...)` turns the box's states (esdf_ref.box_state: any engine's map, the HIP
engine's or the CPU oracle's) into dose, mask, lamp table and summary.  The walk is vectorised over the pairs: one array
step per walk step, no Python loop over pairs.  All float arithmetic is np.float32, one rounded operation per ufunc
call: numpy contracts nothing.

`wrong` names a deliberate deviation from the contract (tests/test_exposure_ref.py shows each one caught):
  "ties_highest"  a tie between two axes goes to the highest one
  "bresenham"     a 26-connected Bresenham line in place of the 6-connected walk
  "descending"    the dose summed over the lamps in descending order
  "contracted"    the two dot products with fused multiply-adds
  "facing_ge"     facing iff c >= 0
  "truncate"      (int)x in place of floorf(x + 0.5f)
Arrays are (dims[2], dims[1], dims[0]): x fastest, as the engine writes them."""
import numpy as np

from esdf_ref import FREE, OCCUPIED, UNKNOWN, box_state, same_bytes  # noqa: F401  (re-exported for the tests)

F = np.float32
UNKNOWN_OCCUPIED, ACCUMULATE = 1, 2
MAX_LAMPS = 64
RGBW_DTYPE = np.dtype([("r", "u1"), ("g", "u1"), ("b", "u1"), ("weight", "u1")])
POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("prob", "<f4"), ("rgbw", RGBW_DTYPE)])
LAMP_DTYPE = np.dtype([("pos", "<f4", (3,)), ("power", "<f4")])
LAMP_RECORD_DTYPE = np.dtype([("accepted", "<i4"), ("lit", "<i4"), ("lit_high", "<i4"), ("reserved", "<i4")])
SUMMARY_DTYPE = np.dtype([("lit_pairs", "<i8"), ("points_lit", "<i4"), ("points_outside", "<i4"),
                          ("lamps_accepted", "<i4"), ("reserved", "<u4", (3,))])
INV_4PI = F(0.07957747)


def blocking_of(state, unknown_occupied=False):
    b = state == OCCUPIED
    return b | (state == UNKNOWN) if unknown_occupied else b


def voxel_of(f, origin, dims, wrong=None):
    """f: float32 [n, 3], the values `x + 0.5f` of the contract.  Returns (voxel [n, 3] int64, box-relative, 0 where
    out of range; in range [n] bool)"""
    origin = np.asarray(origin, dtype=np.int64)
    dims = np.asarray(dims, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        ok = np.all((f >= origin.astype(F)) & (f < (origin + dims).astype(F)), axis=1)
    safe = np.where(ok[:, None], f, F(0))
    if wrong == "truncate":
        v = np.trunc(safe - F(0.5)).astype(np.int64)
        ok = ok & np.all((v >= origin) & (v < origin + dims), axis=1)
        v = np.where(ok[:, None], v, origin)
    else:
        v = np.floor(safe).astype(np.int64)
    return np.where(ok[:, None], v - origin, 0), ok


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def _dot3(a, b, wrong):
    """a[0]*b[0] + a[1]*b[1] + a[2]*b[2], left to right"""
    if wrong == "contracted":
        return _fma(a[..., 2], b[..., 2], _fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _choose(k, n, ties_highest=False):
    """the axis each walk steps on next: [m] (k, n: int64 [m, 3], every row with an axis left)"""
    t = 2 * k + 1
    avail = k < n
    rows = np.arange(len(k))
    order = (2, 1, 0) if ties_highest else (0, 1, 2)
    best = np.where(avail[:, order[0]], order[0], np.where(avail[:, order[1]], order[1], order[2]))
    for b in order[1:]:
        later = b < best if ties_highest else b > best
        smaller = t[:, b] * n[rows, best] < t[rows, best] * n[:, b]
        best = np.where(avail[:, b] & later & smaller, b, best)
    return best


def walk(s, L, ties_highest=False):
    """the voxels of ONE walk from s to L, in order (for hand-written cases)"""
    s, L = np.asarray(s, dtype=np.int64), np.asarray(L, dtype=np.int64)
    pos, n, k, sg = s.copy(), np.abs(L - s), np.zeros(3, dtype=np.int64), np.sign(L - s)
    out = [tuple(int(v) for v in pos)]
    while np.any(k < n):
        a = int(_choose(k[None], n[None], ties_highest)[0])
        pos[a] += sg[a]
        k[a] += 1
        out.append(tuple(int(v) for v in pos))
    return out


def bresenham(s, L):
    """the 26-connected line of the "bresenham" deviation: the longest axis drives, the others follow by error terms"""
    s, L = np.asarray(s, dtype=np.int64), np.asarray(L, dtype=np.int64)
    n, sg = np.abs(L - s), np.sign(L - s)
    drive = int(np.argmax(n))
    pos, err = s.copy(), 2 * n - n[drive]
    out = [tuple(int(v) for v in pos)]
    for _ in range(int(n[drive])):
        for a in range(3):
            if a != drive and err[a] > 0:
                pos[a] += sg[a]
                err[a] -= 2 * n[drive]
            if a != drive:
                err[a] += 2 * n[a]
        pos[drive] += sg[drive]
        out.append(tuple(int(v) for v in pos))
    return out


def clear_walks(blocking, s, L, wrong=None):
    """clear [m] bool: no voxel of the walk s[j] -> L[j] is blocking (s, L: int64 [m, 3], box-relative, in the box)"""
    m = len(s)
    if wrong == "bresenham":
        return np.array([not any(blocking[z, y, x] for x, y, z in bresenham(s[j], L[j])) for j in range(m)], dtype=bool)
    pos, n, k, sg = s.copy(), np.abs(L - s), np.zeros((m, 3), dtype=np.int64), np.sign(L - s)
    clear = np.ones(m, dtype=bool)
    alive = np.arange(m)                      # the walks still under way
    while len(alive):
        hit = blocking[pos[alive, 2], pos[alive, 1], pos[alive, 0]]
        clear[alive[hit]] = False
        alive = alive[~hit & np.any(k[alive] < n[alive], axis=1)]
        if not len(alive):
            break
        a = _choose(k[alive], n[alive], wrong == "ties_highest")
        pos[alive, a] += sg[alive, a]
        k[alive, a] += 1
    return clear


def exposure(state, origin, vs, points, lamps, max_range=np.inf, min_irradiance=0.0, p_cutoff=0.5,
             unknown_occupied=False, dose=None, wrong=None):
    """(dose, mask, table, summary) of the contract.  `dose`: the prior dose of ACCUMULATE, None without the flag --
    then the entries of OUTSIDE points are 0 here (the engine leaves them as they were)."""
    vs = F(vs)
    Z, Y, X = state.shape
    dims = (X, Y, Z)
    pts = np.asarray(points).reshape(-1)
    lmp = np.asarray(lamps).reshape(-1)
    npts, nl = len(pts), len(lmp)
    assert nl <= MAX_LAMPS
    blocking = blocking_of(state, unknown_occupied)
    ppos, nrm, prob = pts["pos"].astype(F).reshape(-1, 3), pts["normal"].astype(F).reshape(-1, 3), pts["prob"].astype(F)
    lpos, power = lmp["pos"].astype(F).reshape(-1, 3), lmp["power"].astype(F)
    with np.errstate(all="ignore"):
        Lv, l_in = voxel_of(lpos / vs + F(0.5), origin, dims, wrong)
        accepted = l_in & ~blocking[Lv[:, 2], Lv[:, 1], Lv[:, 0]]
        sv, p_in = voxel_of((ppos / vs + nrm) + F(0.5), origin, dims, wrong)
        outside = ~p_in
        d = lpos[None, :, :] - ppos[:, None, :]                       # [points, lamps, 3]
        r2 = _dot3(d, d, wrong if wrong == "contracted" else None)
        c = _dot3(np.broadcast_to(nrm[:, None, :], d.shape), d, wrong)
        facing = c >= F(0) if wrong == "facing_ge" else c > F(0)
        mr = F(max_range)
        in_range = ~(r2 > mr * mr)
        e = power[None, :] * (c / (r2 * np.sqrt(r2))) * INV_4PI
    cand = facing & in_range & accepted[None, :] & ~outside[:, None]
    pi, ki = np.nonzero(cand)
    visible = np.zeros((npts, nl), dtype=bool)
    if len(pi):
        visible[pi, ki] = clear_walks(blocking, sv[pi], Lv[ki], wrong)
    acc = np.zeros(npts, dtype=F) if dose is None else np.array(dose, dtype=F).reshape(-1).copy()
    with np.errstate(all="ignore"):
        for k in (range(nl - 1, -1, -1) if wrong == "descending" else range(nl)):
            acc = np.where(visible[:, k], acc + e[:, k], acc)
        lit = visible & (e >= F(min_irradiance))
    mask = np.zeros(npts, dtype=np.uint64)
    for k in range(nl):
        mask |= visible[:, k].astype(np.uint64) << np.uint64(k)
    table = np.zeros(nl, dtype=LAMP_RECORD_DTYPE)
    table["accepted"] = accepted
    table["lit"] = lit.sum(axis=0)
    table["lit_high"] = (lit & (prob >= F(p_cutoff))[:, None]).sum(axis=0)
    summary = np.zeros((), dtype=SUMMARY_DTYPE)
    summary["lit_pairs"] = visible.sum()
    summary["points_lit"] = np.count_nonzero(mask)
    summary["points_outside"] = outside.sum()
    summary["lamps_accepted"] = accepted.sum()
    return acc, mask, table, summary


def exposure_pairs(state, origin, vs, points, lamps, max_range=np.inf, min_irradiance=0.0, unknown_occupied=False,
                   dose=None):
    """the contract per (point, lamp) pair, for callers that weight rows by a multiplicity (tests/capped_grid_cases.py
    evaluates the unique rows of a long list): (dose [n], mask [n], visible [n, lamps] bool, lit [n, lamps] bool,
    outside [n] bool, accepted [lamps] bool).  exposure()'s table and summary are sums over these: lit and
    lit & (prob >= p_cutoff) per lamp, visible over all pairs, the rows with a mask, the outside rows, the accepted
    lamps.  `dose` as in exposure()."""
    vs = F(vs)
    Z, Y, X = state.shape
    dims = (X, Y, Z)
    pts = np.asarray(points).reshape(-1)
    lmp = np.asarray(lamps).reshape(-1)
    npts, nl = len(pts), len(lmp)
    assert nl <= MAX_LAMPS
    blocking = blocking_of(state, unknown_occupied)
    ppos, nrm = pts["pos"].astype(F).reshape(-1, 3), pts["normal"].astype(F).reshape(-1, 3)
    lpos, power = lmp["pos"].astype(F).reshape(-1, 3), lmp["power"].astype(F)
    with np.errstate(all="ignore"):
        Lv, l_in = voxel_of(lpos / vs + F(0.5), origin, dims)
        accepted = l_in & ~blocking[Lv[:, 2], Lv[:, 1], Lv[:, 0]]
        sv, p_in = voxel_of((ppos / vs + nrm) + F(0.5), origin, dims)
        outside = ~p_in
        d = lpos[None, :, :] - ppos[:, None, :]
        r2 = _dot3(d, d, None)
        c = _dot3(np.broadcast_to(nrm[:, None, :], d.shape), d, None)
        mr = F(max_range)
        e = power[None, :] * (c / (r2 * np.sqrt(r2))) * INV_4PI
    cand = (c > F(0)) & ~(r2 > mr * mr) & accepted[None, :] & ~outside[:, None]
    pi, ki = np.nonzero(cand)
    visible = np.zeros((npts, nl), dtype=bool)
    if len(pi):
        visible[pi, ki] = clear_walks(blocking, sv[pi], Lv[ki])
    acc = np.zeros(npts, dtype=F) if dose is None else np.array(dose, dtype=F).reshape(-1).copy()
    mask = np.zeros(npts, dtype=np.uint64)
    with np.errstate(all="ignore"):
        for k in range(nl):
            acc = np.where(visible[:, k], acc + e[:, k], acc)
            mask |= visible[:, k].astype(np.uint64) << np.uint64(k)
        lit = visible & (e >= F(min_irradiance))
    return acc, mask, visible, lit, outside, accepted


def make_points(pos, normal, prob=0.5):
    pos = np.asarray(pos, dtype=F).reshape(-1, 3)
    p = np.zeros(len(pos), dtype=POINT_DTYPE)
    p["pos"] = pos
    p["normal"] = np.broadcast_to(np.asarray(normal, dtype=F), pos.shape)
    p["prob"] = prob
    return p


def make_lamps(pos, power=1.0):
    pos = np.asarray(pos, dtype=F).reshape(-1, 3)
    l = np.zeros(len(pos), dtype=LAMP_DTYPE)
    l["pos"] = pos
    l["power"] = power
    return l
