"""Cases that make the capped launches of the three newest read-outs stride: the exposure of surface points to lamps
(include/ratsdf_surface.h), the label score against points (include/ratsdf_score.h) and against a mesh
(include/ratsdf_score_mesh.h).  Almost every kernel launches one workgroup or one lane per item; these few cap their
grid and let a workgroup loop over several items, and a mistake in such a loop stays hidden until an input is larger
than the cap.  Same role as fuse_cases.py: no GPU and no torch at import; what is expected comes from exposure_ref,
score_ref and score_mesh_ref, never from an engine; the mistakes the cases exist for (MISTAKES) stand beside them.
tests/test_capped_grid_cases.py reads the caps out of the sources, shows that every case crosses its cap and that every
mistake changes an output the GPU test compares; tests/test_gpu_capped_grids.py runs the cases on the engine.

The sizes below are literals, not functions of the caps: a retuned cap breaks the CPU test instead of quietly leaving
the GPU test on the near side of the line.

    launch                                 items of one sweep                       sizes here
    k_exposure_walk                        kExposureMaxWG * 4 waves = 16 384        EXPOSURE_SIZES: the cap, cap + 1,
                                           batches of 64 >> ceil(log2(lamps))       2 sweeps + 7 269 (64 lamps); cap + 1
                                           points                                   at 33, 3 and 1 lamps
    exposure_upload                        kHostChunk / 32 = 1 048 576 points       1 048 577 points (1 lamp)
    k_label_bounds, k_mesh_bounds          kBoundsGrid * 256 = 262 144              262 145; 1 052 676 (4 sweeps + 4 100)
    k_label_count, k_label_scatter         kLabelFillGrid * 256 = 1 048 576         1 052 676 (1 sweep + 4 100)
    k_mesh_refs                            kMeshRefsGrid * 256 = 1 048 576          1 052 676
    k_mesh_cells                           kMeshCellsGrid * 256 / kMeshLanes        262 145; 1 052 676
                                           = 262 144 triangles
    k_score_labels, k_score_mesh           kScoreGrid = 2 048 blocks                4 100 blocks (2 sweeps + 4)

Exposure.  The 16 x 8 x 8 room of test_gpu_exposure.test_packing_edges (floor, pillar, a bar across), floor voxels drawn
at random with probabilities 0.25 / 0.75, points beyond a face (OUTSIDE) only at indices at or beyond one sweep, a
sentinel (or, with ACCUMULATE, a prior dose from four values) in the caller's dose array.  The first lamp sits in the
floor and is not accepted -- except where there is one lamp only, which would light nothing.  The restatement is
evaluated on the unique (point, prior) rows and expanded through np.unique's inverse index.

Scores.  One map of 4 100 blocks with one or two selected voxels each, and sets of 262 145 and 1 052 676 items: a few
thousand near ones (within max_dist of a selected voxel) spread over the whole index range, a lattice of filler above
the map (beyond reach, but inside the rings the walk visits, so a record filed in the wrong place shows), ties between
a low and a high index, non-finite and degenerate items and the six extremes of the bounding box in the tail.  Brute
force leaves out an item only if, in float64, the distance from its box to the box of the selected voxels exceeds
1.01 * max_dist (the margin covers fp32 rounding of the subtraction; a triangle's closest point is clamped to the
triangle's box, so the bound holds for triangles too).

Restatement times, measured on one CPU core (printed again by both test files): the exposure cases 0.03 to 0.2 s up
to 262 149 points and 0.6 s at 1 048 577 (np.unique over the rows is most of it); points_small 0.8 s, points_large
1.1 s, mesh_small 4.4 s, mesh_large 5.2 s (the nearest search of 5 467 voxels against the 2 600 triangles left after
pruning, plus 1 s for the set's info over a million triangles).  A case is searched once; any gather order of the
blocks is a re-tally of that result (tally()).
"""
import functools
import re
from pathlib import Path
from typing import NamedTuple

import numpy as np

import exposure_ref as xr
import query_cases as qc
import score_cases as sc
import score_mesh_cases as smc
import score_mesh_ref as mr
import score_ref
from ratsdf._abi import LAMP_DTYPE, SURFACE_DTYPE

F = np.float32
D = np.float64
CSRC = Path(__file__).resolve().parent.parent / "ra-slam_amd" / "csrc"

MISTAKES = ("tail dropped", "tail twice", "second sweep sees the first's state")

# ---------------------------------------------------------------------------------------------------------------------
# the caps, read from the sources
CONSTANTS = {"kExposureMaxWG": "kernels_exposure.h", "kHostChunk": "ratsdf_engine.hip", "kScoreGrid": "score.inc",
             "kBoundsGrid": "score.inc", "kLabelFillGrid": "score.inc", "kMeshRefsGrid": "score.inc",
             "kMeshCellsGrid": "score.inc", "kMeshLanes": "kernels_score_mesh.h", "kMapChunk": "mapfile.inc"}
# where each named cap is used: a launch that stops using its name no longer has the cap this module believes in
LAUNCHES = {"exposure.inc": ("std::min<uint32_t>((n_batches + 3u) / 4u, kExposureMaxWG)",),
            "kernels_exposure.h": ("batch = blockIdx.x * 4u + (uint32_t)wave; batch < n_batches; batch += gridDim.x * 4u",),
            "score.inc": ("std::min<size_t>((n + 255) / 256, kBoundsGrid)", "std::min<size_t>((n + 255) / 256, kLabelFillGrid)",
                          "dim3(kScoreGrid), dim3(kScoreWG)"),
            "score_mesh.inc": ("std::min<size_t>((std::max(nv, nt) + 255) / 256, kBoundsGrid)",
                               "std::min<size_t>((nt + 255) / 256, kMeshRefsGrid)",
                               "std::min<size_t>((nt * kMeshLanes + 255) / 256, kMeshCellsGrid)")}
WG = 256          # threads of a workgroup of every kernel here
WAVES = 4         # waves of a workgroup of k_exposure_walk: each takes a batch


def source_constant(name):
    """the value of `constexpr <type> name = <integer expression>;` in the file CONSTANTS names"""
    text = (CSRC / CONSTANTS[name]).read_text()
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % re.escape(name), text)
    assert m, f"{name} is not a named constant of {CONSTANTS[name]}"
    expr = re.sub(r"\(\s*[a-z_0-9]+\s*\)", "", m.group(1))          # casts
    expr = re.sub(r"(?<=\d)[uUlL]+", "", expr)                      # suffixes
    assert re.fullmatch(r"[\d\s<*+()]+", expr), (name, m.group(1))
    return int(eval(expr))


@functools.lru_cache(maxsize=None)
def caps():
    return {name: source_constant(name) for name in CONSTANTS}


def sweeps_from(c):
    """the items one sweep of each capped launch takes, from the constants `c` (caps())"""
    return {"exposure_batches": c["kExposureMaxWG"] * WAVES, "upload_points": c["kHostChunk"] // 32,
            "bounds": c["kBoundsGrid"] * WG, "label_fill": c["kLabelFillGrid"] * WG, "mesh_refs": c["kMeshRefsGrid"] * WG,
            "mesh_cells": c["kMeshCellsGrid"] * WG // c["kMeshLanes"], "join": c["kScoreGrid"]}


# the same as literals: what the cases are sized by (the CPU test shows them equal to sweeps_from(caps()))
SWEEP = {"exposure_batches": 16384, "upload_points": 1048576, "bounds": 262144, "label_fill": 1048576,
         "mesh_refs": 1048576, "mesh_cells": 262144, "join": 2048}


def per_wave(n_lamps):
    """points of a batch: 64 >> ceil(log2(n_lamps))"""
    log_m = 0
    while (1 << log_m) < n_lamps:
        log_m += 1
    return 64 >> log_m


# ---------------------------------------------------------------------------------------------------------------------
# exposure
XVS, XTRUNC = 0.01, 0.06
ROOM_ORIGIN, ROOM_DIMS = [0, 0, 0], [16, 8, 8]
SENTINEL = F(-7.0)
PRIORS = np.array([0.0, 0.5, 3.25, 1000.0], dtype=F)
EXPOSURE_PARAMS = dict(min_irradiance=20.0, p_cutoff=0.5)
# (lamps, points, ACCUMULATE)
EXPOSURE_SIZES = ((64, 16384, False), (64, 16385, False), (64, 2 * 16384 + 7269, False), (64, 2 * 16384 + 7269, True),
                  (33, 16385, False), (3, 16 * 16384 + 5, False), (1, 64 * 16384 + 1, False), (1, 64 * 16384 + 1, True))
EXPOSURE_NAMES = tuple(f"{m}_lamps_{n}_points" + ("_accumulate" if acc else "") for m, n, acc in EXPOSURE_SIZES)


def room_state():
    """(Z, Y, X) states of the room: an OCCUPIED floor, a pillar at (5, 3) up to z = 4, a bar along y at x = 11, z = 3"""
    state = np.full((8, 8, 16), xr.FREE, dtype=np.uint8)
    state[0] = xr.OCCUPIED
    state[1:5, 3, 5] = xr.OCCUPIED
    state[3, :, 11] = xr.OCCUPIED
    return state


class ExposureCase(NamedTuple):
    name: str
    points: np.ndarray       # SURFACE_DTYPE [n]
    lamps: np.ndarray        # LAMP_DTYPE [m]
    dose: np.ndarray         # float32 [n]: what the caller's dose array holds (the sentinel, or the prior dose)
    accumulate: bool
    sweep: int               # points of one sweep of k_exposure_walk at this number of lamps


@functools.lru_cache(maxsize=None)
def exposure_case(name):
    n_lamps, n, accumulate = EXPOSURE_SIZES[EXPOSURE_NAMES.index(name)]
    rng = np.random.default_rng(1000 * n_lamps + n % 1000)
    sweep = SWEEP["exposure_batches"] * per_wave(n_lamps)
    at = np.stack([rng.integers(0, 16, n_lamps), rng.integers(0, 8, n_lamps), rng.integers(1, 8, n_lamps)], 1)
    if n_lamps >= 2:
        at[0] = (0, 0, 0)                                            # the first lamp sits in the floor: not accepted
        at[1] = (1, 1, 5)
    else:
        at[0] = (1, 1, 5)
    lamps = np.zeros(n_lamps, dtype=LAMP_DTYPE)
    lamps["pos"] = at.astype(F) * F(XVS)
    lamps["power"] = rng.uniform(0.5, 2.0, n_lamps).astype(F)
    vox = np.stack([rng.integers(0, 16, n), rng.integers(0, 8, n), np.zeros(n, dtype=np.int64)], 1).astype(F)
    vox[0] = (1, 1, 0)                                               # right under the lamp at (1, 1, 5), and so is
    vox[n - 1] = (2, 1, 0)                                           # the last point: the whole tail where it is one
    points = np.zeros(n, dtype=SURFACE_DTYPE)
    points["normal"] = (0, 0, 1)
    points["prob"] = rng.choice(np.array([0.25, 0.75], dtype=F), n)
    tail = np.arange(sweep, n - 1)                                   # (the last point stays inside)
    out = tail[rng.random(len(tail)) < 0.02]
    if len(tail) >= 3:
        out = np.union1d(out, tail[[0, len(tail) // 2, len(tail) - 1]])
    kinds = np.array([(-3, 2, 0), (17, 5, 0), (4, -2, 0), (4, 9, 0), (7, 3, 8), (7, 3, -2)], dtype=F)
    vox[out] = kinds[rng.integers(0, len(kinds), len(out))]
    points["pos"] = vox * F(XVS)
    dose = rng.choice(PRIORS, n) if accumulate else np.full(n, SENTINEL, dtype=F)
    for a in (points, lamps, dose):
        a.setflags(write=False)
    return ExposureCase(name, points, lamps, dose, accumulate, sweep)


def expanded_pairs(points, lamps, dose, state=None):
    """exposure_ref.exposure_pairs of the unique (point, dose) rows, expanded through np.unique's inverse index:
    (dose [n], mask [n], visible [n, lamps], lit [n, lamps], outside [n], accepted [lamps], unique rows)"""
    n = len(points)
    rows = np.zeros((n, 36), dtype=np.uint8)
    rows[:, :32] = np.ascontiguousarray(points).view(np.uint8).reshape(n, 32)
    if dose is not None:
        rows[:, 32:] = np.ascontiguousarray(dose, dtype=F).view(np.uint8).reshape(n, 4)
    _, first, inv = np.unique(rows.view("V36").reshape(n), return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    acc, mask, vis, lit, outside, accepted = xr.exposure_pairs(
        room_state() if state is None else state, ROOM_ORIGIN, XVS, points[first], lamps,
        min_irradiance=EXPOSURE_PARAMS["min_irradiance"], dose=None if dose is None else np.asarray(dose)[first])
    return acc[inv], mask[inv], vis[inv], lit[inv], outside[inv], accepted, len(first)


def exposure_outputs(c, mistake=None):
    """(dose, mask, table, summary) of case `c` as the caller's arrays hold them afterwards -- the entries of OUTSIDE
    points keep what the dose array held.  `mistake` (one of MISTAKES): what a wrong stride would leave --
      tail dropped   the points at or beyond one sweep are never walked: dose and mask untouched (the mask 0), not counted
      tail twice     ... walked a second time: counted twice, and with ACCUMULATE summed on top of their own result
      second sweep   a point at or beyond one sweep starts its sum from the result of the point one sweep before it"""
    n = len(c.points)
    acc, mask, vis, lit, outside, accepted, _ = expanded_pairs(c.points, c.lamps, c.dose if c.accumulate else None)
    dose = np.where(outside, c.dose, acc)
    tail = np.arange(n) >= c.sweep
    w = np.ones(n, dtype=np.int64)
    if mistake == "tail dropped":
        w[tail] = 0
        dose, mask = np.where(tail, c.dose, dose), np.where(tail, np.uint64(0), mask)
    elif mistake == "tail twice":
        w[tail] = 2
        if c.accumulate:
            again = expanded_pairs(c.points[tail], c.lamps, dose[tail])[0]
            dose[tail] = np.where(outside[tail], dose[tail], again)
    elif mistake == "second sweep sees the first's state":
        i = np.flatnonzero(tail & ~outside)
        before = np.where(outside[i - c.sweep], F(0), dose[i - c.sweep])
        start = before + c.dose[i] if c.accumulate else before
        dose[i] = expanded_pairs(c.points[i], c.lamps, start)[0]
    elif mistake is not None:
        raise KeyError(mistake)
    high = c.points["prob"] >= F(EXPOSURE_PARAMS["p_cutoff"])
    table = np.zeros(len(c.lamps), dtype=xr.LAMP_RECORD_DTYPE)
    table["accepted"] = accepted
    table["lit"] = (lit * w[:, None]).sum(axis=0)
    table["lit_high"] = ((lit & high[:, None]) * w[:, None]).sum(axis=0)
    summary = np.zeros((), dtype=xr.SUMMARY_DTYPE)
    summary["lit_pairs"] = (vis.sum(axis=1) * w).sum()
    summary["points_lit"] = w[vis.any(axis=1)].sum()
    summary["points_outside"] = w[outside].sum()
    summary["lamps_accepted"] = accepted.sum()
    return dose.astype(F), mask, table, summary


@functools.lru_cache(maxsize=None)
def exposure_expected(name):
    out = exposure_outputs(exposure_case(name))
    for a in out:
        a.setflags(write=False)
    return out


def same_exposure(a, b):
    return all(xr.same_bytes(x, y) for x, y in zip(a[:3], b[:3])) and a[3].tobytes() == b[3].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the map of both scores
N_BLOCKS = 4100
SVS = qc.VS
SCORE_ENGINE = dict(block_bits=13, bucket_bits=15)
SCORE_PARAMS = dict(tsdf_below=0.1, max_dist=0.3, p_cutoff=0.5, min_weight=0)
SET_SIZES = {"small": 262145, "large": 1048577 + 4099}
SCORE_NAMES = ("points_small", "points_large", "mesh_small", "mesh_large")
REACH = 0.28              # near items lie within this of the selected voxel they were made for
FILLER_Z = 0.5            # the lattice's first plane: 0.36 above the highest voxel, two cells above the map's


@functools.lru_cache(maxsize=None)
def score_map():
    """4 100 blocks in one layer, 64 to a row, around the origin; 0.05 (selected below 0.1) in one voxel of each and in
    a second one of every third, 0.5 elsewhere; weight 1; query_cases' probabilities"""
    i = np.arange(N_BLOCKS)
    pos = np.stack([i % 64 - 32, i // 64 - 32, np.zeros(N_BLOCKS, dtype=np.int64)], axis=1)
    t = np.full((N_BLOCKS, 512), F(0.5), dtype=F)
    t[i, (37 * i + 11) % 512] = F(0.05)
    third = i[i % 3 == 0]
    t[third, (101 * third + 7) % 512] = F(0.05)
    blocks = sc.craft(pos, tsdf=t, weight=1)
    for a in blocks:
        a.setflags(write=False)
    return blocks


@functools.lru_cache(maxsize=None)
def selected_voxels():
    """(block row [k], position [k, 3] float32) of the map's selected voxels, by block row, then voxel slot"""
    b = score_map()
    row, slot = np.nonzero(np.abs(b.tsdf) < F(SCORE_PARAMS["tsdf_below"]))
    return row, score_ref.voxel_positions(b.pos, SVS)[row, slot]


class SetCase(NamedTuple):
    name: str
    vertices: np.ndarray     # [v, 3] float32: the points of a point set, the vertices of a mesh
    labels: np.ndarray       # [v] uint8
    triangles: np.ndarray    # [t, 3] int32, or None for a point set
    marks: dict              # item indices by role: near, filler, tie_low, tie_high, dropped, extremes
    vs: float = SVS
    cell: float = 0.0

    @property
    def items(self):
        return len(self.vertices) if self.triangles is None else len(self.triangles)


def _unit(rng, k):
    u = rng.normal(size=(k, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _layout(rng, n, size, n_near):
    """which item index plays which role.  The tail (at or beyond the last sweep boundary the set crosses) holds the
    bounding box's extremes, the dropped items and the high halves of the ties; the near items are spread over the
    whole range, at least 600 of them at or beyond each sweep boundary that leaves room"""
    b, f = SWEEP["bounds"], SWEEP["label_fill"]
    free = np.ones(n, dtype=bool)

    def take(lo, hi, k):
        cand = np.flatnonzero(free[lo:hi]) + lo
        pick = np.sort(rng.choice(cand, k, replace=False))
        free[pick] = False
        return pick

    m = {}
    if size == "large":
        m["extremes"] = np.arange(n - 6, n)                          # lo x, hi x, lo y, hi y, lo z, hi z
        free[m["extremes"]] = False
        m["dropped"] = take(f, n, 8)
        m["tie_high"] = take(f, n, 40)
        m["tie_low"] = take(0, b, 40)
        near = [take(f, n, 600), take(b, f, 600), take(0, n, n_near - 1200)]
    else:
        m["extremes"] = np.array([n - 1])                            # hi x
        free[m["extremes"]] = False
        m["dropped"] = take(0, b, 8)
        m["tie_high"] = take(b - 50000, b, 40)
        m["tie_low"] = take(0, 50000, 40)
        near = [take(0, b, n_near)]
    m["near"] = np.sort(np.concatenate(near))
    m["filler"] = np.flatnonzero(free)
    return m


def _near_positions(rng, k):
    """k float64 positions within REACH of selected voxels drawn at random"""
    _, q = selected_voxels()
    target = q[rng.integers(0, len(q), k)].astype(D)
    return target + _unit(rng, k) * rng.uniform(0.01, REACH, size=(k, 1))


def _lattice(k):
    """k float64 positions on a lattice above the map: 11 m wide in x and y, planes 0.2 m apart from FILLER_Z up"""
    w = 1024 if k > (1 << 19) else 512
    j = np.arange(k)
    step = 10.5 / (w - 1)
    return np.stack([-5.4 + (j % w) * step, -5.4 + ((j // w) % w) * step, FILLER_Z + (j // (w * w)) * 0.2], axis=1)


EXTREMES = np.array([(-6.5, 0.3, 0.05), (6.7, 0.3, 0.05), (0.3, -6.6, 0.05), (0.3, 6.9, 0.05), (0.3, 0.3, -1.2),
                     (0.3, 0.3, 2.9)])


def _hi_x_voxel():
    _, q = selected_voxels()
    return q[np.argmax(q[:, 0])].astype(D)


@functools.lru_cache(maxsize=None)
def points_case(size):
    n = SET_SIZES[size]
    rng = np.random.default_rng(262145 if size == "small" else 1052676)
    m = _layout(rng, n, size, 4000 if size == "small" else 5000)
    p = np.zeros((n, 3), dtype=D)
    p[m["near"]] = _near_positions(rng, len(m["near"]))
    p[m["filler"]] = _lattice(len(m["filler"]))
    p[m["tie_low"]] = _near_positions(rng, 40)
    p[m["tie_high"]] = p[m["tie_low"]]                               # equal coordinates: equal d2, the low index wins
    p[m["extremes"]] = EXTREMES if size == "large" else EXTREMES[1:2]
    p[m["dropped"]] = _near_positions(rng, 8)
    p = p.astype(F)
    for k, i in enumerate(m["dropped"]):
        p[i, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    labels = rng.integers(0, 3, size=n).astype(np.uint8)
    labels[m["tie_high"]] = (labels[m["tie_low"]] + 1) % 3
    p.setflags(write=False)
    labels.setflags(write=False)
    return SetCase(f"points_{size}", p, labels, None, m)


@functools.lru_cache(maxsize=None)
def mesh_case(size):
    """one triangle per item over three vertices of its own (V = 3 T).  Near and filler items are score_mesh_cases'
    small_tris; 60 near ones are stretched over several cells (more than the kMeshLanes lanes that share a triangle's
    cells); a tenth of the near ones carry three different labels.  The small mesh's last triangle -- its whole tail --
    is near AND the box's hi x: one corner 4 mm from the selected voxel of highest x, the others out at x = 6.7."""
    n = SET_SIZES[size]
    rng = np.random.default_rng(3 * n)
    m = _layout(rng, n, size, 2500)
    anchor = np.zeros((n, 3), dtype=D)
    anchor[m["near"]] = _near_positions(rng, len(m["near"]))
    anchor[m["filler"]] = _lattice(len(m["filler"]))
    anchor[m["tie_low"]] = _near_positions(rng, 40)
    anchor[m["tie_high"]] = anchor[m["tie_low"]]
    anchor[m["extremes"]] = EXTREMES if size == "large" else _hi_x_voxel() + (0.004, 0, 0)
    anchor[m["dropped"]] = _near_positions(rng, 8)
    o1, o2 = np.tile([0.01, 0, 0], (n, 1)), np.tile([0, 0.01, 0], (n, 1))
    o1[m["near"]], o2[m["near"]] = rng.uniform(-0.01, 0.01, (2, len(m["near"]), 3))
    wide = m["near"][:: max(1, len(m["near"]) // 60)][:60]           # spread over the index range like the near ones
    o1[wide] = rng.uniform(0.3, 0.5, (len(wide), 3)) * np.sign(rng.normal(size=(len(wide), 3)))
    m["wide"] = wide
    if size == "small":
        last = m["extremes"][0]
        o1[last], o2[last] = (6.7, 0, 0) - anchor[last], (6.7, 0.01, 0) - anchor[last]
    v = np.stack([anchor, anchor + o1, anchor + o2], axis=1).astype(F)            # [n, 3, 3]
    for k, i in enumerate(m["dropped"]):
        if k % 2:
            v[i, k % 3, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]                  # a non-finite coordinate
        else:
            v[i, 2] = v[i, k % 2]                                                  # two equal vertices
    labels = np.repeat(rng.integers(0, 3, size=n).astype(np.uint8), 3)
    labels.reshape(n, 3)[m["tie_high"]] = ((labels.reshape(n, 3)[m["tie_low"], 0] + 1) % 3)[:, None]
    mixed = np.concatenate([m["near"][::10], m["dropped"][:2]])
    labels.reshape(n, 3)[mixed] = (labels.reshape(n, 3)[mixed, :1] + np.arange(3)) % 3
    m["mixed"] = mixed
    v = v.reshape(-1, 3)
    tri = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    for a in (v, labels, tri):
        a.setflags(write=False)
    return SetCase(f"mesh_{size}", v, labels, tri, m)


def score_case(name):
    kind, size = name.split("_")
    return points_case(size) if kind == "points" else mesh_case(size)


def thinned(c, filler=3000):
    """a copy of the case with its filler cut to `filler` items (evenly taken); the other items keep their order"""
    keep = np.ones(c.items, dtype=bool)
    keep[c.marks["filler"]] = False
    keep[c.marks["filler"][:: max(1, len(c.marks["filler"]) // filler)]] = True
    if c.triangles is None:
        return SetCase(c.name + "_thinned", c.vertices[keep], c.labels[keep], None, {})
    n = int(keep.sum())
    return SetCase(c.name + "_thinned", c.vertices.reshape(-1, 3, 3)[keep].reshape(-1, 3),
                   c.labels.reshape(-1, 3)[keep].reshape(-1), np.arange(3 * n, dtype=np.int32).reshape(n, 3), {})


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, pruned
def item_boxes(c, items=None):
    """(lo, hi) [k, 3] float64: the axis-aligned boxes of the case's items (a point's is the point)"""
    if c.triangles is None:
        p = c.vertices if items is None else c.vertices[items]
        return p.astype(D), p.astype(D)
    t = c.triangles if items is None else c.triangles[items]
    corners = c.vertices[t]
    return corners.min(axis=1).astype(D), corners.max(axis=1).astype(D)


def beyond_reach(lo, hi, q, max_dist):
    """[k] bool: in float64 the distance from the box lo .. hi to the box of the positions q exceeds 1.01 * max_dist
    (False for a box with a NaN: such an item is not pruned, the restatement drops it itself)"""
    qlo, qhi = q.min(axis=0).astype(D), q.max(axis=0).astype(D)
    with np.errstate(invalid="ignore"):
        gap = np.maximum(np.maximum(qlo - hi, lo - qhi), 0.0)
        return np.sqrt((gap * gap).sum(axis=1)) > 1.01 * float(max_dist)


def nearest(c, q, items=None, prune=True):
    """(item index or -2, d2) for the float32 positions q, by the restatement's brute force over the items `items`
    (ascending indices; default all) that are not beyond reach of q's box; returns also how many were pruned"""
    md = SCORE_PARAMS["max_dist"]
    items = np.arange(c.items) if items is None else np.asarray(items)
    lo, hi = item_boxes(c, items)
    far = beyond_reach(lo, hi, q, md) if prune else np.zeros(len(items), dtype=bool)
    sub = items[~far]
    if c.triangles is None:
        idx, d2 = score_ref.nearest(q, c.vertices[sub], md)
    else:
        idx, d2 = mr.nearest(q, c.vertices, c.triangles[sub], md)
    return np.where(idx >= 0, sub[np.maximum(idx, 0)] if len(sub) else idx, idx), d2, int(far.sum())


_NEAREST = {}


def searched(c, prune=True):
    """nearest() of every selected voxel of the map, by block row and slot; computed once per case, never changed"""
    key = (c.name, prune)
    if key not in _NEAREST:
        idx, d2, pruned = nearest(c, selected_voxels()[1], prune=prune)
        idx.setflags(write=False)
        d2.setflags(write=False)
        _NEAREST[key] = (idx, d2, pruned)
    return _NEAREST[key]


def tally(c, rows, idx, d2):
    """(score record, per-voxel records) of the map's blocks gathered in the order `rows`, given the nearest item of
    every selected voxel (by block row and slot, as searched() returns them)"""
    b = score_map()
    rows = np.asarray(rows)
    row_of = selected_voxels()[0]
    first = np.searchsorted(row_of, rows)                            # each block's selected voxels are adjacent
    count = np.searchsorted(row_of, rows, side="right") - first
    take = np.repeat(first, count) + (np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count))
    args = (b.pos[rows], b.tsdf[rows], b.rgbw["weight"][rows], b.prob[rows], SVS, c.vertices, c.labels)
    if c.triangles is None:
        return score_ref.score(*args, **SCORE_PARAMS, nearest_fn=lambda q, p, md: (idx[take], d2[take]))
    return mr.score(*args, c.triangles, **SCORE_PARAMS, nearest_fn=lambda q, md: (idx[take], d2[take]))


_INFO = {}


def expected_info(c, part=None):
    """the set's info by the header's rules (score_cases.expected_info, score_mesh_cases.expected_info); part:
    ("head", k) / ("tail", k) for the set of the first k items / of the items from k on.  Computed once, copied out"""
    key = (c.name, part)
    if key not in _INFO:
        s = c if part is None else head(c, part[1]) if part[0] == "head" else tail_only(c, part[1])
        _INFO[key] = sc.expected_info(s.vertices, s.cell, s.vs) if s.triangles is None else smc.expected_info(s)
    return dict(_INFO[key])


def head(c, k):
    """the case's first k items as a case of its own"""
    if c.triangles is None:
        return c._replace(vertices=c.vertices[:k], labels=c.labels[:k])
    return c._replace(triangles=c.triangles[:k])


def tail_only(c, k):
    if c.triangles is None:
        return c._replace(vertices=c.vertices[k:], labels=c.labels[k:])
    return c._replace(triangles=c.triangles[k:])


STAGES = ("bounds", "refs", "fill", "join")


def stage_sweep(c, stage):
    """the items (blocks for the join) of one sweep of the stage's launches for this kind of set; None if it has none"""
    mesh = c.triangles is not None
    return {"bounds": SWEEP["bounds"], "refs": SWEEP["mesh_refs"] if mesh else None,
            "fill": SWEEP["mesh_cells"] if mesh else SWEEP["label_fill"], "join": SWEEP["join"]}[stage]


def score_outputs(c, rows, mistake=None, stage=None):
    """(info, score record, per-voxel records) of the set `c` against the map gathered in the order `rows`, as the GPU
    test compares them.  With `mistake` (MISTAKES) in `stage` (STAGES): what a wrong stride there would leave --
      bounds  k_label_bounds / k_mesh_bounds.  dropped: kept, mixed and the box from the first sweep's items; twice:
              the tail's kept and mixed counted again; second sweep: the cell ranges of the first sweep only
      refs    k_mesh_refs.  dropped / twice: the tail's references left out / counted again
      fill    count and scatter (k_mesh_cells).  dropped: the tail's items are in no cell -- nothing finds them
      join    k_score_labels / k_score_mesh over the gathered blocks.  dropped: the blocks from 2 048 on are not
              visited (their records keep the buffer's -9 words, their voxels are not counted); twice: counted again;
              second sweep: block b + 2 048 answers with the nearest item of block b's first selected voxel
    Returns None where the mistake has no model in that stage."""
    idx, d2, _ = searched(c)
    info = expected_info(c)
    if mistake is None:
        return (info,) + tally(c, rows, idx, d2)
    sweep = stage_sweep(c, stage)
    dropped, twice = mistake == "tail dropped", mistake == "tail twice"
    if stage in ("bounds", "refs"):
        if sweep is None or c.items <= sweep:
            return None
        first, rest = expected_info(c, ("head", sweep)), expected_info(c, ("tail", sweep))
        wrong = dict(info)
        counts = ("kept", "mixed") if c.triangles is not None else ("kept",)
        if stage == "refs":
            if not (dropped or twice):
                return None
            assert first["cell"] == info["cell"] == rest["cell"]
            per = _refs_per_triangle(c, info)
            wrong["refs"] = int(per[:sweep].sum()) + (2 * int(per[sweep:].sum()) if twice else 0)
        elif dropped:
            wrong.update({k: first[k] for k in counts + ("origin", "cells", "cell") + (("refs",) if "refs" in info else ())})
        elif twice:
            wrong.update({k: info[k] + rest[k] for k in counts})
        else:
            wrong.update(origin=first["origin"], cells=first["cells"])
        return (wrong,) + tally(c, rows, idx, d2)
    if stage == "fill":
        if not dropped or c.items <= sweep:
            return None
        idx2, d22 = idx.copy(), d2.copy()
        lost = np.flatnonzero(idx >= sweep)
        idx2[lost], d22[lost], _ = nearest(c, selected_voxels()[1][lost], items=np.arange(sweep))
        return (info,) + tally(c, rows, idx2, d22)
    assert stage == "join"
    rows = np.asarray(rows)
    if len(rows) <= sweep:
        return None
    rec, pv = tally(c, rows, idx, d2)
    if dropped or twice:
        part = tally(c, rows[sweep:], idx, d2)[0]
        for field in ("selected", "unmatched", "unannotated", "confusion", "hist"):
            rec[field] = rec[field] + part[field] * (1 if twice else -1)
        if dropped:
            pv = pv.copy()
            pv[512 * sweep:].view(np.int32)[...] = -9
        return info, rec, pv
    row_of = selected_voxels()[0]
    stale_idx, stale_d2 = idx.copy(), d2.copy()
    for k in range(sweep, len(rows)):
        mine = np.flatnonzero(row_of == rows[k])
        theirs = np.searchsorted(row_of, rows[k - sweep])
        stale_idx[mine], stale_d2[mine] = idx[theirs], d2[theirs]
    return (info,) + tally(c, rows, stale_idx, stale_d2)


def _refs_per_triangle(c, info):
    """the cells each triangle's box meets in the grid `info` describes (0 for a dropped triangle)"""
    v, t = mr.as_mesh(c.vertices, c.triangles)
    keep = mr.kept_triangles(v, t)
    corners = v[t[keep]]
    lo = np.array([float(F(x)) for x in info["origin"]])
    e = float(F(info["cell"]))
    spans = np.floor((corners.max(axis=1).astype(D) - lo) / e) - np.floor((corners.min(axis=1).astype(D) - lo) / e) + 1
    per = np.zeros(len(t), dtype=np.int64)
    per[keep] = spans.prod(axis=1).astype(np.int64)
    return per


def same_score(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
