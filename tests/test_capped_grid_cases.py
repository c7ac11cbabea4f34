"""The cases of tests/capped_grid_cases.py without a GPU: the caps they are sized by are the ones in the sources, every
case crosses its cap, the pruned and the expanded restatements equal the direct ones, and each of the three mistakes a
strided loop can make changes an output that tests/test_gpu_capped_grids.py compares."""
import time

import numpy as np
import pytest

import capped_grid_cases as cg
import exposure_ref as xr
import score_ref

F = np.float32
ROWS = np.arange(cg.N_BLOCKS)


# ---------------------------------------------------------------------------------------------------------------------
def test_the_caps_are_the_ones_in_the_sources():
    caps = cg.caps()
    print(caps)
    assert cg.sweeps_from(caps) == cg.SWEEP
    for file, lines in cg.LAUNCHES.items():
        text = (cg.CSRC / file).read_text()
        for line in lines:
            assert line in text, f"{file} no longer launches with `{line}`"
    # out of scope, and why: a chunk of the map file never makes the pack / unpack grids (2048 workgroups, two records
    # each) stride
    assert (caps["kMapChunk"] + 1) // 2 <= 2048


def test_every_case_crosses_its_cap():
    s = cg.sweeps_from(cg.caps())
    b = s["exposure_batches"]
    want = [(64, b), (64, b + 1), (64, 2 * b + 7269), (64, 2 * b + 7269), (33, b + 1), (3, 16 * b + 5), (1, 64 * b + 1),
            (1, 64 * b + 1)]
    assert [(m, n) for m, n, _ in cg.EXPOSURE_SIZES] == want and 0 < 7269 < b and 7269 % cg.WAVES
    assert [acc for _, _, acc in cg.EXPOSURE_SIZES] == [False, False, False, True, False, False, False, True]
    for (m, n, _), name in zip(cg.EXPOSURE_SIZES, cg.EXPOSURE_NAMES):
        c = cg.exposure_case(name)
        assert c.sweep == b * cg.per_wave(m) and len(c.points) == n and len(c.lamps) == m
        assert [cg.per_wave(k) for k in (1, 2, 3, 4, 32, 33, 64)] == [64, 32, 16, 16, 2, 1, 1]
        print(f"{n} points, {m} lamps: {n / c.sweep:.2f} sweeps")
        # the cap, a tail of one point, a tail of one ragged batch (5 of 16 points), or two sweeps and a ragged rest
        assert n - c.sweep in (0, 1, 5) or (n > 2 * c.sweep and n % c.sweep)
    # the host form of the one-lamp case is the one that uploads in two pieces
    assert 32 * (64 * b) <= cg.caps()["kHostChunk"] < 32 * (64 * b + 1) and s["upload_points"] == 64 * b
    small, large = cg.SET_SIZES["small"], cg.SET_SIZES["large"]
    assert small == s["bounds"] + 1 == s["mesh_cells"] + 1
    assert large == s["label_fill"] + 1 + 4099 == s["mesh_refs"] + 1 + 4099
    assert large // s["bounds"] >= 2 and large % s["bounds"] and large // s["mesh_cells"] >= 2
    assert cg.N_BLOCKS // s["join"] >= 2 and 0 < cg.N_BLOCKS % s["join"]
    for name in cg.SCORE_NAMES:
        c = cg.score_case(name)
        assert c.items == cg.SET_SIZES[name.split("_")[1]]
        if c.triangles is not None:
            assert len(c.vertices) == 3 * c.items > s["bounds"]
    assert len(cg.score_map().pos) == cg.N_BLOCKS == len(set(map(tuple, cg.score_map().pos.tolist())))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cg.EXPOSURE_NAMES)
def test_exposure_cases_hold_what_they_are_for(name):
    c = cg.exposure_case(name)
    n = len(c.points)
    t0 = time.perf_counter()
    dose, mask, table, summary = cg.exposure_expected(name)
    print(f"{name}: restated in {time.perf_counter() - t0:.2f} s; {summary}")
    _, _, vis, _, outside, accepted, unique = cg.expanded_pairs(c.points, c.lamps, c.dose if c.accumulate else None)
    assert unique < 3000
    vox = np.rint(c.points["pos"] / F(cg.XVS)).astype(np.int64)
    for period in (64, 16384):                                       # no period that a batch or a sweep could hide
        if n > period:
            assert not np.array_equal(vox[period:], vox[:-period])
    assert set(np.unique(c.points["prob"]).tolist()) == {0.25, 0.75}
    assert not outside[:c.sweep].any()                               # OUTSIDE points only at or beyond one sweep
    assert summary["points_outside"] == outside.sum() and (outside.sum() > 0) == (n > c.sweep + 1)
    if len(c.lamps) >= 2:
        assert not accepted[0] and accepted[1] and table["accepted"][0] == 0 and not (mask & np.uint64(1)).any()
    assert 0 < summary["points_lit"] < n and table["lit"].sum() < summary["lit_pairs"]
    assert 0 < table["lit_high"].sum() < table["lit"].sum()
    if n > c.sweep:                                                  # the tail is seen in every output
        tail = np.arange(n) >= c.sweep
        assert mask[tail].any() and mask[0] != 0 and mask[n - 1] != 0 and dose[n - 1] != c.dose[n - 1]
    if c.accumulate:
        assert set(np.unique(c.dose).tolist()) == set(cg.PRIORS.tolist())
        dark = mask == 0
        assert dark.any() and np.array_equal(dose[dark], c.dose[dark])
    else:
        assert (c.dose == cg.SENTINEL).all() and np.array_equal(dose == cg.SENTINEL, outside)


@pytest.mark.parametrize("name", cg.EXPOSURE_NAMES)
def test_the_expanded_restatement_equals_the_direct_one_on_a_sample(name):
    c = cg.exposure_case(name)
    rng = np.random.default_rng(5000)
    pick = np.sort(rng.choice(len(c.points), 5000, replace=False))
    pick[-1] = len(c.points) - 1
    sub = c._replace(points=c.points[pick], dose=c.dose[pick])
    got = cg.exposure_outputs(sub)
    want = xr.exposure(cg.room_state(), cg.ROOM_ORIGIN, cg.XVS, sub.points, sub.lamps,
                       dose=sub.dose if c.accumulate else None, **cg.EXPOSURE_PARAMS)
    outside = got[0] == cg.SENTINEL if not c.accumulate else np.zeros(5000, dtype=bool)
    assert outside.sum() == (0 if c.accumulate else want[3]["points_outside"])
    assert cg.same_exposure((np.where(outside, F(0), got[0]),) + got[1:], want)


@pytest.mark.parametrize("mistake", cg.MISTAKES)
@pytest.mark.parametrize("name", cg.EXPOSURE_NAMES)
def test_exposure_mistakes_change_a_compared_output(name, mistake):
    c = cg.exposure_case(name)
    right = cg.exposure_expected(name)
    wrong = cg.exposure_outputs(c, mistake)
    differs = [not xr.same_bytes(a, b) for a, b in zip(wrong[:3], right[:3])] + [wrong[3].tobytes() != right[3].tobytes()]
    print(name, mistake, dict(zip(("dose", "mask", "table", "summary"), differs)))
    if len(c.points) == c.sweep:                                     # the cap itself: one sweep, nothing to get wrong
        assert not any(differs)
        return
    assert any(differs)
    if mistake == "tail twice":                                      # counts always; the dose only under ACCUMULATE
        assert differs[2] and differs[3] and differs[0] == c.accumulate and not differs[1]
    if mistake == "second sweep sees the first's state":
        assert differs[0]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cg.SCORE_NAMES)
def test_score_cases_hold_what_they_are_for(name):
    c = cg.score_case(name)
    large = name.endswith("large")
    m = c.marks
    b, f = cg.SWEEP["bounds"], cg.SWEEP["label_fill"]
    t0 = time.perf_counter()
    idx, d2, pruned = cg.searched(c)
    info, rec, pv = cg.score_outputs(c, ROWS)
    print(f"{name}: restated in {time.perf_counter() - t0:.2f} s; {pruned} of {c.items} items pruned; {info}")
    assert pruned <= 0.999 * c.items                                 # a condition on the case, not a tolerance
    assert score_ref.identities(rec) and int(rec["voxels"]) == 512 * cg.N_BLOCKS == len(pv)
    row_of, q = cg.selected_voxels()
    per_block = np.bincount(row_of, minlength=cg.N_BLOCKS)
    assert per_block.min() == 1 and per_block.max() == 2 and int(rec["selected"]) == len(q)
    # every record is compared: the -1 of the voxels not selected, the -2 of those without a match
    assert (pv["nearest"] == -1).sum() == 512 * cg.N_BLOCKS - len(q) and 0 < (pv["nearest"] == -2).sum() < len(q) // 2
    assert (rec["confusion"] > 0).all() and int(rec["unannotated"]) > 0
    # near items over the whole index range, the winners too
    near = m["near"]
    assert len(near) >= 2500 and len(near) + 100 > c.items - len(m["filler"])
    won = np.unique(idx[idx >= 0])
    assert np.isin(won, np.concatenate([near, m["tie_low"], m["extremes"]])).all()
    if large:
        for lo in (b, f):
            assert (near >= lo).sum() >= 500 and (won >= lo).sum() >= 200
        assert (m["extremes"] >= f).all() and (m["dropped"] >= f).all() and (m["tie_high"] >= f).all()
    else:
        assert m["extremes"].tolist() == [b]
    assert (m["tie_low"] < b).all() and (m["tie_high"] > m["tie_low"].max()).all() and np.isin(m["tie_low"], won).sum() >= 5 and not np.isin(m["tie_high"], won).any()
    lo, hi = cg.item_boxes(c)
    assert np.array_equal(lo[m["tie_low"]], lo[m["tie_high"]]) and np.array_equal(hi[m["tie_low"]], hi[m["tie_high"]])
    assert not np.isin(m["dropped"], won).any() and info["kept"] == c.items - len(m["dropped"])
    if c.triangles is None:
        assert set(c.labels[won].tolist()) == {0, 1, 2}
    else:
        assert info["mixed"] == len(m["mixed"]) - 2 and np.isin(m["mixed"], won).any()
        spans = cg._refs_per_triangle(c, info)
        assert (spans[m["wide"]] > cg.caps()["kMeshLanes"]).all() and np.isin(m["wide"], won).any()
        assert info["refs"] == spans.sum()
        if not large:
            assert won.max() == b and spans[b] > cg.caps()["kMeshLanes"]     # the one-triangle tail: near, wide, hi x
    # each extreme of the box is attained by its tail item alone: without the tail the grid is another one
    finite = np.isfinite(lo).all(axis=1) & np.isfinite(hi).all(axis=1)
    finite[m["dropped"]] = False
    rest = finite.copy()
    rest[m["extremes"]] = False
    axes = ((0, lo, np.less), (0, hi, np.greater), (1, lo, np.less), (1, hi, np.greater), (2, lo, np.less),
            (2, hi, np.greater))
    for k, item in enumerate(m["extremes"]):
        axis, side, beyond = axes[k] if large else axes[1]
        others = side[rest, axis].min() if side is lo else side[rest, axis].max()
        assert beyond(side[item, axis], others) and abs(float(side[item, axis]) - float(others)) > info["cell"]
    # the filler is beyond reach, and the asked cell edge is the one the set reports
    assert info["cell"] == float(F(8) * F(cg.SVS)) and cg.SCORE_PARAMS["max_dist"] <= 64 * info["cell"]
    assert cg.beyond_reach(lo[m["filler"]], hi[m["filler"]], q, cg.SCORE_PARAMS["max_dist"]).all()
    # ... but inside the rings the walk visits (two beyond a block's own cells: score_walk ends once
    # (r * cell)^2 exceeds max_dist^2), so a record filed in the wrong cell meets a voxel
    zc = np.floor((cg.FILLER_Z - float(F(info["origin"][2]))) / info["cell"])
    top = np.floor((float(q[:, 2].max()) - float(F(info["origin"][2]))) / info["cell"])
    assert 1 <= zc - top <= 2 and (2 * info["cell"]) ** 2 > cg.SCORE_PARAMS["max_dist"] ** 2


@pytest.mark.parametrize("name", cg.SCORE_NAMES)
def test_the_pruned_restatement_equals_the_unpruned_one_on_a_thinned_copy(name):
    c = cg.thinned(cg.score_case(name), 2000)
    q = cg.selected_voxels()[1]
    if c.triangles is not None:
        q = q[::2]                                                   # (half the voxels: the unpruned search is the slow one)
    a = cg.nearest(c, q, prune=True)
    b = cg.nearest(c, q, prune=False)
    print(f"{c.name}: {c.items} items, {a[2]} pruned")
    assert 1500 < a[2] < c.items and b[2] == 0
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("mistake", cg.MISTAKES)
@pytest.mark.parametrize("name", cg.SCORE_NAMES)
def test_score_mistakes_change_a_compared_output(name, mistake):
    c = cg.score_case(name)
    right = cg.score_outputs(c, ROWS)
    modelled = {}
    for stage in cg.STAGES:
        wrong = cg.score_outputs(c, ROWS, mistake, stage)
        if wrong is not None:
            modelled[stage] = [wrong[0] != right[0], wrong[1].tobytes() != right[1].tobytes(),
                               wrong[2].tobytes() != right[2].tobytes()]
    print(name, mistake, {k: dict(zip(("info", "score", "records"), v)) for k, v in modelled.items()})
    large, mesh = name.endswith("large"), name.startswith("mesh")
    want = {"bounds", "join"}                                        # the stages whose launches this case makes stride
    if mistake == "tail dropped" and (large or mesh):
        want.add("fill")
    if mistake != cg.MISTAKES[2] and large and mesh:
        want.add("refs")
    assert set(modelled) == want
    for stage, differs in modelled.items():
        assert any(differs), f"{mistake} in {stage} is not told apart by {name}"
        assert differs[0] == (stage in ("bounds", "refs"))           # the set's info from the builders' first passes,
        if stage in ("fill", "join"):                                # the records from what the join finds
            assert differs[1] or differs[2]
