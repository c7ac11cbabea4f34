"""The crafted cases of the label score against a mesh (tests/score_mesh_cases.py) without a GPU: the restatement is
self-consistent on every case, the search over rings of cells filled by box overlap gives what brute force gives,
every wrong variant the issue names differs from the contract on the case that targets it, the cases reach what they
are named after, and the float32 contract picks the winners a float64 evaluation picks."""
import numpy as np
import pytest

import score_cases as sc
import score_mesh_cases as mc
import score_mesh_ref as mr
import score_ref

F = np.float32


def test_the_case_list_is_complete_and_every_variant_has_a_case():
    assert tuple(c.name for c in mc.cases()) == mc.NAMES
    targeted = {w for c in mc.cases() for w in c.wrong}
    assert targeted == set(mc.VARIANTS)


@pytest.mark.parametrize("name", mc.NAMES)
def test_restatement_is_self_consistent(name):
    c = mc.case(name)
    rec, pv = mc.expected(c, np.arange(len(c.blocks)))
    assert mr.identities(rec)
    assert int(rec["voxels"]) == 512 * len(c.blocks) == len(pv)
    assert int(rec["selected"]) == int((pv["nearest"] != -1).sum()) > 0
    assert int(rec["unmatched"]) == int((pv["nearest"] == -2).sum())
    matched = pv["nearest"] >= 0
    assert np.isnan(pv["dist2"][~matched]).all() and not np.isnan(pv["dist2"][matched]).any()
    assert (pv["dist2"].view(np.uint32)[~matched] == mr.QNAN_BITS).all()
    keep = mr.kept_triangles(c.vertices, c.triangles)
    assert np.isin(pv["nearest"][matched], keep).all()          # a dropped triangle is never nearest
    md2 = F(c.params["max_dist"]) * F(c.params["max_dist"])
    assert (pv["dist2"][matched] <= md2).all() and (pv["dist2"][matched] >= 0).all()


@pytest.mark.parametrize("name", mc.NAMES)
def test_grid_search_over_boxes_equals_brute_force(name):
    c = mc.case(name)
    assert mc.same(mc.through_grid(c), mc.expected(c, np.arange(len(c.blocks))))


@pytest.mark.parametrize("name,wrong", [(c.name, w) for c in mc.cases() for w in c.wrong])
def test_wrong_variant_differs_on_its_case(name, wrong):
    c = mc.case(name)
    bad, good = mc.variant(c, wrong)
    assert mc.same(good, mc.expected(c, np.arange(len(c.blocks))))
    assert not mc.same(bad, good), f"{wrong} is not told apart by {name}"


def _regions(p, a, b, c):
    """which of the header's seven cases decides, 1 .. 7, for positions p [m, 3] and one triangle"""
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = ap @ ab, ap @ ac, bp @ ab, bp @ ac, cp @ ab, cp @ ac
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    out = np.full(len(p), 7)
    for k in range(5, -1, -1):
        out[conds[k]] = k + 1
    return out


def test_cases_reach_what_they_are_for():
    """the properties a case is named after hold in the restatement's result"""
    c = mc.case("voronoi")
    rec, pv = mc.expected(c, np.arange(len(c.blocks)))
    q = score_ref.voxel_positions(c.blocks.pos, c.vs).reshape(-1, 3).astype(np.float64)
    a, b, cc = (c.vertices[k].astype(np.float64) for k in range(3))
    reg = _regions(q, a, b, cc)
    assert set(reg) == {1, 2, 3, 4, 5, 6, 7}                    # every region holds voxels
    on_plane = q[:, 2] == 0
    inside = (q[:, 0] >= 0) & (q[:, 1] >= 0) & (q[:, 0] + q[:, 1] <= 0.125)
    assert (pv["dist2"][on_plane & inside] == 0).all() and (on_plane & inside).sum() == 45
    assert (pv["dist2"] == (q[:, 2] ** 2).astype(F))[inside].all()          # exact above the face
    for corner in (a, b, cc):                                               # borders: the voxels at the vertices
        assert ((q == corner).all(axis=1)).sum() == 1
    rec, pv = mc.expected(mc.case("max_dist_edge"), np.arange(1))
    assert int(rec["selected"]) == 512 and int(rec["unmatched"]) == 511
    assert pv["nearest"][0] == 0 and pv["dist2"][0] == F(0.0625) and pv["nearest"][7] == -2
    c = mc.case("ties")
    rec, pv = mc.expected(c, np.arange(4))
    q = score_ref.voxel_positions(c.blocks.pos, c.vs).reshape(-1, 3)
    on_edge_plane = (q[:, 1] == 0) & (q[:, 0] >= 0) & (q[:, 0] <= 0.125)
    assert (pv["nearest"][on_edge_plane] == 1).all() and on_edge_plane.sum() > 8    # four-way ties: the lowest index
    assert set(pv["nearest"]) == {1, 2} and int(rec["unannotated"]) == 0
    c = mc.case("mixed_labels")
    assert mc.expected_info(c)["mixed"] == 1 and mc.expected_info(c)["kept"] == 2
    rec, _ = mc.expected(c, np.arange(len(c.blocks)))
    assert int(rec["unannotated"]) == 0 and int(rec["confusion"][[1, 3]].sum()) == 0      # all HIGH: the first vertex
    for name in ("far", "huge"):
        c = mc.case(name)
        rec, pv = mc.expected(c, np.arange(len(c.blocks)))
        assert int(rec["confusion"].sum()) > 0
        last = len(c.triangles) - 1
        assert not (pv["nearest"] == last - 1).any()
        # (the last triangle of "huge" has one vertex inside the block and two at 1e30: near that vertex it wins)
        assert (pv["nearest"] == last).any() == (name == "huge")
    rec, pv = mc.expected(mc.case("far"), np.arange(3))
    assert (pv["nearest"][512:] < 0).all() and (pv["nearest"][512:] == -2).any()   # the far blocks: nothing matched
    # the winner of "wide_ring" is first met in the second pass over its ring's rows of cells (256 rows per pass)
    c = mc.case("wide_ring")
    rec, pv = mc.expected(c, np.arange(1))
    matched = pv["nearest"] >= 0
    assert 0 < matched.sum() < 512 and int(rec["selected"]) == 512 and int(rec["unmatched"]) == 512 - matched.sum()
    assert set(pv["nearest"][matched]) == {2} and np.flatnonzero(matched).min() >= 7 * 64      # the top plane alone
    info = mc.expected_info(c)
    assert info["cell"] == c.vs and min(info["cells"]) == 25 and info["refs"] == info["kept"] == 3
    corners = c.vertices[c.triangles[2]]
    ring, row = sc.ring_row(info, c.blocks.pos[0], c.vs, corners.min(axis=0), corners.max(axis=0))
    assert ring == 5 and 256 <= row < 18 * 18
    for name in ("tris_0", "all_dropped", "no_vertices"):
        c = mc.case(name)
        rec, _ = mc.expected(c, np.arange(len(c.blocks)))
        assert int(rec["selected"]) == int(rec["unmatched"]) > 0 and mc.expected_info(c)["kept"] == 0
    info = mc.expected_info(mc.case("coincident"))
    assert (info["triangles"], info["kept"]) == (25, 21)
    info = mc.expected_info(mc.case("non_finite"))
    assert 0 < info["kept"] < info["triangles"]
    info = mc.expected_info(mc.case("unused_vertices"))
    assert info["kept"] == 20 and max(abs(v) for v in info["origin"]) < 1 and max(info["cells"]) <= 5
    for name in ("collinear", "slivers", "tiny"):
        c = mc.case(name)
        rec, pv = mc.expected(c, np.arange(len(c.blocks)))
        assert mc.expected_info(c)["kept"] == len(c.triangles) and int(rec["confusion"].sum()) > 100
    _, pv = mc.expected(mc.case("tiny"), np.arange(3))
    assert pv["nearest"][0] == 0 and pv["dist2"][0] == 0
    rec, _ = mc.expected(mc.case("score"), np.arange(1))
    assert (rec["confusion"] > 0).all() and int(rec["unannotated"]) > 0 and (rec["hist"] > 0).sum() > 100
    for k in (300, 600):
        info = mc.expected_info(mc.case(f"crowded_{k}"))
        assert info["cells"] == (1, 1, 1) and info["refs"] == info["kept"] == k > (k // 300) * mc.CHUNK
    # the reference cap: the cell limit alone would stop at 0.64, where the twenty spanning triangles alone hold more
    # references than the cap admits
    c = mc.case("ref_cap")
    info = mc.expected_info(c)
    assert info["cell"] == float(F(1.28)) and info["refs"] <= mc.MAX_REFS
    assert np.prod(np.floor(100.0 / 0.64) + 1) ** 3 <= mc.MAX_CELLS < 20 * (np.floor(100.0 / 0.64)) ** 3
    assert 20 * (np.floor(100.0 / 0.64)) ** 3 > mc.MAX_REFS


def test_collinear_triangles_give_the_exact_segment_distance():
    c = mc.case("collinear")
    v = c.vertices[c.triangles[:3]].astype(np.float64)          # the three axis-parallel ones: [3, 3, 3]
    q = score_ref.voxel_positions(c.blocks.pos, c.vs).reshape(-1, 3)
    for a, b, far in v:
        d2 = mr.tri_dist2(q[:, None, :], *(x.astype(F)[None, None] for x in (a, b, far)))[:, 0]
        lo, hi = min(a[0], far[0]), max(a[0], far[0])
        foot = np.clip(q[:, 0].astype(np.float64), lo, hi)
        want = (foot - q[:, 0]) ** 2 + (a[1] - q[:, 1]) ** 2 + (a[2] - q[:, 2]) ** 2
        assert not np.isnan(d2).any() and np.allclose(d2, want, rtol=1e-5, atol=1e-12)


def test_mesh_and_points_disagree_on_the_wall():
    """the case that shows why the feature exists: the point score on the same vertices labels the wall's voxels by the
    handle"""
    c = mc.case("mesh_against_points")
    rows = np.arange(len(c.blocks))
    b = c.blocks
    mesh, pv = mc.expected(c, rows)
    pts, pp = score_ref.score(b.pos[rows], b.tsdf[rows], b.rgbw["weight"][rows], b.prob[rows], c.vs, c.vertices,
                              c.labels, **c.params)
    assert int(mesh["selected"]) == int(pts["selected"]) == 1024
    assert tuple(mesh["confusion"]) != tuple(pts["confusion"])
    low = lambda r: int(r["confusion"][1] + r["confusion"][3])
    assert low(mesh) > 300 and low(pts) == 0                    # the wall is LOW; by points nothing is
    q = score_ref.voxel_positions(b.pos, c.vs).reshape(-1, 3)
    on_wall = q[:, 2] == 0
    assert (pv["nearest"][on_wall] < 2).all() and (pv["dist2"][on_wall] < 1e-12).all()
    assert (c.labels[pp["nearest"][on_wall & (pp["nearest"] >= 0)]] == mr.HIGH).all()


def test_float32_winners_equal_a_float64_evaluation():
    """a random surface of 2 to 5 cm triangles, a tenth of them slivers: the contract's winners are those of the same
    steps in float64, except where the float64 best and runner-up lie within 1e-6 m of each other (at most 1 % of the
    voxels)"""
    rng = np.random.default_rng(3)
    k = 1500
    a = rng.uniform(0.0, 0.32, size=(k, 3))
    a[:, 2] = 0.08 + 0.04 * np.sin(9 * a[:, 0]) * np.cos(7 * a[:, 1])
    e1, e2 = rng.uniform(-0.05, 0.05, size=(k, 3)), rng.uniform(-0.05, 0.05, size=(k, 3))
    e1[:, 2] *= 0.2
    e2[:, 2] *= 0.2
    thin = np.arange(k) % 10 == 0
    e2[thin] = e1[thin] * rng.uniform(0.2, 0.8, size=(thin.sum(), 1)) + rng.normal(size=(thin.sum(), 3)) * 1e-6
    va, vb, vc = a.astype(F), (a + e1).astype(F), (a + e2).astype(F)
    q = score_ref.voxel_positions(np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)]), 0.02).reshape(-1, 3)
    vertices = np.stack([va, vb, vc], axis=1).reshape(-1, 3)
    triangles = np.arange(3 * k).reshape(-1, 3)
    idx, d2 = mr.nearest(q, vertices, triangles, 0.3)
    assert (idx >= 0).all() and not np.isnan(d2).any()
    exact = np.concatenate([mr.tri_dist2(q[s:s + 256, None, :], va[None], vb[None], vc[None], dtype=np.float64)
                            for s in range(0, len(q), 256)])
    order = np.argsort(exact, axis=1)[:, :2]
    best, second = (np.sqrt(np.take_along_axis(exact, order[:, j:j + 1], axis=1)[:, 0]) for j in (0, 1))
    clear = second - best >= 1e-6
    assert (idx[clear] == order[clear, 0]).all()
    assert (~clear).sum() <= 0.01 * len(q), (~clear).sum()
    print("exempted", int((~clear).sum()), "of", len(q), "largest distance error",
          float(np.abs(np.sqrt(d2.astype(np.float64)) - best).max()))
    assert np.abs(np.sqrt(d2.astype(np.float64)) - best)[clear].max() < 1e-6
