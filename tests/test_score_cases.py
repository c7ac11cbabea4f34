"""The crafted label-score cases (tests/score_cases.py) without a GPU: the restatement is self-consistent on every
case, the grid search with its conservative bound gives what brute force gives, and every wrong variant the issue
names differs from the contract on the case that targets it."""
import numpy as np
import pytest

import score_cases as sc
import score_ref

VARIANTS = ("select_le", "ties_highest", "fma", "first_hit", "truncate", "cutoff_ge", "bin_round")


def test_the_case_list_is_complete_and_every_variant_has_a_case():
    assert tuple(c.name for c in sc.cases()) == sc.NAMES
    targeted = {w for c in sc.cases() for w in c.wrong}
    assert targeted == set(VARIANTS)


@pytest.mark.parametrize("name", sc.NAMES)
def test_restatement_is_self_consistent(name):
    c = sc.case(name)
    rec, pv = sc.expected(c, np.arange(len(c.blocks)))
    assert score_ref.identities(rec)
    assert int(rec["voxels"]) == 512 * len(c.blocks) == len(pv)
    assert int(rec["selected"]) == int((pv["nearest"] != -1).sum())
    assert int(rec["unmatched"]) == int((pv["nearest"] == -2).sum())
    matched = pv["nearest"] >= 0
    assert np.isnan(pv["dist2"][~matched]).all() and not np.isnan(pv["dist2"][matched]).any()
    assert (pv["dist2"].view(np.uint32)[~matched] == score_ref.QNAN_BITS).all()
    keep = score_ref.kept_points(c.points)
    assert np.isin(pv["nearest"][matched], keep).all()          # a dropped point is never nearest
    md2 = np.float32(c.params["max_dist"]) * np.float32(c.params["max_dist"])
    assert (pv["dist2"][matched] <= md2).all()


def test_cases_reach_what_they_are_for():
    """the properties a case is named after hold in the restatement's result"""
    rec, pv = sc.expected(sc.case("max_dist_edge"), np.arange(1))
    assert int(rec["selected"]) == 512 and int(rec["unmatched"]) == 511
    assert pv["nearest"][0] == 0 and pv["dist2"][0] == np.float32(0.0625) and pv["nearest"][7] == -2
    rec, pv = sc.expected(sc.case("ties"), np.arange(4))
    assert pv["nearest"][0] == 1 and pv["dist2"][0] == np.float32(1 / 128) ** 2     # three-way tie: lowest index
    for name in ("far", "huge"):
        c = sc.case(name)
        rec, pv = sc.expected(c, np.arange(len(c.blocks)))
        assert int(rec["confusion"].sum()) > 0 and (name == "huge" or int(rec["unmatched"]) > 0)
        assert not np.isin(pv["nearest"], np.arange(len(c.points) - 2, len(c.points))).any()
    rec, pv = sc.expected(sc.case("far"), np.arange(3))
    assert (pv["nearest"][512:] < 0).all() and (pv["nearest"][512:] == -2).any()   # the far blocks: nothing matched
    # the winner of "wide_ring" is first met in the second pass over its ring's rows of cells (256 rows per pass)
    c = sc.case("wide_ring")
    rec, pv = sc.expected(c, np.arange(1))
    matched = pv["nearest"] >= 0
    assert 0 < matched.sum() < 512 and int(rec["selected"]) == 512 and int(rec["unmatched"]) == 512 - matched.sum()
    assert set(pv["nearest"][matched]) == {2} and np.flatnonzero(matched).min() >= 7 * 64      # the top plane alone
    info = sc.expected_info(c.points, c.cell, c.vs)
    assert info["cell"] == c.vs and min(info["cells"]) == 25
    ring, row = sc.ring_row(info, c.blocks.pos[0], c.vs, c.points[2])
    assert ring == 5 and 256 <= row < 18 * 18
    for name in ("points_0", "none_finite"):
        c = sc.case(name)
        rec, _ = sc.expected(c, np.arange(len(c.blocks)))
        assert int(rec["selected"]) == int(rec["unmatched"]) > 0
    rec, _ = sc.expected(sc.case("score"), np.arange(1))
    assert (rec["confusion"] > 0).all() and int(rec["unannotated"]) > 0 and (rec["hist"] > 0).sum() > 100
    assert sc.expected_info(sc.case("doubled_cell").points, 0, sc.VS)["cell"] == float(np.float32(0.64))
    assert sc.expected_info(sc.case("one_cell").points, 0, sc.VS)["cells"] == (1, 1, 1)
    for k in (2049, 4097):
        assert sc.expected_info(sc.case(f"crowded_{k}").points, 0, sc.VS)["cells"] == (1, 1, 1)


@pytest.mark.parametrize("name", [c.name for c in sc.cases() if c.grid_cell])
def test_grid_search_with_the_conservative_bound_equals_brute_force(name):
    c = sc.case(name)
    _, right = sc.variant(c, "first_hit")
    assert sc.same(right, sc.expected(c, np.arange(len(c.blocks))))


@pytest.mark.parametrize("name,wrong", [(c.name, w) for c in sc.cases() for w in c.wrong])
def test_wrong_variant_differs_on_its_case(name, wrong):
    c = sc.case(name)
    bad, good = sc.variant(c, wrong)
    assert sc.same(good, sc.expected(c, np.arange(len(c.blocks))))
    assert not sc.same(bad, good), f"{wrong} is not told apart by {name}"
