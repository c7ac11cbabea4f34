"""Compile-time resource guard for the cost-to-go kernels (kernels_cost.h; no GPU needed: hipcc cross-compiles).

None may spill.  The values pinned here are the ones the cross-compile gives and DESIGN.md 4 "Cost to go" records: only
the relaxation holds a tile in LDS, 8 424 bytes (8 160 of them the 34 x 10 x 6 cost words of a tile with its halo); the
summary keeps its four waves' partial sums there (64 bytes); nothing else uses LDS.  Every kernel
keeps 8 waves per SIMD but the 26-move relaxation, whose 54 neighbour words per lane leave 5."""
from test_kernel_resources import resource_usage

KERNELS = {"k_cost_seedE": (0, 8, 8), "k_cost_goalsILb1EE": (0, 16, 8), "k_cost_goalsILb0EE": (0, 16, 8),
           "k_cost_relaxILb1EE": (8424, 64, 8), "k_cost_relaxILb0EE": (8424, 96, 5), "k_cost_summaryE": (64, 24, 8),
           "k_cost_nextILb1EE": (0, 16, 8), "k_cost_nextILb0EE": (0, 24, 8)}
# mangled name's tail: (LDS bytes, VGPR ceiling, waves per SIMD)


def test_cost_kernels_exist_do_not_spill_and_keep_their_occupancy():
    usage = resource_usage()
    assert len([n for n in usage if "k_cost_" in n]) == len(KERNELS), sorted(n for n in usage if "k_cost_" in n)
    for name, (lds, vgprs, waves) in KERNELS.items():
        base = name[:name.index("I")] if "I" in name else name[:-1]
        found = [v for n, v in usage.items() if f"{len(base)}{name}" in n]
        assert len(found) == 1, (name, sorted(usage))
        res = found[0]
        assert res["ScratchSize"] == 0, f"{name}: {res}"
        assert res["Occupancy"] == waves, f"{name}: {res}"
        assert res["LDS"] == lds, f"{name}: {res}"
        assert res["VGPRs"] <= vgprs, f"{name}: {res}"


def test_design_records_the_same_values():
    """DESIGN's resource line is this table: `name` (`<faces>` for the face-move instance) LDS bytes / VGPR ceiling /
    waves per SIMD"""
    from pathlib import Path
    text = (Path(__file__).resolve().parent.parent / "DESIGN.md").read_text()
    section = text[text.index("### Cost to go"):]
    section = " ".join(section[:section.index("### Label score")].split())
    for name, (lds, vgprs, waves) in KERNELS.items():
        base = name[:name.index("I")] if "I" in name else name[:-1]
        shown = f"`{base}{'<faces>' if 'ILb1' in name else ''}` {lds:,} / {vgprs} / {waves}".replace(",", " ")
        assert shown in section, shown
