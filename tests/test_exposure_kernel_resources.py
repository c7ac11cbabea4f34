"""Compile-time resource guard for the exposure kernels (kernels_exposure.h; no GPU needed: hipcc cross-compiles).

None may spill.  The values pinned here are the ones the cross-compile gives and DESIGN.md 4 "Exposure" records: only the
walk uses LDS, 524 bytes (the two count rows of 64 lamps and three sums of a workgroup), and every kernel keeps 8 waves
per SIMD."""
from test_kernel_resources import resource_usage

KERNELS = {"k_exposure_packE": (0, 24, 8), "k_exposure_lampsE": (0, 16, 8), "k_exposure_walkE": (524, 56, 8)}
# mangled name's tail: (LDS bytes, VGPR ceiling, waves per SIMD)


def test_exposure_kernels_exist_do_not_spill_and_keep_their_occupancy():
    usage = resource_usage()
    assert len([n for n in usage if "k_exposure_" in n]) == len(KERNELS), sorted(n for n in usage if "k_exposure_" in n)
    for name, (lds, vgprs, waves) in KERNELS.items():
        found = [v for n, v in usage.items() if f"{len(name) - 1}{name}" in n]
        assert len(found) == 1, (name, sorted(usage))
        res = found[0]
        assert res["ScratchSize"] == 0, f"{name}: {res}"
        assert res["Occupancy"] == waves, f"{name}: {res}"
        assert res["LDS"] == lds, f"{name}: {res}"
        assert res["VGPRs"] <= vgprs, f"{name}: {res}"


def test_design_records_the_same_values():
    """DESIGN's resource line is this table: `name` LDS bytes / VGPR ceiling / waves per SIMD"""
    from pathlib import Path
    text = (Path(__file__).resolve().parent.parent / "DESIGN.md").read_text()
    section = text[text.index("### Exposure"):]
    section = " ".join(section[:section.index("\n### ", 10)].split())
    for name, (lds, vgprs, waves) in KERNELS.items():
        shown = f"`{name[:-1]}` {lds:,} / {vgprs} / {waves}".replace(",", " ")
        assert shown in section, shown
