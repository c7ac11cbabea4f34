"""Compile-time resource guard for the region kernels (kernels_regions.h; no GPU needed: hipcc cross-compiles).

None may spill, and all keep 8 waves per SIMD.  The values pinned here are the ones the cross-compile gives and
DESIGN.md 4 "Regions" records: only the local pass holds a tile in LDS, 5 120 bytes (1 024 parent words and 1 024 member
bytes); the seed keeps its block index there (4 bytes) and the table pass its four waves' partial records (128 bytes);
nothing else uses LDS."""
from test_kernel_resources import resource_usage

KERNELS = {"k_regions_seed": (4, 12), "k_regions_local": (5120, 14), "k_regions_merge": (0, 13),
           "k_regions_flatten": (0, 10), "k_regions_init": (0, 6), "k_regions_accumulate": (128, 26),
           "k_regions_finish": (0, 18)}          # name: (LDS bytes, VGPRs)


def test_region_kernels_exist_do_not_spill_and_keep_their_occupancy():
    usage = resource_usage()
    for name, (lds, vgprs) in KERNELS.items():
        found = [v for n, v in usage.items() if f"{len(name)}{name}E" in n]
        assert len(found) == 1, (name, sorted(usage))
        res = found[0]
        assert res["ScratchSize"] == 0, f"{name}: {res}"
        assert res["Occupancy"] == 8, f"{name}: {res}"
        assert res["LDS"] == lds, f"{name}: {res}"
        assert res["VGPRs"] <= vgprs, f"{name}: {res}"
