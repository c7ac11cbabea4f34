"""Compile-time resource guard for the coarsening kernel (kernels_coarsen.h; no GPU needed: hipcc cross-compiles).

k_coarsen_blocks stages a 17^3 region of fine voxels in LDS: four workgroups of 512 lanes must share a CU's 160 KiB
(LDS at most 40 KiB) at 8 waves per SIMD, and it must not spill (recorded in DESIGN.md 4 "Map coarsening": 63 VGPRs,
occupancy 8, 29 280 bytes of LDS)."""
from test_kernel_resources import resource_usage


def test_coarsening_kernels_do_not_spill_and_keep_their_occupancy():
    k = {n: v for n, v in resource_usage().items() if "k_coarsen_" in n}
    assert sorted(n.split("k_coarsen_")[1][:6] for n in k) == ["blocks"], sorted(k)
    for name, res in k.items():
        assert "k_resample_" not in name and "k_fuse_" not in name
        assert res["ScratchSize"] == 0, f"{name}: {res}"
        assert res["LDS"] <= 40 * 1024, f"{name}: {res}"
    blocks = next(iter(k.values()))
    assert blocks["VGPRs"] <= 63 and blocks["Occupancy"] >= 8 and blocks["LDS"] <= 29280, blocks
