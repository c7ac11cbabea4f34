"""Compile-time resource guard for the surface-point kernels (kernels_surface.h; no GPU needed: hipcc cross-compiles).

Both passes stage a block's neighbourhood in LDS and must not spill; the values pinned here are the ones the
cross-compile gives and DESIGN.md 4 "Surface points" records: count pass 36 VGPRs, emit pass 48 VGPRs, 14 672 bytes
of LDS each (11 x 11 rows of 24 words of tsdf, as many observed bytes, 27 block indices, the scan's 8 words), 8 waves
per SIMD."""
from test_kernel_resources import resource_usage


def test_surface_kernels_do_not_spill_and_keep_their_occupancy():
    k = {n: v for n, v in resource_usage().items() if "k_surfaceILb" in n}
    assert sorted(n.split("k_surfaceILb")[1][0] for n in k) == ["0", "1"], sorted(k)   # count pass, emit pass
    for name, res in k.items():
        assert res["ScratchSize"] == 0, f"{name}: {res}"
        assert res["LDS"] == 14672 and res["Occupancy"] == 8, f"{name}: {res}"
    count = next(v for n, v in k.items() if "k_surfaceILb0" in n)
    emit = next(v for n, v in k.items() if "k_surfaceILb1" in n)
    assert count["VGPRs"] <= 36 and emit["VGPRs"] <= 48, (count, emit)
