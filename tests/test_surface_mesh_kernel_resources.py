"""Compile-time resource guard for the surface-mesh kernels (kernels_surface_mesh.h; no GPU needed: hipcc
cross-compiles).

Both passes stage a block's neighbourhood in LDS and must not spill; the values pinned here are the ones the
cross-compile gives and DESIGN.md 4 "Surface mesh" records: count pass 39 VGPRs and 17 584 bytes of LDS, emit pass 44
VGPRs and 19 088 bytes (11 x 11 rows of 24 words of tsdf, as many observed bytes and as many cell flags, 27 block
indices, the scan's 8 words, 8 vertex starts; the emit pass 730 halfwords of vertex codes more), 8 waves per SIMD."""
from test_kernel_resources import resource_usage


def test_surface_mesh_kernels_do_not_spill_and_keep_their_occupancy():
    k = {n: v for n, v in resource_usage().items() if "k_surface_meshILb" in n}
    assert sorted(n.split("k_surface_meshILb")[1][0] for n in k) == ["0", "1"], sorted(k)   # count pass, emit pass
    for name, res in k.items():
        assert res["ScratchSize"] == 0, f"{name}: {res}"
        assert res["Occupancy"] == 8, f"{name}: {res}"
    count = next(v for n, v in k.items() if "k_surface_meshILb0" in n)
    emit = next(v for n, v in k.items() if "k_surface_meshILb1" in n)
    assert count["LDS"] == 17584 and emit["LDS"] == 19088, (count, emit)
    assert count["VGPRs"] <= 39 and emit["VGPRs"] <= 44, (count, emit)
