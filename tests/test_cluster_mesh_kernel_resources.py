"""Compile-time resource guard for the clustered-mesh kernels (kernels_cluster_mesh.h; no GPU needed: hipcc
cross-compiles).

Both passes stage a block's neighbourhood in LDS and must not spill; the values pinned here are the ones the
cross-compile gives and DESIGN.md 4 "Clustered mesh" records: count pass 37 VGPRs and 27 056 bytes of LDS, emit pass 52
VGPRs and 33 200 bytes (12 x 12 rows of 24 words of tsdf, as many observed bytes and as many cell flags, the triangle
bitmap of 1 458 words, 27 masks, vertex starts and block indices, the scan's 8 words; the emit pass 12 x 128 words of
plane sums more), 8 waves per SIMD.  The pinned resources of k_surface and k_surface_mesh stay with their own tests."""
from test_kernel_resources import resource_usage


def test_cluster_mesh_kernels_do_not_spill_and_keep_their_occupancy():
    k = {n: v for n, v in resource_usage().items() if "k_cluster_meshILb" in n}
    assert sorted(n.split("k_cluster_meshILb")[1][0] for n in k) == ["0", "1"], sorted(k)   # count pass, emit pass
    for name, res in k.items():
        assert res["ScratchSize"] == 0, f"{name}: {res}"
        assert res["Occupancy"] == 8, f"{name}: {res}"
    count = next(v for n, v in k.items() if "k_cluster_meshILb0" in n)
    emit = next(v for n, v in k.items() if "k_cluster_meshILb1" in n)
    assert count["LDS"] == 27056 and emit["LDS"] == 33200, (count, emit)
    assert count["VGPRs"] <= 37 and emit["VGPRs"] <= 52, (count, emit)
