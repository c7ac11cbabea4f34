"""Compile-time resource guard for the map-fusion kernels (kernels_fuse.h; no GPU needed: hipcc cross-compiles).

k_fuse_blocks is a bandwidth pass that keeps twelve 16-byte loads per lane in flight: it must not spill, and it must
keep enough waves per SIMD to cover the loads' latency (recorded in DESIGN.md 4 "Map fusion": 72 VGPRs, occupancy 7)."""
from test_kernel_resources import resource_usage


def test_fusion_kernels_do_not_spill_and_keep_their_occupancy():
    k = {n: v for n, v in resource_usage().items() if "k_fuse_" in n}
    assert sorted(n.split("k_fuse_")[1][:6] for n in k) == ["allocE", "blocks", "unpack"], sorted(k)
    for name, res in k.items():
        assert res["ScratchSize"] == 0 and res["LDS"] == 0, f"{name}: {res}"
    blocks = next(v for n, v in k.items() if "k_fuse_blocks" in n)
    assert blocks["VGPRs"] <= 72 and blocks["Occupancy"] >= 7, blocks
