"""Compile-time resource guard for the resampling kernels (kernels_resample.h; no GPU needed: hipcc cross-compiles).

k_resample_blocks keeps 17 loads per lane in flight behind one shared directory probe: it must not spill, and it must
keep the waves per SIMD that cover the loads' latency (recorded in DESIGN.md 4 "Transformed fusion": 57 VGPRs,
occupancy 8, 384 bytes of LDS)."""
from test_kernel_resources import resource_usage


def test_resampling_kernels_do_not_spill_and_keep_their_occupancy():
    k = {n: v for n, v in resource_usage().items() if "k_resample_" in n}
    assert sorted(n.split("k_resample_")[1][:4] for n in k) == ["bloc", "mark"], sorted(k)
    for name, res in k.items():
        assert res["ScratchSize"] == 0, f"{name}: {res}"
    blocks = next(v for n, v in k.items() if "k_resample_blocks" in n)
    assert blocks["VGPRs"] <= 57 and blocks["Occupancy"] >= 8 and blocks["LDS"] <= 384, blocks
    mark = next(v for n, v in k.items() if "k_resample_mark" in n)
    assert mark["VGPRs"] <= 6 and mark["Occupancy"] >= 8 and mark["LDS"] == 0, mark
