"""Compile-time resource guard for the label-score kernels (kernels_score.h; no GPU needed: hipcc cross-compiles).

None may spill.  The values pinned here are the ones the cross-compile gives and DESIGN.md 4 "Label score" records.
The join holds a chunk of 1 024 sixteen-byte point records (16 384 bytes), two run tables of 512 words, the scan's 32
words and its 520 counters in LDS: 22 944 bytes with padding, seven workgroups of four waves per CU, which is the 7
waves per SIMD the compiler reports.  The three build kernels keep 8 waves; the bounds pass holds its eight partial
words in LDS."""
from test_kernel_resources import resource_usage

KERNELS = {"k_label_bounds": (32, 22, 8), "k_label_count": (0, 22, 8), "k_label_scatter": (0, 26, 8),
           "k_score_labels": (22944, 57, 7)}          # name: (LDS bytes, VGPRs, waves per SIMD)


def test_score_kernels_exist_do_not_spill_and_keep_their_occupancy():
    usage = resource_usage()
    for name, (lds, vgprs, waves) in KERNELS.items():
        found = [v for n, v in usage.items() if f"{len(name)}{name}E" in n]
        assert len(found) == 1, (name, sorted(usage))
        res = found[0]
        assert res["ScratchSize"] == 0, f"{name}: {res}"
        assert res["Occupancy"] == waves, f"{name}: {res}"
        assert res["LDS"] == lds, f"{name}: {res}"
        assert res["VGPRs"] <= vgprs, f"{name}: {res}"
