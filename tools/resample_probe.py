"""GPU box: cost of transformed map fusion (ratsdf_fuse_map_transformed, kernels_resample.h) against plain fusion
(ratsdf_fuse_map, kernels_fuse.h) of the same source into twin destinations.

Source: the bench.py map (synthetic room, 640x480, 5 mm voxels, 32 frames).  Per repetition two fresh destinations:
one takes the source with ratsdf_fuse_map, the other with ratsdf_fuse_map_transformed under a generic pose (0.3 rad
about (1, 2, 3) / sqrt(14), a translation that is no multiple of the voxel size).  One JSON line: wall time per call
with its synchronisation (median / min) and the statistics of both.  Kernel times come from a run under
`rocprofv3 --kernel-trace --stats` (k_resample_blocks, k_resample_mark | k_fuse_blocks, and the allocation passes
k_fuse_alloc, k_alloc_rank, k_commit_only, k_settle); tools/resample_probe.py --summarise <kernel_trace.csv> prints
the medians per launch, the workgroups (= candidate blocks) of k_resample_blocks and its bytes per second.
usage: tools/resample_probe.py [--reps 5] | --summarise FILE"""
import argparse
import csv
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "ra-slam_amd"))

PEAK_TBPS = 8.0
_AXIS = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
POSE = tuple(float(v) for v in (*(_AXIS * math.sin(0.15)), math.cos(0.15), 0.1234, -0.0567, 0.0891))


def summarise(path):
    """medians per launch from a rocprofv3 kernel trace; for k_resample_blocks the bytes it must move -- 6 KB written per
    workgroup (a candidate block) -- per second of its summed time"""
    rows = list(csv.DictReader(open(path)))
    by = {}
    for r in rows:
        name = r["Kernel_Name"]
        for k in ("k_resample_blocks", "k_resample_mark", "k_fuse_blocks", "k_fuse_alloc", "k_fuse_unpack"):
            if k in name:
                wgs = int(r["Grid_Size_X"] if "Grid_Size_X" in r else r["Grid_Size"]) // int(
                    r["Workgroup_Size_X"] if "Workgroup_Size_X" in r else r["Workgroup_Size"])
                by.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), wgs))
    for k, v in by.items():
        ns = np.array([a for a, _ in v], dtype=np.float64)
        wg = np.array([b for _, b in v], dtype=np.float64)
        out = dict(kernel=k, launches=len(v), median_us=round(float(np.median(ns)) / 1e3, 2),
                   total_us=round(float(ns.sum()) / 1e3, 1), workgroups_total=int(wg.sum()))
        if k == "k_resample_blocks":
            full = wg == wg.max()
            out["median_us_full_chunk"] = round(float(np.median(ns[full])) / 1e3, 2)
            out["ns_per_block"] = round(float(ns.sum() / wg.sum()), 2)
            out["written_GBps"] = round(float(wg.sum() * 6144 / ns.sum()), 1)
            out["share_of_peak"] = round(float(wg.sum() * 6144 / ns.sum()) / (PEAK_TBPS * 1e3), 4)
        print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--summarise")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    import ratsdf
    from ratsdf import synthetic
    vs = 0.005
    src = ratsdf.TSDFGrid(vs, 6 * vs)
    for i in range(32):
        f = synthetic.frame("room", i, noise=True, holes=True)
        src.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
    src.synchronize()
    n = src.num_active_blocks()
    t_plain, t_xf, s_plain, s_xf = [], [], None, None
    for rep in range(a.reps + 1):  # (the first repetition warms up)
        d_plain, d_xf = ratsdf.TSDFGrid(vs, 6 * vs), ratsdf.TSDFGrid(vs, 6 * vs)
        src.synchronize()
        t0 = time.perf_counter()
        s_plain = d_plain.fuse_map(src)
        t1 = time.perf_counter()
        s_xf = d_xf.fuse_map_transformed(src, POSE)
        t2 = time.perf_counter()
        if rep:
            t_plain.append(t1 - t0)
            t_xf.append(t2 - t1)
        d_plain.close()
        d_xf.close()
    print(json.dumps(dict(source_blocks=n, voxel_size=vs, pose=POSE,
                          fuse_map_wall_us_median=round(float(np.median(t_plain)) * 1e6, 1),
                          fuse_map_wall_us_min=round(min(t_plain) * 1e6, 1), fuse_map_stats=s_plain,
                          transformed_wall_us_median=round(float(np.median(t_xf)) * 1e6, 1),
                          transformed_wall_us_min=round(min(t_xf) * 1e6, 1), transformed_stats=s_xf,
                          transformed_over_plain=round(float(np.median(t_xf) / np.median(t_plain)), 2))), flush=True)
    src.close()


if __name__ == "__main__":
    main()
