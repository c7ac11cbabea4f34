"""GPU box: cost of map coarsening (ratsdf_fuse_map_coarsened, kernels_coarsen.h) per source block, against
transformed fusion under the identity pose (ratsdf_fuse_map_transformed, kernels_resample.h) of the same source in the
same run -- the path that existed before and reads the same map through the same record path.

Source: the fly-through map of tools/fuse_probe.py (the 1280x720 room pass at 2 mm, 120 frames, ~69 k blocks).  Per
repetition two fresh, empty destinations: one of twice the voxel size takes the coarsened source, one of the same voxel
size takes the source under the identity pose.  Both calls return when the fusion is done; each is bracketed by HIP
events on the destination's stream and by the wall clock.  One JSON line: microseconds per SOURCE block of both
(median / min of the event times), the wall medians, the statistics, and the ratio.
usage: tools/coarsen_probe.py [--reps 5] [--frames 120]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "ra-slam_amd"))

IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=120)
    a = ap.parse_args()
    import torch
    import ratsdf
    from ratsdf import synthetic
    vs = 0.002
    vs2 = float(np.float32(2) * np.float32(vs))
    src = ratsdf.TSDFGrid(vs, 6 * vs)
    for i in range(a.frames):
        f = synthetic.frame("room", i, cam="l515_720p", noise=True, holes=True)
        src.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
    src.synchronize()
    n = src.num_active_blocks()

    def timed(dst, call):
        stream = torch.cuda.ExternalStream(dst.stream())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        src.synchronize()
        dst.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        stats = call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0, stats

    ev_c, ev_x, wall_c, wall_x, s_c, s_x = [], [], [], [], None, None
    for rep in range(a.reps + 1):  # (the first repetition warms up)
        d_c, d_x = ratsdf.TSDFGrid(vs2, 6 * vs), ratsdf.TSDFGrid(vs, 6 * vs)
        tc, wc, s_c = timed(d_c, lambda: d_c.fuse_map_coarsened(src))
        tx, wx, s_x = timed(d_x, lambda: d_x.fuse_map_transformed(src, IDENTITY))
        if rep:
            ev_c.append(tc)
            ev_x.append(tx)
            wall_c.append(wc)
            wall_x.append(wx)
        d_c.close()
        d_x.close()
    us = lambda t: round(float(t) * 1e6 / n, 4)
    print(json.dumps(dict(source_blocks=n, voxel_size=vs, frames=a.frames, reps=a.reps,
                          coarsened_us_per_source_block_median=us(np.median(ev_c)),
                          coarsened_us_per_source_block_min=us(min(ev_c)),
                          coarsened_wall_ms_median=round(float(np.median(wall_c)) * 1e3, 3), coarsened_stats=s_c,
                          transformed_identity_us_per_source_block_median=us(np.median(ev_x)),
                          transformed_identity_us_per_source_block_min=us(min(ev_x)),
                          transformed_identity_wall_ms_median=round(float(np.median(wall_x)) * 1e3, 3),
                          transformed_identity_stats=s_x,
                          coarsened_over_transformed=round(float(np.median(ev_c) / np.median(ev_x)), 3))), flush=True)
    src.close()


if __name__ == "__main__":
    main()
