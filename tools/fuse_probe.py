"""GPU box: cost of map fusion (ratsdf_fuse_map, kernels_fuse.h) against the other device path between two maps,
ratsdf_export_blocks_device + ratsdf_import_blocks_device of the same blocks (24 KB per block moved, overwrites).

Maps: `bench` (the bench.py map: synthetic room, 640x480, 5 mm voxels) and `fly` (the 1280x720 room pass at 2 mm).
Cases: `all` -- every block of the source is in the destination already (the destination is a copy; no allocation
needed, every pass is repeated on one pair of engines); `half` -- the destination holds every second block of the
source (a fresh destination per repetition: half of the blocks are allocated by the call).  The two paths alternate in
one process.  Per case one JSON line: wall time per call with a synchronisation (median / min), per block, GB/s
against 18 KB per block (6 read in the source, 6 read + 6 written in the destination) and that as a share of the
6.3 TB/s a float4 copy reaches.  Kernel times, the allocation passes apart from the voxel pass, come from a run of its
own under `rocprofv3 --kernel-trace --stats` (k_fuse_blocks | k_fuse_alloc, k_alloc_rank, k_commit_only, k_settle).
usage: tools/fuse_probe.py [--maps bench,fly] [--reps 5]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "ra-slam_amd"))

import ratsdf  # noqa: E402
from ratsdf import devmem, synthetic  # noqa: E402

COPY_TBPS = 6.3
PAIR_CHUNK = 4096  # blocks per export / import call, as ratsdf.multi.copy_blocks_device


def build_map(name):
    if name == "bench":
        vs, frames = 0.005, [synthetic.frame("room", i, noise=True, holes=True) for i in range(32)]
    else:
        vs, frames = 0.002, [synthetic.frame("room", i, cam="l515_720p", noise=True, holes=True) for i in range(120)]
    e = ratsdf.TSDFGrid(vs, 6 * vs)
    for f in frames:
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
    e.synchronize()
    return e, vs


def pair_copy(src, dst, d_pos, d_rec, d_missing, n):
    for lo in range(0, n, PAIR_CHUNK):
        m = min(PAIR_CHUNK, n - lo)
        src.export_blocks_device(m, d_pos.data_ptr() + lo * 6, d_rec.data_ptr(), d_missing.data_ptr())
        dst.import_blocks_device(m, d_pos.data_ptr() + lo * 6, d_rec.data_ptr())   # (same stream order: one device)
    dst.synchronize()


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="bench,fly")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for name in a.maps.split(","):
        src, vs = build_map(name)
        _, blocks = src.dump_directory()
        pos = np.ascontiguousarray(np.stack([blocks["x"], blocks["y"], blocks["z"]], axis=1).astype(np.int16))
        n = len(pos)
        d_pos = devmem.DeviceArray(pos)
        d_half = devmem.DeviceArray(np.ascontiguousarray(pos[::2]))
        d_rec = devmem.DeviceArray(np.zeros(PAIR_CHUNK * 1536, dtype=np.int32))
        d_missing = devmem.DeviceArray(np.zeros(1, dtype=np.int32))

        def destination(case):
            e = ratsdf.TSDFGrid(vs, 6 * vs)
            if case == "all":
                e.fuse_map(src)
            else:
                pair_copy(src, e, d_half, d_rec, d_missing, (n + 1) // 2)
            return e

        for case in ("all", "half"):
            t_fuse, t_pair, stats = [], [], None
            keep = [destination(case), destination(case)] if case == "all" else None
            for rep in range(a.reps + 1):  # (the first repetition warms up)
                d_f, d_p = keep if keep else (destination(case), destination(case))
                src.synchronize()
                tf, stats_now = timed(lambda: d_f.fuse_map(src))
                tp, _ = timed(lambda: pair_copy(src, d_p, d_pos, d_rec, d_missing, n))
                if rep:
                    t_fuse.append(tf)
                    t_pair.append(tp)
                if rep <= 1:
                    stats = stats_now
                if not keep:
                    d_f.close()
                    d_p.close()
            if keep:
                for e in keep:
                    e.close()
            med_f, med_p = float(np.median(t_fuse)), float(np.median(t_pair))
            gbps = n * 18432 / med_f / 1e9
            print(json.dumps(dict(map=name, case=case, blocks=n, stats=stats,
                                  fuse_wall_us_median=round(med_f * 1e6, 1), fuse_wall_us_min=round(min(t_fuse) * 1e6, 1),
                                  fuse_ns_per_block=round(med_f * 1e9 / n, 1), fuse_GBps_18KB=round(gbps, 1),
                                  share_of_float4_copy=round(gbps / (COPY_TBPS * 1e3), 3),
                                  pair_wall_us_median=round(med_p * 1e6, 1), pair_wall_us_min=round(min(t_pair) * 1e6, 1),
                                  pair_ns_per_block=round(med_p * 1e9 / n, 1),
                                  pair_over_fuse=round(med_p / med_f, 2))), flush=True)
        src.close()


if __name__ == "__main__":
    main()
