#!/usr/bin/env python3
"""Timings of ratsdf_regions_device (include/ratsdf_regions.h) beside ratsdf_esdf_device on the same boxes:
tools/regions_bench.py [calls]  (GPU box).  The map is the 12-frame noisy sphere stream of the tests at 1 cm voxels;
the boxes are the whole map and 512 x 384 x 256 around it.  Every call is timed by the host clock with the engine's
stream synchronised before and after; the median and the minimum of `calls` (default 7) are printed.  states = 7 makes
the box one region: the worst case of the table's atomics (DESIGN 4 "Regions")."""
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "ra-slam_amd"))
import ratsdf  # noqa: E402
from ratsdf import devmem, synthetic  # noqa: E402
from ratsdf._abi import RegionsParams  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 7
e = ratsdf.TSDFGrid(0.01, 0.06)
for f in synthetic.stream("sphere", 12, scale=0.25, noise=True, holes=True):
    e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
e.synchronize()
print("map:", e.num_active_blocks(), "blocks")


def timed(fn):
    ts = []
    for _ in range(calls + 1):              # (the first call grows the workspace: dropped)
        e.synchronize()
        t0 = time.perf_counter()
        fn()
        e.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[1:]), min(ts[1:])


for origin, dims in (([-72, -56, 112], [152, 112, 48]), ([-259, -193, -60], [512, 384, 256])):
    n = int(np.prod(dims))
    capacity = 1 << 16
    d_out = devmem.DeviceArray(np.zeros(n, dtype=np.float32))
    d_lab = devmem.DeviceArray(np.zeros(n, dtype=np.int32))
    d_reg = devmem.DeviceArray(np.zeros((capacity, 32), dtype=np.uint8))
    d_cnt = devmem.DeviceArray(np.zeros(1, dtype=np.int64))
    box = [(C.c_int32 * 3)(*v) for v in (origin, dims)]
    med, lo = timed(lambda: e.esdf_device(origin, dims, d_out.data_ptr(), 0))
    print(f"box {dims} ({n} voxels): esdf_device median {med:.3f} ms, min {lo:.3f} ms")
    for states, occupied_below, min_prob in ((2, 0.0, 0.0), (7, 0.0, 0.0), (4, 0.0, 0.0), (4, 0.5, 0.0)):
        params = RegionsParams(occupied_below, min_prob, states, 0)

        def run():
            st = e.lib.fn["regions_device"](e._h, *box, C.byref(params), d_lab.data_ptr(), d_reg.data_ptr(), capacity,
                                            d_cnt.data_ptr())
            if st != 0:
                raise ratsdf.RatsdfError(st, "regions_device")

        med, lo = timed(run)
        print(f"  regions_device states={states} occupied_below={occupied_below}: {int(d_cnt.numpy()[0])} regions, "
              f"median {med:.3f} ms, min {lo:.3f} ms")
e.close()
