#!/usr/bin/env python3
"""Timings of ratsdf_exposure_device (include/ratsdf_surface.h): tools/exposure_bench.py [calls]  (GPU box).  The map
is 24 frames of the synthetic room at half resolution and 1 cm voxels; the box is "the far wall": origin (-160, -128,
40), 320 x 256 x 128 voxels around the wall z = 1.5 m that the camera faces.  The points are the surface points that box
yields (ratsdf_surface_points_device: they stay on the device), the lamps an 8 x 8 grid 0.7 m in front of the wall.
Every call is timed by the host clock with the engine's stream synchronised before and after; the median and the
minimum of `calls` (default 7) are printed, for 64, 8 and 1 lamps and for no points at all (the states, the bitmap and
the lamps: everything but the walks).

Then the numpy restatement (tests/exposure_ref.py) runs on the CPU on every 64th point with the 64 lamps, is timed
likewise (once), and its doses and masks are compared with the engine's byte for byte."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "ra-slam_amd"))
sys.path.insert(0, str(ROOT / "tests"))
import ratsdf  # noqa: E402
from ratsdf import devmem, synthetic  # noqa: E402
from ratsdf._abi import EXPOSURE_SUMMARY_DTYPE, LAMP_DTYPE, LAMP_RECORD_DTYPE, SURFACE_DTYPE  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 7
VS = 0.01
e = ratsdf.TSDFGrid(VS, 0.06)
for f in synthetic.stream("room", 24, scale=0.5):
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


origin, dims = [-160, -128, 40], [320, 256, 128]
d_count = devmem.DeviceArray(np.zeros(1, dtype=np.int64))
n = e.surface_points_device(origin, dims, 0, 0, d_count)
d_points = devmem.DeviceArray(np.zeros(n, dtype=SURFACE_DTYPE))
med, lo = timed(lambda: e.surface_points_device(origin, dims, d_points, n, d_count))
print(f"box {dims} at {origin} ({int(np.prod(dims))} voxels): {n} surface points; surface_points_device (with its "
      f"read-back of the count) median {med:.3f} ms, min {lo:.3f} ms")
gx, gy = np.meshgrid(np.linspace(-1.0, 1.0, 8), np.linspace(-0.8, 0.8, 8))
lamps = np.zeros(64, dtype=LAMP_DTYPE)
lamps["pos"] = np.stack([gx.reshape(-1), gy.reshape(-1), np.full(64, 0.8)], 1).astype(np.float32)
lamps["power"] = 30.0
d_lamps = devmem.DeviceArray(lamps)
d_dose = devmem.DeviceArray(np.zeros(n, dtype=np.float32))
d_mask = devmem.DeviceArray(np.zeros(n, dtype=np.uint64))
d_table = devmem.DeviceArray(np.zeros(64, dtype=LAMP_RECORD_DTYPE))
d_sum = devmem.DeviceArray(np.zeros(1, dtype=EXPOSURE_SUMMARY_DTYPE))
raw = [b.data_ptr() for b in (d_dose, d_mask, d_table, d_sum)]


def run(n_points, n_lamps):                  # raw pointers: nothing is read back inside the timed call
    e.exposure_device(origin, dims, d_points.data_ptr(), n_points, d_lamps.data_ptr(), n_lamps, *raw,
                      min_irradiance=1.0)


for n_points, n_lamps in ((0, 64), (n, 1), (n, 8), (n, 64)):
    med, lo = timed(lambda: run(n_points, n_lamps))
    s = d_sum.numpy()[0]
    pairs = n_points * n_lamps
    print(f"  exposure_device {n_points} points x {n_lamps} lamps: lit pairs {s['lit_pairs']}, points lit "
          f"{s['points_lit']}, outside {s['points_outside']}, lamps accepted {s['lamps_accepted']}; median {med:.3f} ms, "
          f"min {lo:.3f} ms" + (f"; {med * 1e6 / pairs:.2f} ns a pair" if pairs else ""))

import exposure_ref as ref  # noqa: E402
points = d_points.numpy()
sub = np.arange(0, n, 64)
t0 = time.perf_counter()
state = ref.box_state(e, origin, dims)
t1 = time.perf_counter()
want = ref.exposure(state, origin, VS, points[sub], lamps, min_irradiance=1.0)
t2 = time.perf_counter()
same = ref.same_bytes(d_dose.numpy()[sub], want[0]) and ref.same_bytes(d_mask.numpy()[sub], want[1])
print(f"  numpy restatement on every 64th point ({len(sub)} points x 64 lamps, lit pairs {want[3]['lit_pairs']}): states "
      f"{(t1 - t0) * 1e3:.0f} ms, walks {(t2 - t1) * 1e3:.0f} ms on the CPU; doses and masks equal the engine's: {same}")
e.close()
sys.exit(0 if same else 1)
