#!/usr/bin/env python3
"""Timings of ratsdf_cost_to_go_device (include/ratsdf_cost.h) beside ratsdf_esdf_device and ratsdf_regions_device on
the same boxes: tools/cost_bench.py [calls]  (GPU box).  The map is the 12-frame noisy sphere stream of the tests at
1 cm voxels; the boxes are the whole map and 512 x 384 x 256 around it (tools/regions_bench.py's).  Every call is timed
by the host clock with the engine's stream synchronised before and after; the median and the minimum of `calls`
(default 7) are printed.

The goals are FREE voxels of the small box (it lies inside the large one).  For every setting the smallest power of two
of rounds at which the field has converged is found first; the call is then timed with one round (the ESDF, the seed, the
goals, one relaxation launch, the summary and the moves: everything but the relaxation) and with that many, and the
difference is the relaxation.  Per-kernel times come from running this script under a kernel trace."""
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
from ratsdf._abi import CostParams, RegionsParams  # noqa: E402

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


small = ([-72, -56, 112], [152, 112, 48])
_, state = e.esdf(*small, with_state=True)
free = np.argwhere(state == ratsdf.ESDF_STATE_FREE)
goals = np.array([[small[0][0] + x, small[0][1] + y, small[0][2] + z]
                  for z, y, x in free[[0, len(free) // 2, len(free) - 1]]], dtype=np.int32)
d_goals = devmem.DeviceArray(goals)
print("goals:", goals.tolist())

for origin, dims in (small, ([-259, -193, -60], [512, 384, 256])):
    n = int(np.prod(dims))
    d_out = devmem.DeviceArray(np.zeros(n, dtype=np.float32))
    d_lab = devmem.DeviceArray(np.zeros(n, dtype=np.int32))
    d_reg = devmem.DeviceArray(np.zeros((1 << 16, 32), dtype=np.uint8))
    d_cnt = devmem.DeviceArray(np.zeros(1, dtype=np.int64))
    d_cost = devmem.DeviceArray(np.zeros(n, dtype=np.uint32))
    d_next = devmem.DeviceArray(np.zeros(n, dtype=np.uint8))
    d_sum = devmem.DeviceArray(np.zeros(8, dtype=np.uint32))
    box = [(C.c_int32 * 3)(*v) for v in (origin, dims)]
    med, lo = timed(lambda: e.esdf_device(origin, dims, d_out.data_ptr(), 0))
    print(f"box {dims} ({n} voxels): esdf_device median {med:.3f} ms, min {lo:.3f} ms")
    params = RegionsParams(0.0, 0.0, 2, 0)

    def regions():
        st = e.lib.fn["regions_device"](e._h, *box, C.byref(params), d_lab.data_ptr(), d_reg.data_ptr(), 1 << 16,
                                        d_cnt.data_ptr())
        if st != 0:
            raise ratsdf.RatsdfError(st, "regions_device")

    med, lo = timed(regions)
    print(f"  regions_device states=2: {int(d_cnt.numpy()[0])} regions, median {med:.3f} ms, min {lo:.3f} ms")
    for clearance, through, faces in ((0.0, False, False), (0.03, False, False), (0.0, True, False), (0.0, True, True)):
        kw = dict(clearance=clearance, through_unknown=through, faces_only=faces)
        rounds = 1
        while True:
            s = e.cost_to_go_device(origin, dims, d_goals, len(goals), d_cost, d_next, d_sum, rounds=rounds, **kw)
            if s["pending"] == 0 or rounds == 4096:
                break
            rounds *= 2

        def run(r):                          # the entry point itself, as the yardsticks are timed: nothing is read back
            p = CostParams(0.0, clearance, (2 if through else 0) | (4 if faces else 0), r)
            st = e.lib.fn["cost_to_go_device"](e._h, *box, C.byref(p), d_goals.data_ptr(), len(goals),
                                               d_cost.data_ptr(), d_next.data_ptr(), d_sum.data_ptr())
            if st != 0:
                raise ratsdf.RatsdfError(st, "cost_to_go_device")

        one, _ = timed(lambda: run(1))
        med, lo = timed(lambda: run(rounds))
        print(f"  cost_to_go_device clearance={clearance} through_unknown={through} faces_only={faces}: "
              f"traversable {s['traversable']}, reached {s['reached']}, max_cost {s['max_cost']}, pending "
              f"{s['pending']} after {rounds} rounds; 1 round median {one:.3f} ms; {rounds} rounds median {med:.3f} ms, "
              f"min {lo:.3f} ms; a round {(med - one) / max(rounds - 1, 1) * 1e3:.1f} us")
e.close()
