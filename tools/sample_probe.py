"""GPU box: throughput of batched point sampling (ratsdf_sample_points_device, kernels_sample.h).

Maps: `bench` (the bench.py map: synthetic room, 640x480, 5 mm voxels) and `fly` (a grown fly-through map: the 1280x720
room pass at 2 mm).  Point sets: `uniform` in the map's bounding box plus one truncation, `surface` (valid voxel
positions plus up to one voxel of jitter, random order) and `path` (the same points sorted along a path: Morton order
of their blocks).  Per case one JSON line: points/s and wall time per call (device buffers, a synchronisation per call,
so launch overhead included), flags seen, and the byte model -- 12 B in + 32 B out per point, plus ~7 cache lines of
128 B of directory and voxels for a random point (an estimate, not a measurement).  Kernel times come from a separate
run under `rocprofv3 --kernel-trace --stats` (k_sample).
usage: tools/sample_probe.py [--maps bench,fly] [--points 1048576,16777216] [--reps 10]"""
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


def build_map(name):
    if name == "bench":
        cam, vs, frames = "scannet", 0.005, [synthetic.frame("room", i, noise=True, holes=True) for i in range(32)]
    else:
        cam, vs, frames = "l515_720p", 0.002, [synthetic.frame("room", i, cam="l515_720p", noise=True, holes=True)
                                               for i in range(120)]
    e = ratsdf.TSDFGrid(vs, 6 * vs)
    for f in frames:
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
    e.synchronize()
    return e, vs


def morton(b):
    b = (b.astype(np.int64) + (1 << 12)) & 0x1FFF
    code = np.zeros(len(b), dtype=np.int64)
    for bit in range(13):
        for ax in range(3):
            code |= ((b[:, ax] >> bit) & 1) << (3 * bit + ax)
    return code


def point_sets(e, vs, n, rng):
    vox = e.gather_valid()
    xyz = np.stack([vox["x"], vox["y"], vox["z"]], axis=1).astype(np.float32)
    lo, hi = xyz.min(0) - 6 * vs, xyz.max(0) + 6 * vs
    uni = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    surf = (xyz[rng.integers(0, len(xyz), n)] + rng.uniform(-vs, vs, size=(n, 3))).astype(np.float32)
    path = surf[np.argsort(morton(np.floor(surf / np.float32(vs * 8))), kind="stable")]
    return {"uniform": uni, "surface": surf, "path": path}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="bench,fly")
    ap.add_argument("--points", default="1048576,16777216")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    for name in a.maps.split(","):
        e, vs = build_map(name)
        blocks = e.num_active_blocks()
        for n in [int(v) for v in a.points.split(",")]:
            for set_name, pts in point_sets(e, vs, n, rng).items():
                d_pts = devmem.DeviceArray(pts)
                d_out = devmem.DeviceArray(np.zeros(n * 32, dtype=np.uint8))
                e.sample_points_device(d_pts.data_ptr(), n, d_out.data_ptr())   # warm-up
                e.synchronize()
                t = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    e.sample_points_device(d_pts.data_ptr(), n, d_out.data_ptr())
                    e.synchronize()
                    t.append(time.perf_counter() - t0)
                flags = d_out.numpy().view(ratsdf.SAMPLE_DTYPE)["flags"]
                med = float(np.median(t))
                print(json.dumps(dict(map=name, active_blocks=blocks, set=set_name, points=n,
                                      wall_us_median=round(med * 1e6, 1), wall_us_min=round(min(t) * 1e6, 1),
                                      points_per_s=round(n / med, 0),
                                      allocated=round(float(np.mean(flags & 1 != 0)), 4),
                                      observed=round(float(np.mean(flags & 2 != 0)), 4),
                                      stream_GBps=round(n * 44 / med / 1e9, 1),
                                      model_GBps=round(n * (44 + 7 * 128) / med / 1e9, 1))), flush=True)
                del d_pts, d_out
        e.close()


if __name__ == "__main__":
    main()
