#!/usr/bin/env python3
"""Timings of the label score (include/ratsdf_score.h) on the bench map: tools/score_bench.py [calls] [points]
(GPU box; RATSDF_LIB selects the library, e.g. a build with another -DRATSDF_SCORE_CHUNK).

The map is bench.py's: 45 noisy 640 x 480 room frames at 5 mm voxels.  The labelled points are synthetic, about as many
as the vertices of a ScanNet room mesh (default 300 000): positions of near-surface voxels (|tsdf| < 0.05) drawn at
random, jittered by up to half a voxel, labelled high / low by the voxel's probability, every tenth unannotated.
Timed by the host clock with the engine's stream synchronised before and after, median and minimum of `calls`
(default 7): set creation from host arrays and from device pointers, score_labels_device without and with per-voxel
records, the host form, and as the yardstick gather_valid_semantic -- the download the reference's pipeline needs
before its KD-tree can start."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "ra-slam_amd"))
import ratsdf  # noqa: E402
from ratsdf import devmem, synthetic  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 7
n_points = int(sys.argv[2]) if len(sys.argv) > 2 else 300000
VS = 0.005
e = ratsdf.TSDFGrid(VS, 6 * VS)
for i in range(45):
    f = synthetic.frame("room", i, noise=True, holes=True)
    e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
e.synchronize()
print("library:", ratsdf.library().dll._name)
print("map:", e.num_active_blocks(), "blocks")


def timed(fn, drop=1):
    ts = []
    for _ in range(calls + drop):           # (the first call grows buffers: dropped)
        e.synchronize()
        t0 = time.perf_counter()
        fn()
        e.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[drop:]), min(ts[drop:])


vox = e.gather_valid_semantic()
print(f"gather_valid_semantic: {len(vox)} records, {vox.nbytes / 1e6:.1f} MB")
rng = np.random.default_rng(20261020)
near = np.flatnonzero(np.abs(vox["tsdf"]) < 0.05)
pick = near[rng.choice(len(near), size=n_points, replace=len(near) < n_points)]   # (a voxel may be drawn twice)
points = (np.stack([vox["x"][pick], vox["y"][pick], vox["z"][pick]], axis=1) +
          rng.uniform(-VS / 2, VS / 2, size=(len(pick), 3))).astype(np.float32)
labels = np.where(np.arange(len(pick)) % 10 == 0, 0, np.where(vox["prob"][pick] > 0.5, 2, 1)).astype(np.uint8)
n_vox = len(vox)
del vox
print(f"labelled points: {len(points)} ({(labels == 2).sum()} high, {(labels == 1).sum()} low, {(labels == 0).sum()} "
      f"unannotated)")

med, lo = timed(lambda: e.gather_valid_semantic())
print(f"gather_valid_semantic (the yardstick): median {med:.3f} ms, min {lo:.3f} ms")
med, lo = timed(lambda: e.label_set(points, labels).close())
print(f"label_set from host arrays: median {med:.3f} ms, min {lo:.3f} ms")
d_xyz, d_lab = devmem.DeviceArray(points), devmem.DeviceArray(labels)
med, lo = timed(lambda: e.label_set(d_xyz, d_lab).close())
print(f"label_set from device pointers: median {med:.3f} ms, min {lo:.3f} ms")

with e.label_set(points, labels) as s:
    print("set:", s.info)
    d_score = devmem.DeviceArray(np.zeros(520, dtype=np.int64))
    d_pv = devmem.DeviceArray(np.zeros((n_vox, 2), dtype=np.int32))
    d_count = devmem.DeviceArray(np.zeros(1, dtype=np.int64))
    for max_dist in (0.02, 0.04, 0.16):
        kw = dict(tsdf_below=0.1, max_dist=max_dist, p_cutoff=0.5)
        med, lo = timed(lambda: e.score_labels_device(s, d_score, 0, 0, d_count, **kw))
        print(f"max_dist {max_dist}: score_labels_device, no records: median {med:.3f} ms, min {lo:.3f} ms")
        med, lo = timed(lambda: e.score_labels_device(s, d_score, d_pv, n_vox, d_count, **kw))
        print(f"max_dist {max_dist}: score_labels_device, {n_vox} records: median {med:.3f} ms, min {lo:.3f} ms")
        med, lo = timed(lambda: e.score_labels(s, **kw))
        print(f"max_dist {max_dist}: score_labels (host form, no records): median {med:.3f} ms, min {lo:.3f} ms")
        print("   ", e.score_labels(s, **kw))
    med, lo = timed(lambda: e.score_labels(s, tsdf_below=0.1, max_dist=0.04, per_voxel=True))
    print(f"max_dist 0.04: score_labels (host form, records downloaded): median {med:.3f} ms, min {lo:.3f} ms")
e.close()
