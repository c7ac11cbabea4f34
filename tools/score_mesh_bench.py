#!/usr/bin/env python3
"""Timings of the label score against a mesh (include/ratsdf_score_mesh.h) on the bench map:
tools/score_mesh_bench.py [calls] [spacing in metres]
(GPU box; RATSDF_LIB selects the library, e.g. build/libratsdf_mesh_plain.so of `make -C ra-slam_amd/csrc
score-mesh-plain`, the other lane layout of the join, or a build with another -DRATSDF_SCORE_MESH_CHUNK).

The map is bench.py's: 45 noisy 640 x 480 room frames at 5 mm voxels.  The mesh is the room itself, the six faces of
the 4 x 2.5 x 3 m box triangulated on a regular lattice whose vertices are jittered by up to 2 mm, about as many
vertices and triangles as a ScanNet room mesh (spacing 0.014 m: about 300 000 vertices, 600 000 triangles), and a
coarse variant of ten times the spacing.  Vertices are labelled high / low by a smooth pattern, every tenth
unannotated.  Timed by the host clock with the engine's stream synchronised before and after, median and minimum of
`calls` (default 7) after a warm-up call: set creation from host arrays and from device pointers, score_mesh_device
without and with per-voxel records at three reaches, the host form; as yardsticks gather_valid_semantic -- the
download the reference's pipeline needs before pymesh can start -- and score_labels_device on the mesh's vertices."""
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
spacing = float(sys.argv[2]) if len(sys.argv) > 2 else 0.014
VS = 0.005
LO, HI = np.array([-2.0, -1.25, -1.5]), np.array([2.0, 1.25, 1.5])      # synthetic.py's room


def room_mesh(step, rng):
    """(vertices [n, 3] f32, labels [n] u8, triangles [m, 3] i32): the six faces of the room, each a lattice of about
    `step` metres split into two triangles per cell"""
    vs_, ts, base = [], [], 0
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        nu, nv = int(np.ceil((HI[u] - LO[u]) / step)), int(np.ceil((HI[v] - LO[v]) / step))
        gu, gv = np.meshgrid(np.linspace(LO[u], HI[u], nu + 1), np.linspace(LO[v], HI[v], nv + 1), indexing="ij")
        i = (np.arange(nu)[:, None] * (nv + 1) + np.arange(nv)[None, :]).reshape(-1)
        quad = np.stack([i, i + nv + 1, i + nv + 2, i, i + nv + 2, i + 1], axis=1).reshape(-1, 3)
        for side in (LO[axis], HI[axis]):
            p = np.zeros(((nu + 1) * (nv + 1), 3))
            p[:, u], p[:, v], p[:, axis] = gu.reshape(-1), gv.reshape(-1), side
            p += rng.uniform(-0.002, 0.002, size=p.shape)
            vs_.append(p)
            ts.append(quad + base)
            base += len(p)
    p = np.concatenate(vs_)
    high = np.sin(3.1 * p[:, 0]) * np.cos(2.3 * p[:, 1]) + np.sin(1.7 * p[:, 2]) > 0
    labels = np.where(np.arange(len(p)) % 10 == 0, 0, np.where(high, 2, 1)).astype(np.uint8)
    return p.astype(np.float32), labels, np.concatenate(ts).astype(np.int32)


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


n_vox = len(e.gather_valid_semantic())
med, lo = timed(lambda: e.gather_valid_semantic())
print(f"gather_valid_semantic (the yardstick), {n_vox} records: median {med:.3f} ms, min {lo:.3f} ms")
d_score = devmem.DeviceArray(np.zeros(520, dtype=np.int64))
d_pv = devmem.DeviceArray(np.zeros((n_vox, 2), dtype=np.int32))
d_count = devmem.DeviceArray(np.zeros(1, dtype=np.int64))
rng = np.random.default_rng(20261021)
for name, step in (("fine", spacing), ("coarse", 10 * spacing)):
    vertices, labels, triangles = room_mesh(step, rng)
    print(f"--- {name} mesh, spacing {step} m: {len(vertices)} vertices, {len(triangles)} triangles "
          f"({(labels == 2).sum()} high, {(labels == 1).sum()} low, {(labels == 0).sum()} unannotated vertices)")
    med, lo = timed(lambda: e.label_mesh(vertices, labels, triangles).close())
    print(f"{name}: label_mesh from host arrays: median {med:.3f} ms, min {lo:.3f} ms")
    d_v, d_l, d_t = devmem.DeviceArray(vertices), devmem.DeviceArray(labels), devmem.DeviceArray(triangles)
    med, lo = timed(lambda: e.label_mesh(d_v, d_l, d_t).close())
    print(f"{name}: label_mesh from device pointers: median {med:.3f} ms, min {lo:.3f} ms")
    with e.label_mesh(vertices, labels, triangles) as m, e.label_set(vertices, labels) as s:
        info = m.info
        print(f"{name}: set: {info}; refs / kept = {info['refs'] / max(info['kept'], 1):.3f}")
        for max_dist in (0.02, 0.04, 0.16):
            kw = dict(tsdf_below=0.1, max_dist=max_dist, p_cutoff=0.5)
            med, lo = timed(lambda: e.score_mesh_device(m, d_score, 0, 0, d_count, **kw))
            print(f"{name}: max_dist {max_dist}: score_mesh_device, no records: median {med:.3f} ms, min {lo:.3f} ms")
            med, lo = timed(lambda: e.score_mesh_device(m, d_score, d_pv, n_vox, d_count, **kw))
            print(f"{name}: max_dist {max_dist}: score_mesh_device, {n_vox} records: median {med:.3f} ms, "
                  f"min {lo:.3f} ms")
            med, lo = timed(lambda: e.score_mesh(m, **kw))
            print(f"{name}: max_dist {max_dist}: score_mesh (host form, no records): median {med:.3f} ms, "
                  f"min {lo:.3f} ms")
            med, lo = timed(lambda: e.score_labels_device(s, d_score, 0, 0, d_count, **kw))
            print(f"{name}: max_dist {max_dist}: score_labels_device on the vertices (the yardstick), no records: "
                  f"median {med:.3f} ms, min {lo:.3f} ms")
            print("    mesh  ", e.score_mesh(m, **kw))
            print("    points", e.score_labels(s, **kw))
        if name == "fine":
            med, lo = timed(lambda: e.score_mesh(m, tsdf_below=0.1, max_dist=0.04, per_voxel=True))
            print(f"{name}: max_dist 0.04: score_mesh (host form, records downloaded): median {med:.3f} ms, "
                  f"min {lo:.3f} ms")
e.close()
