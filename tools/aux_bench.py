#!/usr/bin/env python3
"""Timings of the query-side entry points on the bench map, HIP engine vs
the CPU oracle (16 threads): tools/aux_bench.py  (GPU box).  The last leg times the surface points
(include/ratsdf_surface.h) and the welded surface mesh (include/ratsdf_surface_mesh.h) beside the mesh export and the
host route on the same map; `--surface` runs that leg and the mesh export alone (no oracle); `--no-oracle` runs every row on the HIP engine alone (a same-box A/B of two
libraries, RATSDF_LIB, needs no CPU column); `--cluster` runs the `--surface` legs and then times the clustered mesh
(include/ratsdf_cluster_mesh.h) at k = 2, 4, 8 beside the welded mesh, both over the bounding box as ONE box."""
import sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "ra-slam_amd")); sys.path.insert(0, str(ROOT / "tests"))
import numpy as np, torch
torch.cuda.init()
import ratsdf
from ratsdf import synthetic
from ratsdf._abi import Engine
from oracle_binding import load_oracle

vs, md = 0.005, 4.0
gpu = ratsdf.TSDFGrid(vs, 6 * vs)
only_surface = "--surface" in sys.argv or "--cluster" in sys.argv
cpu = None if only_surface or "--no-oracle" in sys.argv else Engine(load_oracle(), vs, 6 * vs, threads=16)
frames = [synthetic.frame("room", i, noise=True, holes=True) for i in range(45)]
for f in frames:
    for e in (gpu, cpu) if cpu else (gpu,):
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], md, f["intrinsics"], f["pose"])
print("map:", gpu.num_active_blocks(), "blocks")

def timed(fn, reps):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        r = fn()
    return (time.perf_counter() - t) / reps, r

f = frames[20]
H, W = f["depth"].shape
rows = []
for name, g, c, reps in [
    ("raycast 640x480 (host images out)", lambda: gpu.raycast(f["intrinsics"], H, W, f["pose"], 2 * md),
     lambda: cpu.raycast(f["intrinsics"], H, W, f["pose"], 2 * md), 20),
    ("gather_valid (16-B records)", gpu.gather_valid, cpu and cpu.gather_valid, 5),
    ("gather_valid_semantic (20-B records)", gpu.gather_valid_semantic, cpu and cpu.gather_valid_semantic, 5),
    ("query, 1 m cube", lambda: gpu.query((-0.5, 0.5, -0.5, 0.5, 1.0, 2.0)), lambda: cpu.query((-0.5, 0.5, -0.5, 0.5, 1.0, 2.0)), 10),
    ("gather_valid_mesh (marching cubes)", gpu.gather_valid_mesh, cpu and cpu.gather_valid_mesh, 3),
][4 if only_surface else 0:]:
    tg, rg = timed(g, reps)
    tc, rc = timed(c, max(1, reps // 3)) if cpu else (float("nan"), None)
    n = len(rg[0]) if isinstance(rg, tuple) else len(rg)
    rows.append((name, tg * 1e3, tc * 1e3, n))
    print(f"{name:40s} HIP {tg * 1e3:8.2f} ms   CPU-16T oracle {tc * 1e3:9.2f} ms   ({n} items)")

# ---- surface points of the map's bounding box and of a 128^3 box, beside the mesh export above and the host route ----
from ratsdf import devmem
_, blocks = gpu.dump_directory()
pos = np.stack([blocks["x"], blocks["y"], blocks["z"]], axis=1).astype(int)
lo, hi = pos.min(0) * 8, pos.max(0) * 8 + 7
# the entry point takes at most 2^27 voxels and 1024 per axis: block-aligned boxes of at most 512 cover the rest
tiles = [([x, y, z], [min(512, hi[0] - x + 1), min(512, hi[1] - y + 1), min(512, hi[2] - z + 1)])
         for z in range(lo[2], hi[2] + 1, 512) for y in range(lo[1], hi[1] + 1, 512) for x in range(lo[0], hi[0] + 1, 512)]
d_cnt = devmem.DeviceArray(np.zeros(1, dtype=np.int64))
total = sum(gpu.surface_points_device(o, d, 0, 0, d_cnt) for o, d in tiles)
d_pts = devmem.DeviceArray(np.zeros((total + 1, 8), dtype=np.int32))


def whole_box():
    n = 0
    for o, d in tiles:      # (each call returns after a synchronise: the time is the kernels', not the enqueue's)
        n += gpu.surface_points_device(o, d, d_pts.data_ptr() + 32 * n, total - n, d_cnt)
    return n


mid = (lo + hi + 1) // 2 // 8 * 8
cube = ([int(v) - 64 for v in mid], [128, 128, 128])
in_cube = int(np.all((pos * 8 >= np.array(cube[0]) - 7) & (pos * 8 < np.array(cube[0]) + 128), axis=1).sum())


def host_route():
    """every voxel of the map to the host, then a numpy sign-change search inside each block (edges across block
    seams, the observed rule, normals and compaction are not even attempted: a lower bound of the host route)"""
    rec = gpu.gather_valid_semantic()
    t = rec["tsdf"].reshape(-1, 8, 8, 8)
    neg = t < 0
    return int((neg[:, :, :, 1:] != neg[:, :, :, :-1]).sum() + (neg[:, :, 1:] != neg[:, :, :-1]).sum() +
               (neg[:, 1:] != neg[:, :-1]).sum())


t_box, n_box = timed(whole_box, 10)
t_cube, n_cube = timed(lambda: gpu.surface_points_device(*cube, d_pts, total, d_cnt), 20)
t_host, n_host = timed(host_route, 3)
t_mesh = rows[-1][1]
print(f"surface points: map of {len(pos)} blocks, bounding box {[int(v) for v in hi - lo + 1]} voxels in {len(tiles)} call(s)")
print(f"  surface_points_device, bounding box   {t_box * 1e3:8.2f} ms   ({n_box} points)")
print(f"  surface_points_device, 128^3 box      {t_cube * 1e3:8.2f} ms   ({n_cube} points, {in_cube} blocks in the box)")
print(f"  gather_valid_mesh (from above)        {t_mesh:8.2f} ms")
print(f"  host route (gather_valid_semantic + numpy sign changes inside blocks) {t_host * 1e3:8.2f} ms   ({n_host} changes)")

# ---- the welded surface mesh of the same bounding box (a library without the entry point, an earlier commit's under
# RATSDF_LIB, reports not-implemented: the line is left out then) ----
try:
    d_cnt2 = devmem.DeviceArray(np.zeros(2, dtype=np.int64))
    counts = [gpu.surface_mesh_device(o, d, 0, 0, 0, 0, d_cnt2) for o, d in tiles]
    nv, nt = sum(c[0] for c in counts), sum(c[1] for c in counts)
    d_v = devmem.DeviceArray(np.zeros((nv + 1, 8), dtype=np.int32))
    d_t = devmem.DeviceArray(np.zeros((nt + 1, 3), dtype=np.int32))

    def whole_mesh():
        v = t = 0
        for o, d in tiles:
            a, b = gpu.surface_mesh_device(o, d, d_v.data_ptr() + 32 * v, nv - v, d_t.data_ptr() + 12 * t, nt - t, d_cnt2)
            v, t = v + a, t + b
        return v, t

    t_smesh, (mv, mt) = timed(whole_mesh, 10)
    print(f"  surface_mesh_device, bounding box     {t_smesh * 1e3:8.2f} ms   ({mv} vertices, {mt} triangles; "
          f"gather_valid_mesh: {rows[-1][3]} vertices, {len(gpu.gather_valid_mesh()[1])} triangles)")
except ratsdf.RatsdfError as err:
    if err.status != 6:
        raise

# ---- the clustered mesh of the bounding box as one box, k = 2, 4, 8, beside the welded mesh of the same box ----
if "--cluster" in sys.argv:
    box = ([int(v) for v in lo], [int(v) for v in hi - lo + 1])
    assert max(box[1]) <= 1024 and np.prod(box[1], dtype=np.int64) <= 1 << 27, box
    d_cnt2 = devmem.DeviceArray(np.zeros(2, dtype=np.int64))
    nv, nt = gpu.surface_mesh_device(*box, 0, 0, 0, 0, d_cnt2)
    d_v = devmem.DeviceArray(np.zeros((nv + 1, 8), dtype=np.int32))
    d_t = devmem.DeviceArray(np.zeros((nt + 1, 3), dtype=np.int32))
    t_w, _ = timed(lambda: gpu.surface_mesh_device(*box, d_v, nv, d_t, nt, d_cnt2), 20)
    t_wc, _ = timed(lambda: gpu.surface_mesh_device(*box, 0, 0, 0, 0, d_cnt2), 20)
    print(f"cluster mesh: one box {box[1]} voxels at {box[0]}")
    print(f"  surface_mesh_device                   {t_w * 1e3:8.2f} ms   ({nv} vertices, {nt} triangles; "
          f"pure count {t_wc * 1e3:.2f} ms)")
    for k in (2, 4, 8):
        cv, ct = gpu.cluster_mesh_device(*box, 0, 0, 0, 0, d_cnt2, k)
        t_c, got = timed(lambda: gpu.cluster_mesh_device(*box, d_v, cv, d_t, ct, d_cnt2, k), 20)
        t_cc, _ = timed(lambda: gpu.cluster_mesh_device(*box, 0, 0, 0, 0, d_cnt2, k), 20)
        assert got == (cv, ct)
        print(f"  cluster_mesh_device, k = {k}            {t_c * 1e3:8.2f} ms   ({cv} vertices, {ct} triangles; "
              f"pure count {t_cc * 1e3:.2f} ms; {t_c / t_w:.2f} x the welded mesh)")
