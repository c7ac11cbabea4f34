#!/usr/bin/env python3
"""GPU box: map checkpoint throughput (ratsdf_save_map / ratsdf_load_map) on the fly-through-grown map (the
non-repeating 1280x720 / 2 mm pass of tools/flythrough_probe.py, ~149 k blocks, ~0.9 GB of voxels).  Prints
seconds and GB/s for validation alone, load (validation included; the file is in the page cache) and save.  The device share -- k_map_pack /
k_map_unpack -- comes from a run under rocprofv3 --kernel-trace --stats.
usage: tools/mapfile_probe.py [frames] [dir]
The map is checkpointed every 30 frames while it grows; a save the engine refuses (a directory that names a pool
block twice) ends the growth and the last checkpoint written is measured: a fresh engine loads it and saves
it again, and the two files must be identical."""
import os
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "ra-slam_amd"))
import numpy as np
import torch
import ratsdf
from ratsdf import synthetic

n = int(sys.argv[1]) if len(sys.argv) > 1 else 360
out_dir = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="mapfile_probe_")
cam, vs = ("l515_720p", 0.002)
dev = torch.device("cuda", 0)
path = os.path.join(out_dir, "flythrough.map")
path2 = os.path.join(out_dir, "again.map")
eng = ratsdf.TSDFGrid(vs, 6 * vs)
t0 = time.perf_counter()
good = None
for i in range(n):
    f = synthetic.frame("room", i, cam=cam, noise=True, holes=True)
    d = [torch.from_numpy(f[k]).to(dev) for k in ("rgb", "depth", "ht", "lt")]
    H, W = f["depth"].shape
    torch.cuda.synchronize()
    eng.integrate_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), H, W, 4.0,
                         f["intrinsics"], f["pose"])
    eng.synchronize()
    if (i + 1) % 30 == 0 or i + 1 == n:  # a checkpoint every 30 frames; a refused save keeps the previous file
        try:
            eng.save_map(path)
            good = (i + 1, eng.num_active_blocks())
        except ratsdf.RatsdfError as err:
            print(f"save after {i + 1} frames ({eng.num_active_blocks()} blocks) refused: {err}", flush=True)
            break
print(f"grown: {i + 1} frames, {eng.num_active_blocks()} blocks in {time.perf_counter() - t0:.1f} s; "
      f"measuring the checkpoint of frame {good[0]} ({good[1]} blocks)", flush=True)
eng.close()
blocks = good[1]
size = os.path.getsize(path)
gb = size / 1e9
rows = []
for rep in range(3):
    t0 = time.perf_counter()
    info = ratsdf.map_file_info(path)
    t_info = time.perf_counter() - t0
    other = ratsdf.TSDFGrid(vs, 6 * vs)
    t0 = time.perf_counter()
    other.load_map(path)
    t_load = time.perf_counter() - t0
    t0 = time.perf_counter()
    other.save_map(path2)
    t_save = time.perf_counter() - t0
    assert info["n_blocks"] == blocks == other.num_active_blocks()
    if rep == 0:  # load + save reproduce the file byte for byte
        with open(path, "rb") as a, open(path2, "rb") as b:
            while True:
                x, y = a.read(1 << 26), b.read(1 << 26)
                assert x == y, "the re-saved map differs"
                if not x:
                    break
    other.close()
    rows.append((t_save, t_info, t_load))
    print(f"rep {rep}: file {gb:.3f} GB | save {t_save:.3f} s ({gb / t_save:.2f} GB/s) | validate only "
          f"{t_info:.3f} s ({gb / t_info:.2f} GB/s) | load {t_load:.3f} s ({gb / t_load:.2f} GB/s, "
          f"validation included)", flush=True)
best = np.min(np.array(rows), axis=0)
print(f"best: save {best[0]:.3f} s, validate {best[1]:.3f} s, load {best[2]:.3f} s; {blocks} blocks, {gb:.3f} GB",
      flush=True)
os.remove(path)
os.remove(path2)
