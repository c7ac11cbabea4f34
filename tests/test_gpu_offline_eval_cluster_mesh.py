"""ratsdf_offline_eval --cluster-mesh: the PLY it writes for the map of a folder dataset is well formed (the layout of
--surface-mesh), and its vertices and faces equal the Python API's clustered mesh of the map's bounding box."""
import subprocess

import numpy as np
import pytest

from test_gpu_offline_eval_mesh import read_ply

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("factor", [None, 2])
def test_offline_eval_writes_the_cluster_mesh_of_the_map(tmp_path, factor):
    import ratsdf
    from make_dataset import write_folder
    from test_dataset_reader import build
    write_folder(tmp_path / "ds", n=3, scale=0.25, factor=1000.0, scene="room")
    ply, saved = tmp_path / "mesh.ply", tmp_path / "map.ratsdf"
    extra = [] if factor is None else ["--cluster-factor", str(factor)]
    r = subprocess.run([str(build()), str(tmp_path / "ds"), "--lib", str(ratsdf.LIB_PATH), "--voxel", "0.02",
                        "--save-map", str(saved), "--cluster-mesh", str(ply)] + extra, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    v, f = read_ply(ply)
    assert len(f) > 100 and (f["n"] == 3).all()
    assert f["v"].min() >= 0 and f["v"].max() < len(v)          # every index is in range
    e = ratsdf.TSDFGrid(0.02, float(np.float32(0.02) * np.float32(6)))   # the harness' truncation: 6 voxels
    try:
        e.load_map(saved)
        _, b = e.dump_directory()
        pos = np.stack([b["x"], b["y"], b["z"]], axis=1).astype(int)
        lo, hi = pos.min(0) * 8, pos.max(0) * 8 + 7
        wv, wt = e.cluster_mesh(lo, hi - lo + 1, factor or 4)   # one box: the default factor is 4
        welded = e.surface_mesh(lo, hi - lo + 1)
    finally:
        e.close()
    assert 0 < len(wv) < len(welded[0]) and 0 < len(wt) < len(welded[1])      # fewer than the welded mesh has
    assert len(v) == len(wv) and len(f) == len(wt)
    assert np.array_equal(f["v"], wt)
    assert np.array_equal(v["pos"].view(np.uint32), wv["pos"].view(np.uint32))
    assert np.array_equal(v["normal"].view(np.uint32), wv["normal"].view(np.uint32))
    assert np.array_equal(v["prob"].view(np.uint32), wv["prob"].view(np.uint32))
    assert np.array_equal(v["rgb"], np.stack([wv["rgbw"]["r"], wv["rgbw"]["g"], wv["rgbw"]["b"]], axis=1))
    assert np.array_equal(v["weight"], wv["rgbw"]["weight"])
