"""ratsdf_offline_eval --surface-mesh: the PLY it writes for the map of a folder dataset is well formed, and its first
tile's vertices and faces equal the Python API's mesh of the same box."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLY_VERTEX = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("rgb", "u1", (3,)), ("prob", "<f4"),
                       ("weight", "u1")])
PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
HEADER = ["ply", "format binary_little_endian 1.0", None, None, "property float x", "property float y",
          "property float z", "property float nx", "property float ny", "property float nz", "property uchar red",
          "property uchar green", "property uchar blue", "property float prob", "property uchar weight", None,
          "property list uchar int vertex_indices", "end_header"]


def read_ply(path):
    raw = path.read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert len(lines) == len(HEADER) and all(w is None or w == g for g, w in zip(lines, HEADER)), lines
    assert lines[2].startswith("comment ") and lines[3].startswith("element vertex ")
    assert lines[15].startswith("element face ")
    nv, nt = int(lines[3].split()[2]), int(lines[15].split()[2])
    assert PLY_VERTEX.itemsize == 32 and PLY_FACE.itemsize == 13
    assert len(raw) == end + nv * 32 + nt * 13                  # the header's counts against the file size
    v = np.frombuffer(raw, dtype=PLY_VERTEX, count=nv, offset=end)
    f = np.frombuffer(raw, dtype=PLY_FACE, count=nt, offset=end + nv * 32)
    return v, f


def test_offline_eval_writes_the_surface_mesh_of_the_map(tmp_path):
    import ratsdf
    from make_dataset import write_folder
    from test_dataset_reader import build
    write_folder(tmp_path / "ds", n=3, scale=0.25, factor=1000.0, scene="room")
    ply, saved = tmp_path / "mesh.ply", tmp_path / "map.ratsdf"
    r = subprocess.run([str(build()), str(tmp_path / "ds"), "--lib", str(ratsdf.LIB_PATH), "--voxel", "0.02",
                        "--save-map", str(saved), "--surface-mesh", str(ply)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    v, f = read_ply(ply)
    assert len(f) > 1000 and (f["n"] == 3).all()
    assert f["v"].min() >= 0 and f["v"].max() < len(v)          # every index is in range
    e = ratsdf.TSDFGrid(0.02, float(np.float32(0.02) * np.float32(6)))   # the harness' truncation: 6 voxels
    try:
        e.load_map(saved)
        _, b = e.dump_directory()
        pos = np.stack([b["x"], b["y"], b["z"]], axis=1).astype(int)
        lo, hi = pos.min(0) * 8, pos.max(0) * 8 + 7
        wv, wt = e.surface_mesh(lo, np.minimum(hi - lo + 1, 512))        # the first tile
    finally:
        e.close()
    n, k = len(wv), len(wt)
    assert k > 1000 and n <= len(v) and k <= len(f)
    if (hi - lo + 1 <= 512).all():
        assert n == len(v) and k == len(f)                      # one tile: the whole file
    assert np.array_equal(f["v"][:k], wt)
    got = v[:n]
    assert np.array_equal(got["pos"].view(np.uint32), wv["pos"].view(np.uint32))
    assert np.array_equal(got["normal"].view(np.uint32), wv["normal"].view(np.uint32))
    assert np.array_equal(got["prob"].view(np.uint32), wv["prob"].view(np.uint32))
    assert np.array_equal(got["rgb"], np.stack([wv["rgbw"]["r"], wv["rgbw"]["g"], wv["rgbw"]["b"]], axis=1))
    assert np.array_equal(got["weight"], wv["rgbw"]["weight"])
