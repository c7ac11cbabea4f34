"""ratsdf_offline_eval --score-mesh: the four counts and the IoU it prints for the map of the committed folder dataset
equal those of the Python API on the same map (saved by the harness, loaded here) and the same labelled mesh; given
together with --score-labels the lines of the two scores carry their prefixes."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "folder_dataset"
VOXEL = 0.02
CUTOFF, MAX_DIST, TSDF_BELOW = 0.25, 0.07, 0.2        # (no segmentation in the harness: every probability is 0.5)


def test_offline_eval_scores_the_map_against_a_mesh_like_the_python_api(tmp_path):
    import ratsdf
    from test_dataset_reader import build
    exe, lib = str(build()), str(ratsdf.LIB_PATH)
    saved, mesh_file, label_file = tmp_path / "map.ratsdf", tmp_path / "mesh.bin", tmp_path / "labels.bin"
    r = subprocess.run([exe, str(GOLD), "--lib", lib, "--voxel", str(VOXEL), "--save-map", str(saved)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    e = ratsdf.TSDFGrid(VOXEL, float(np.float32(VOXEL) * np.float32(6)))  # the harness' truncation: 6 voxels
    try:
        e.load_map(saved)
        _, b = e.dump_directory()
        pos = np.stack([b["x"], b["y"], b["z"]], axis=1).astype(int)
        lo, hi = pos.min(0) * 8, pos.max(0) * 8 + 7
        verts, tris = e.surface_mesh(lo, hi - lo + 1)
        tris = np.ascontiguousarray(tris[::2]).astype(np.int32)
        assert len(tris) > 200
        points = np.ascontiguousarray(verts["pos"])
        labels = (np.arange(len(verts)) % 3).astype(np.uint32)           # unannotated, low, high by turns
        rec = np.zeros(len(verts), dtype=[("xyz", "<f4", (3,)), ("label", "<u4")])
        rec["xyz"], rec["label"] = points, labels
        rec.tofile(label_file)
        with open(mesh_file, "wb") as fh:
            fh.write(np.array([len(verts), len(tris)], dtype="<i8").tobytes())
            fh.write(rec.tobytes())
            fh.write(tris.astype("<i4").tobytes())
        with e.label_mesh(points, labels.astype(np.uint8), tris) as m, \
                e.label_set(points, labels.astype(np.uint8)) as s:
            want = e.score_mesh(m, TSDF_BELOW, MAX_DIST, CUTOFF)
            want_points = e.score_labels(s, TSDF_BELOW, MAX_DIST, CUTOFF)
    finally:
        e.close()
    assert want.confusion[0] > 100 and want.confusion[1] > 100 and want.unannotated > 100
    common = [exe, str(GOLD), "--lib", lib, "--voxel", str(VOXEL), "--load-map", str(saved), "--frames", "0",
              "--score-cutoff", str(CUTOFF), "--score-max-dist", str(MAX_DIST), "--score-tsdf-below", str(TSDF_BELOW)]
    # the saved map continued with no further frame, then scored against the mesh
    r = subprocess.run(common + ["--score-mesh", str(mesh_file)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    counts = re.search(r"^score (\d+) (\d+) (\d+) (\d+)$", r.stdout, flags=re.M)
    iou = re.search(r"^iou (\S+)$", r.stdout, flags=re.M)
    assert counts and iou and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert tuple(int(v) for v in counts.groups()) == want.confusion
    assert float(iou.group(1)) == want.iou
    # against both: prefixed lines
    r = subprocess.run(common + ["--score-mesh", str(mesh_file), "--score-labels", str(label_file)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for prefix, w in (("mesh", want), ("points", want_points)):
        counts = re.search(rf"^{prefix} score (\d+) (\d+) (\d+) (\d+)$", r.stdout, flags=re.M)
        iou = re.search(rf"^{prefix} iou (\S+)$", r.stdout, flags=re.M)
        assert counts and iou, r.stdout + r.stderr
        assert tuple(int(v) for v in counts.groups()) == w.confusion and float(iou.group(1)) == w.iou
    assert not re.search(r"^(score|iou) ", r.stdout, flags=re.M)
    # a file whose length does not follow from its header, or that holds an index beyond the vertices, is refused
    bad = tmp_path / "bad.bin"
    bad.write_bytes(mesh_file.read_bytes()[:-3])
    r = subprocess.run(common + ["--score-mesh", str(bad)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "--score-mesh" in r.stderr
    raw = bytearray(mesh_file.read_bytes())
    raw[-4:] = np.array([len(verts)], dtype="<i4").tobytes()
    bad.write_bytes(bytes(raw))
    r = subprocess.run(common + ["--score-mesh", str(bad)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "--score-mesh" in r.stderr
