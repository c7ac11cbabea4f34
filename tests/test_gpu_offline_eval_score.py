"""ratsdf_offline_eval --score-labels: the four counts and the IoU it prints for the map of the committed folder dataset
equal those of the Python API on the same map (saved by the harness, loaded here) and the same labelled points."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "folder_dataset"
VOXEL = 0.02
CUTOFF, MAX_DIST, TSDF_BELOW = 0.25, 0.07, 0.2        # (no segmentation in the harness: every probability is 0.5)


def test_offline_eval_scores_the_map_like_the_python_api(tmp_path):
    import ratsdf
    from test_dataset_reader import build
    exe, lib = str(build()), str(ratsdf.LIB_PATH)
    saved, surf_file, label_file = tmp_path / "map.ratsdf", tmp_path / "surface.bin", tmp_path / "labels.bin"
    r = subprocess.run([exe, str(GOLD), "--lib", lib, "--voxel", str(VOXEL), "--save-map", str(saved),
                        "--surface-points", str(surf_file)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    surf = np.fromfile(surf_file, dtype=ratsdf.SURFACE_DTYPE)[::4]
    assert len(surf) > 200
    points = np.ascontiguousarray(surf["pos"])
    labels = (np.arange(len(surf)) % 3).astype(np.uint32)                # unannotated, low, high by turns
    rec = np.zeros(len(surf), dtype=[("xyz", "<f4", (3,)), ("label", "<u4")])
    rec["xyz"], rec["label"] = points, labels
    rec.tofile(label_file)
    # the saved map continued with no further frame, then scored
    r = subprocess.run([exe, str(GOLD), "--lib", lib, "--voxel", str(VOXEL), "--load-map", str(saved), "--frames", "0",
                        "--score-labels", str(label_file), "--score-cutoff", str(CUTOFF), "--score-max-dist",
                        str(MAX_DIST), "--score-tsdf-below", str(TSDF_BELOW)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    counts = re.search(r"^score (\d+) (\d+) (\d+) (\d+)$", r.stdout, flags=re.M)
    iou = re.search(r"^iou (\S+)$", r.stdout, flags=re.M)
    assert counts and iou and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    e = ratsdf.TSDFGrid(VOXEL, float(np.float32(VOXEL) * np.float32(6)))  # the harness' truncation: 6 voxels
    try:
        e.load_map(saved)
        with e.label_set(points, labels.astype(np.uint8)) as s:
            want = e.score_labels(s, TSDF_BELOW, MAX_DIST, CUTOFF)
    finally:
        e.close()
    assert tuple(int(v) for v in counts.groups()) == want.confusion
    assert want.confusion[0] > 100 and want.confusion[1] > 100 and want.unannotated > 100
    assert float(iou.group(1)) == want.iou
    # a file that is no whole number of records, or holds a label above 2, is refused
    bad = tmp_path / "bad.bin"
    bad.write_bytes(label_file.read_bytes()[:-3])
    r = subprocess.run([exe, str(GOLD), "--lib", lib, "--voxel", str(VOXEL), "--frames", "0", "--score-labels",
                        str(bad)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "--score-labels" in r.stderr
