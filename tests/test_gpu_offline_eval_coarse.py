"""`ratsdf_offline_eval --save-coarse-map FILE --coarse-levels K` on the HIP engine: the checkpoint beside the full map
is the restatement of the coarsening contract (tests/coarsen_ref.py) applied K times to the full map of the same run
(needs a GPU)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import coarsen_ref
import fuse_ref

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def test_offline_eval_saves_a_coarse_map(tmp_path):
    import ratsdf
    from make_dataset import write_folder
    from test_dataset_reader import build
    write_folder(tmp_path / "ds", n=6, scale=0.25, factor=1000.0, scene="room")
    fine, coarse = tmp_path / "fine.map", tmp_path / "coarse.map"
    lib = ROOT / "ra-slam_amd" / "csrc" / "build" / "libratsdf.so"
    r = subprocess.run([str(build()), str(tmp_path / "ds"), "--lib", str(lib), "--voxel", "0.01", "--save-map", str(fine),
                        "--save-coarse-map", str(coarse), "--coarse-levels", "2"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "level 2" in r.stderr, r.stdout + r.stderr
    a, b = ratsdf.map_file_info(fine), ratsdf.map_file_info(coarse)
    assert np.float32(b["voxel_size"]) == np.float32(4) * np.float32(a["voxel_size"]) == np.float32(4) * np.float32(0.01)
    assert np.float32(b["truncation"]) == np.float32(a["truncation"])
    level = fuse_ref.set_from_map_file(fine.read_bytes())
    assert len(level[0]) > 100
    for _ in range(2):
        level, _ = coarsen_ref.coarsen_map(level)
    want, info = fuse_ref.fuse(fuse_ref.empty_set(), level)
    assert b["n_blocks"] == len(want[0]) > 4 and info["voxels_copied"] > 1000
    got = fuse_ref.set_from_map_file(coarse.read_bytes())
    fuse_ref.assert_sets_match(got, want, info["colour_known"], prob_tol=0.0, what="offline_eval --save-coarse-map")
