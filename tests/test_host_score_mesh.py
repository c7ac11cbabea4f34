"""The label score against a mesh through the C++ host layer (TSDFGrid / TSDFSystem MakeLabelMesh and ScoreMesh, the
LabelMesh owner; tests/cpp/test_host_score_mesh.cc).

Against the CPU oracle's prefix every call reports not-implemented (status 6) and hands back nothing; on the HIP engine
(-m gpu) the set's info, the score and the per-voxel records equal the Python binding's for the same frame and mesh,
byte for byte."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from ratsdf import synthetic

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "ra-slam_amd" / "host"
EXE = HOST / "build" / "test_host_score_mesh"
VS, TRUNC, MAX_DEPTH = 0.01, 0.06, 4.0
CELL, TSDF_BELOW, MAX_DIST, P_CUTOFF, MIN_WEIGHT = 0.0, 0.1, 0.05, 0.5, 1


def build_test_program():
    subprocess.run(["make", "-C", str(HOST)], check=True, capture_output=True)
    src = ROOT / "tests" / "cpp" / "test_host_score_mesh.cc"
    deps = [src, HOST / "src" / "tsdf_host.cc", ROOT / "include" / "ratsdf_score_mesh.h"] + \
        list((HOST / "include" / "ratsdf").glob("*.hpp"))
    if not EXE.exists() or EXE.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", f"-I{HOST / 'include'}", str(src),
                        str(HOST / "src" / "tsdf_host.cc"), "-ldl", "-o", str(EXE)], check=True)
    return EXE


def write_case(path, f, vertices, labels, triangles):
    h, w = f["depth"].shape
    with open(path, "wb") as fh:
        fh.write(np.array([h, w, len(vertices), len(triangles), MIN_WEIGHT], dtype=np.int32).tobytes())
        fh.write(np.array(list(f["intrinsics"]) + list(f["pose"]) +
                          [VS, TRUNC, MAX_DEPTH, CELL, TSDF_BELOW, MAX_DIST, P_CUTOFF], dtype=np.float32).tobytes())
        for k, dt in (("rgb", np.uint8), ("depth", np.float32), ("ht", np.float32), ("lt", np.float32)):
            fh.write(np.ascontiguousarray(f[k], dtype=dt).tobytes())
        fh.write(np.ascontiguousarray(vertices, dtype=np.float32).tobytes())
        fh.write(np.ascontiguousarray(labels, dtype=np.uint8).tobytes())
        fh.write(np.ascontiguousarray(triangles, dtype=np.int32).tobytes())


def run(lib, prefix, tmp_path, f, vertices, labels, triangles):
    exe = build_test_program()
    case, out = tmp_path / "case.bin", tmp_path / "out.bin"
    write_case(case, f, vertices, labels, triangles)
    r = subprocess.run([str(exe), str(lib), prefix, str(case), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, out


def test_host_score_mesh_on_oracle_is_not_implemented(oracle_lib, tmp_path):
    f = synthetic.frame("sphere", 0, scale=0.25)
    rng = np.random.default_rng(5)
    stdout, out = run(oracle_lib.path, "ratsdf_oracle_", tmp_path, f, rng.uniform(-1, 1, size=(60, 3)),
                      rng.integers(0, 3, size=60), np.arange(60).reshape(-1, 3))
    assert "cpu-oracle" in stdout and "status 6 6 6 6 6" in stdout and "not implemented OK" in stdout
    assert not out.exists()


@pytest.mark.gpu
def test_host_score_mesh_on_hip_engine_equals_the_binding(tmp_path):
    import ratsdf
    from ratsdf._abi import LABEL_SCORE_DTYPE, VOXEL_LABEL_DTYPE, LabelMeshInfo
    f = synthetic.frame("sphere", 0, scale=0.25)
    e = ratsdf.TSDFGrid(VS, TRUNC)
    try:
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], MAX_DEPTH, f["intrinsics"], f["pose"])
        _, b = e.dump_directory()
        pos = np.stack([b["x"], b["y"], b["z"]], axis=1).astype(int)
        lo, hi = pos.min(0) * 8, pos.max(0) * 8 + 7
        verts, tris = e.surface_mesh(lo, hi - lo + 1)
        vertices = np.ascontiguousarray(verts["pos"])
        triangles = np.ascontiguousarray(tris[::3]).astype(np.int32)
        labels = np.where(np.arange(len(verts)) % 5 == 0, 0, np.where(verts["prob"] > 0.5, 2, 1)).astype(np.uint8)
        with e.label_mesh(vertices, labels, triangles, CELL) as s:
            info = s.info
            score, pv = e.score_mesh(s, TSDF_BELOW, MAX_DIST, P_CUTOFF, MIN_WEIGHT, per_voxel=True)
    finally:
        e.close()
    assert score.selected > 1000 and sum(score.confusion) > 500 and len(pv) == score.voxels and info["kept"] > 500
    stdout, out = run(ratsdf.LIB_PATH, "ratsdf_", tmp_path, f, vertices, labels, triangles)
    assert "hip-gfx950" in stdout and "score OK" in stdout
    raw = out.read_bytes()
    one = 72 + 4160 + 8 + 8 * len(pv)
    assert len(raw) == 2 * one
    for k in range(2):                                       # the grid's, then the system's
        part = raw[k * one:(k + 1) * one]
        got = LabelMeshInfo.from_buffer_copy(part[:72])
        assert (got.vertices, got.triangles, got.kept, got.mixed, got.refs, got.cell, tuple(got.origin),
                tuple(got.cells)) == tuple(info[n] for n in ("vertices", "triangles", "kept", "mixed", "refs", "cell",
                                                             "origin", "cells"))
        assert part[72:72 + 4160] == score.record.tobytes()
        assert np.frombuffer(part, dtype=np.uint64, count=1, offset=72 + 4160)[0] == len(pv)
        assert part[72 + 4160 + 8:] == pv.tobytes()
    assert np.frombuffer(raw, dtype=LABEL_SCORE_DTYPE, count=1, offset=72)["voxels"][0] == len(pv)
    assert VOXEL_LABEL_DTYPE.itemsize == 8
