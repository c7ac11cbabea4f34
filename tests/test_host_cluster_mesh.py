"""The clustered mesh through the C++ host layer (TSDFGrid::ClusterMesh, TSDFSystem::ClusterMesh;
tests/cpp/test_host_cluster_mesh.cc).

Against the CPU oracle's prefix both calls report not-implemented (status 6) and hand back nothing; on the HIP engine
(-m gpu) vertices and triangles equal the Python binding's for the same frame and box, byte for byte."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from ratsdf import synthetic

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "ra-slam_amd" / "host"
EXE = HOST / "build" / "test_host_cluster_mesh"
VS, TRUNC, MAX_DEPTH = 0.01, 0.06, 4.0
ORIGIN, DIMS = [-83, -61, 97], [170, 125, 70]


def build_test_program():
    subprocess.run(["make", "-C", str(HOST)], check=True, capture_output=True)
    src = ROOT / "tests" / "cpp" / "test_host_cluster_mesh.cc"
    deps = [src, HOST / "src" / "tsdf_host.cc", ROOT / "include" / "ratsdf_cluster_mesh.h"] + \
        list((HOST / "include" / "ratsdf").glob("*.hpp"))
    if not EXE.exists() or EXE.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", f"-I{HOST / 'include'}", str(src),
                        str(HOST / "src" / "tsdf_host.cc"), "-ldl", "-o", str(EXE)], check=True)
    return EXE


def make_case(tmp_path):
    f = synthetic.frame("sphere", 0, scale=0.25)
    h, w = f["depth"].shape
    path = tmp_path / "case.bin"
    with open(path, "wb") as fh:
        fh.write(np.array([h, w] + ORIGIN + DIMS, dtype=np.int32).tobytes())
        fh.write(np.array(list(f["intrinsics"]) + list(f["pose"]) + [VS, TRUNC, MAX_DEPTH], dtype=np.float32).tobytes())
        for k, dt in (("rgb", np.uint8), ("depth", np.float32), ("ht", np.float32), ("lt", np.float32)):
            fh.write(np.ascontiguousarray(f[k], dtype=dt).tobytes())
    return f, path


def run(lib, prefix, tmp_path):
    exe = build_test_program()
    f, case = make_case(tmp_path)
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(lib), prefix, str(case), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, f, out


def test_host_cluster_mesh_on_oracle_is_not_implemented(oracle_lib, tmp_path):
    stdout, _, out = run(oracle_lib.path, "ratsdf_oracle_", tmp_path)
    assert "cpu-oracle" in stdout and "status 6 6" in stdout and "not implemented OK" in stdout
    assert not out.exists()


@pytest.mark.gpu
def test_host_cluster_mesh_on_hip_engine_equals_the_binding(tmp_path):
    import ratsdf
    stdout, f, out = run(ratsdf.LIB_PATH, "ratsdf_", tmp_path)
    assert "hip-gfx950" in stdout and "cluster mesh OK" in stdout
    raw = np.fromfile(out, dtype=np.uint8)
    e = ratsdf.TSDFGrid(VS, TRUNC)
    try:
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], MAX_DEPTH, f["intrinsics"], f["pose"])
        v, tri = e.cluster_mesh(ORIGIN, DIMS, 2)
    finally:
        e.close()
    assert len(tri) > 300                                       # the box reaches the surface
    one = np.concatenate([np.array([len(v), len(tri)], dtype=np.uint64).view(np.uint8), v.view(np.uint8),
                          np.ascontiguousarray(tri).view(np.uint8).reshape(-1)])
    assert np.array_equal(raw, np.concatenate([one, one]))
