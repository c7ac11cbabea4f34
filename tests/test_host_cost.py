"""The cost-to-go field through the C++ host layer (TSDFGrid::CostToGo, TSDFSystem::CostToGo;
tests/cpp/test_host_cost.cc).

Against the CPU oracle's prefix both calls report not-implemented (status 6) and hand back nothing; on the HIP engine
(-m gpu) cost, moves and summary equal the Python binding's for the same frame, box and goals, byte for byte (but for
the summary's `rounds`, which the contract leaves open)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from ratsdf import synthetic

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "ra-slam_amd" / "host"
EXE = HOST / "build" / "test_host_cost"
VS, TRUNC, MAX_DEPTH = 0.01, 0.06, 4.0
ORIGIN, DIMS = [-40, -30, 100], [80, 60, 40]
FLAGS, OCCUPIED_BELOW, CLEARANCE = 2, 0.0, 0.02       # through unknown space: most of the box is walkable
GOALS = np.array([[-40, -30, 100], [39, 29, 100], [0, 0, 101], [500, 0, 0]], dtype=np.int32)


def build_test_program():
    subprocess.run(["make", "-C", str(HOST)], check=True, capture_output=True)
    src = ROOT / "tests" / "cpp" / "test_host_cost.cc"
    deps = [src, HOST / "src" / "tsdf_host.cc", ROOT / "include" / "ratsdf_cost.h"] + \
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
        fh.write(np.array([h, w] + ORIGIN + DIMS + [FLAGS, len(GOALS)], dtype=np.int32).tobytes())
        fh.write(np.array(list(f["intrinsics"]) + list(f["pose"]) + [VS, TRUNC, MAX_DEPTH, OCCUPIED_BELOW, CLEARANCE],
                          dtype=np.float32).tobytes())
        for k, dt in (("rgb", np.uint8), ("depth", np.float32), ("ht", np.float32), ("lt", np.float32)):
            fh.write(np.ascontiguousarray(f[k], dtype=dt).tobytes())
        fh.write(GOALS.tobytes())
    return f, path


def run(lib, prefix, tmp_path):
    exe = build_test_program()
    f, case = make_case(tmp_path)
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(lib), prefix, str(case), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, f, out


def test_host_cost_on_oracle_is_not_implemented(oracle_lib, tmp_path):
    stdout, _, out = run(oracle_lib.path, "ratsdf_oracle_", tmp_path)
    assert "cpu-oracle" in stdout and "status 6 6" in stdout and "not implemented OK" in stdout
    assert not out.exists()


@pytest.mark.gpu
def test_host_cost_on_hip_engine_equals_the_binding(tmp_path):
    import ratsdf
    stdout, f, out = run(ratsdf.LIB_PATH, "ratsdf_", tmp_path)
    assert "hip-gfx950" in stdout and "cost OK" in stdout
    raw = np.fromfile(out, dtype=np.uint8)
    e = ratsdf.TSDFGrid(VS, TRUNC)
    try:
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], MAX_DEPTH, f["intrinsics"], f["pose"])
        cost, nxt, summary = e.cost_to_go(ORIGIN, DIMS, GOALS, CLEARANCE, OCCUPIED_BELOW, through_unknown=True,
                                          with_next=True)
    finally:
        e.close()
    assert summary["goals"] >= 1 and summary["reached"] > 1000 and summary["traversable"] < cost.size
    summary = summary.copy()
    summary["rounds"] = 0
    one = np.concatenate([np.frombuffer(summary.tobytes(), dtype=np.uint8), cost.reshape(-1).view(np.uint8),
                          nxt.reshape(-1)])
    assert np.array_equal(raw, np.concatenate([one, one]))
