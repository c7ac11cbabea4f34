"""The exposure read-out through the C++ host layer (TSDFGrid::Exposure, TSDFSystem::Exposure;
tests/cpp/test_host_exposure.cc).

Against the CPU oracle's prefix both calls report not-implemented (status 6) and hand back nothing; on the HIP engine
(-m gpu) summary, lamp table, doses and masks equal the Python binding's for the same frame, box, points and lamps, byte
for byte."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from ratsdf import synthetic
from ratsdf._abi import LAMP_DTYPE

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "ra-slam_amd" / "host"
EXE = HOST / "build" / "test_host_exposure"
VS, TRUNC, MAX_DEPTH = 0.01, 0.06, 4.0
ORIGIN, DIMS = [-40, -30, 130], [80, 60, 40]            # the sphere's far cap, 1.41 .. 1.5 m from the camera
FLAGS, OCCUPIED_BELOW, MAX_RANGE, MIN_IRRADIANCE, P_CUTOFF = 0, 0.0, 0.6, 2.0, 0.5
MAX_POINTS = 700
LAMPS = np.zeros(5, dtype=LAMP_DTYPE)
LAMPS["pos"] = [(0.0, 0.0, 1.35), (-0.3, 0.2, 1.33), (0.3, -0.25, 1.32), (0.0, 0.0, 5.0), (0.1, 0.1, 1.40)]
LAMPS["power"] = [10.0, 4.0, 6.0, 1.0, 3.0]


def build_test_program():
    subprocess.run(["make", "-C", str(HOST)], check=True, capture_output=True)
    src = ROOT / "tests" / "cpp" / "test_host_exposure.cc"
    deps = [src, HOST / "src" / "tsdf_host.cc", ROOT / "include" / "ratsdf_surface.h"] + \
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
        fh.write(np.array([h, w] + ORIGIN + DIMS + [FLAGS, len(LAMPS), MAX_POINTS], dtype=np.int32).tobytes())
        fh.write(np.array(list(f["intrinsics"]) + list(f["pose"]) +
                          [VS, TRUNC, MAX_DEPTH, OCCUPIED_BELOW, MAX_RANGE, MIN_IRRADIANCE, P_CUTOFF],
                          dtype=np.float32).tobytes())
        for k, dt in (("rgb", np.uint8), ("depth", np.float32), ("ht", np.float32), ("lt", np.float32)):
            fh.write(np.ascontiguousarray(f[k], dtype=dt).tobytes())
        fh.write(LAMPS.tobytes())
    return f, path


def run(lib, prefix, tmp_path):
    exe = build_test_program()
    f, case = make_case(tmp_path)
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(lib), prefix, str(case), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, f, out


def test_host_exposure_on_oracle_is_not_implemented(oracle_lib, tmp_path):
    stdout, _, out = run(oracle_lib.path, "ratsdf_oracle_", tmp_path)
    assert "cpu-oracle" in stdout and "status 6 6" in stdout and "not implemented OK" in stdout
    assert not out.exists()


@pytest.mark.gpu
def test_host_exposure_on_hip_engine_equals_the_binding(tmp_path):
    import ratsdf
    stdout, f, out = run(ratsdf.LIB_PATH, "ratsdf_", tmp_path)
    assert "hip-gfx950" in stdout and "exposure OK" in stdout
    raw = np.fromfile(out, dtype=np.uint8)
    e = ratsdf.TSDFGrid(VS, TRUNC)
    try:
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], MAX_DEPTH, f["intrinsics"], f["pose"])
        points = e.surface_points(ORIGIN, DIMS)[:MAX_POINTS]
        dose, mask, table, summary = e.exposure(ORIGIN, DIMS, points, LAMPS, occupied_below=OCCUPIED_BELOW,
                                                max_range=MAX_RANGE, min_irradiance=MIN_IRRADIANCE,
                                                p_cutoff=P_CUTOFF, with_mask=True)
    finally:
        e.close()
    assert len(points) == MAX_POINTS and table["accepted"].tolist() == [1, 1, 1, 0, 1]
    assert summary["points_lit"] > 50 and 0 < table["lit"].sum() <= summary["lit_pairs"]
    one = np.concatenate([np.frombuffer(summary.tobytes(), dtype=np.uint8), table.view(np.uint8),
                          dose.view(np.uint8), mask.view(np.uint8)])
    assert np.array_equal(raw, np.concatenate([one, one]))
