"""The workspace layout of the exposure read-out (exposure_layout in ra-slam_amd/csrc/workspace.h;
tests/cpp/test_workspace_exposure_layout.cc).  Not a GPU test: the header is plain C++ and the program needs nothing
else.  The measured size is the hand-written sum and where the carved parts end, the parts are aligned and do not
overlap, no box has more 4 x 4 x 4 bricks than the bitmap holds, and the bound never falls as the box grows."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ra-slam_amd" / "csrc"


def test_exposure_workspace_layout(tmp_path):
    exe = tmp_path / "test_workspace_exposure_layout"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", f"-I{CSRC}",
                    str(ROOT / "tests" / "cpp" / "test_workspace_exposure_layout.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "workspace exposure layout OK: 6 sizes" in r.stdout, r.stdout + r.stderr
