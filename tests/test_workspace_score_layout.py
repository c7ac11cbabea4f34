"""The workspace layout of the label scores, points and mesh (score_layout in ra-slam_amd/csrc/workspace.h;
tests/cpp/test_workspace_score_layout.cc).  Not a GPU test: the header is plain C++ and the program needs nothing else.
The measured size is where the carved parts end, the score table starts the buffer and the count lies behind it."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ra-slam_amd" / "csrc"


def test_score_workspace_layout(tmp_path):
    exe = tmp_path / "test_workspace_score_layout"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", f"-I{CSRC}",
                    str(ROOT / "tests" / "cpp" / "test_workspace_score_layout.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "workspace score layout OK: 3 sizes" in r.stdout, r.stdout + r.stderr
