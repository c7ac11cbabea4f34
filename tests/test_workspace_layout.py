"""The workspace layouts of the box read-outs (ra-slam_amd/csrc/workspace.h; tests/cpp/test_workspace_layout.cc).

Not a GPU test: the header is plain C++ and the program needs nothing else.  For the ESDF, the surface points, the
welded mesh and the regions, at counts on both sides of the 256-byte rounding and of the scan's 4096-item tile, it
checks that the size a null-based cursor measures is where the carved parts end, that every part starts where the
hand-written pointer chains of the four read-outs put it (rounded parts 256-aligned, none reaching into the next), and
that the size is the old closed-form sum."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ra-slam_amd" / "csrc"


def test_workspace_layouts_equal_the_hand_written_ones(tmp_path):
    exe = tmp_path / "test_workspace_layout"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", f"-I{CSRC}",
                    str(ROOT / "tests" / "cpp" / "test_workspace_layout.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "workspace layout OK: 4 layouts x 7 sizes" in r.stdout, r.stdout + r.stderr
