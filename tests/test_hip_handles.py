"""The owners of the engine's events, streams and graphs, and the twin page-locked table (ra-slam_amd/csrc/hip_handles.h;
tests/cpp/test_hip_handles.cc).

Not a GPU test: without a device every create of the HIP runtime fails, which is the branch the owners' invariant is
about (empty after any failure); on an MI355X the same program takes the success branch.  Both branches, the moves and
the twin table's order of calls (wait, hand out, copy, record; the sides in turn) are also driven through a stand-in on
every machine.  A few kilobytes are asked for, never more."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
ROCM = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))


def test_hip_handle_owner_and_twin_table_invariants(tmp_path):
    exe = tmp_path / "test_hip_handles"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    f"-I{ROCM / 'include'}", str(ROOT / "tests" / "cpp" / "test_hip_handles.cc"), f"-L{ROCM / 'lib'}",
                    "-lamdhip64", f"-Wl,-rpath,{ROCM / 'lib'}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hip_handles OK" in r.stdout, r.stdout + r.stderr
    # the stand-in took both branches, whatever the runtime of this machine did
    assert "stand-in, event: 3 create(s) succeeded, 3 destroy(s)" in r.stdout
    assert "stand-in, graph: 6 create(s) succeeded, 6 destroy(s)" in r.stdout
    assert "stand-in, twin table: grown, 7 create(s), 7 destroy(s)" in r.stdout
    assert "stand-in refusing, twin table: not grown, 0 create(s), 0 destroy(s)" in r.stdout
