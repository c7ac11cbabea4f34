"""The owner of the engine's device and page-locked host memory (ra-slam_amd/csrc/hip_mem.h; tests/cpp/test_hip_mem.cc).

Not a GPU test: without a device every allocation of the HIP runtime fails, which is the branch the owner's invariant is
about (empty after any failure); on an MI355X the same program takes the success branch.  Both branches are also driven
through a stand-in allocator on every machine.  A few kilobytes are asked for, never more."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
ROCM = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))


def test_hip_mem_owner_invariants(tmp_path):
    exe = tmp_path / "test_hip_mem"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM / 'include'}",
                    str(ROOT / "tests" / "cpp" / "test_hip_mem.cc"), f"-L{ROCM / 'lib'}", "-lamdhip64",
                    f"-Wl,-rpath,{ROCM / 'lib'}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hip_mem OK" in r.stdout, r.stdout + r.stderr
    # the stand-in allocator took both branches, whatever the runtime of this machine did
    assert "stand-in, device: 3 allocation(s) succeeded, 3 free(s)" in r.stdout
    assert "stand-in refusing, page-locked: 0 allocation(s) succeeded, 0 free(s)" in r.stdout
