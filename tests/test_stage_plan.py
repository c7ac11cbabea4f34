"""The upload-ahead schedule of the host-image batch (ra-slam_amd/csrc/stage_plan.h; tests/cpp/test_stage_plan.cc).

Not a GPU test: the header is plain C++ and the program needs nothing else.  For every batch length from 0 to 53, every
ring position of the call's first frame and four kinds of batch (no frame packed, all packed side by side, packed but
apart, a fixed-seed mix) it runs the schedule with recording callables and checks that every frame is uploaded once and
in order, that the uploads of frames i and i + 1 precede launch(i), that a slot's previous reader has been launched
before the slot is uploaded again, that no run is too long, crosses the ring's end or takes a frame that is not packed
and adjacent, that the trace equals that of the loop as it stood inside ratsdf_integrate_batch, and that a refusal at
any step ends the loop with its status."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ra-slam_amd" / "csrc"


def test_schedule_uploads_ahead_in_order_and_as_the_earlier_loop_did(tmp_path):
    exe = tmp_path / "test_stage_plan"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}",
                    str(ROOT / "tests" / "cpp" / "test_stage_plan.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # 54 lengths x 16 ring positions x 4 kinds of batch
    assert "stage plan OK: 3456 cases, " in r.stdout, r.stdout + r.stderr
