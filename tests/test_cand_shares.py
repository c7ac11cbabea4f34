"""The look-ahead shares of the candidate pass (ra-slam_amd/csrc/cand_shares.h; tests/cpp/test_cand_shares.cc).

Not a GPU test: the header is plain C++ and the program needs nothing else.  For every super-tile count from 1 to 9216
(ragged images among them), split_a in {0, 10, 50, 100}, split_b in {0, 30}, share B launched and not, it checks that
the three shares are disjoint and cover every tile, that B and C begin at multiples of 64 tiles, that tiles_per_wg is
in 1 .. 16 and that a share without a launch has no tiles.  (Until the arithmetic moved into the header the last one
failed wherever split_a was 100, B had no launch and the super-tile count was no multiple of 16: DESIGN.md 4.)"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ra-slam_amd" / "csrc"


def test_shares_cover_every_tile_once_and_only_in_launches_that_run(tmp_path):
    exe = tmp_path / "test_cand_shares"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", f"-I{CSRC}",
                    str(ROOT / "tests" / "cpp" / "test_cand_shares.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "cand shares OK: 26525 sizes up to 9216 super-tiles" in r.stdout, r.stdout + r.stderr
