"""The map-fusion ABI (include/ratsdf_fuse.h) without a GPU: exports, the statistics structure's layout against the
binding's FUSE_STATS, the oracle's not-implemented status, and the refusals that are decided on the host."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMS = ("ratsdf_fuse_map", "ratsdf_fuse_blocks", "ratsdf_fuse_blocks_device", "ratsdf_fuse_map_file")
FIELDS = ("blocks_seen", "blocks_allocated", "blocks_skipped", "voxels_copied", "voxels_averaged")


def _hip_lib():
    import ratsdf
    if not ratsdf.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return ratsdf.library()


def test_hip_library_exports_the_fusion_entry_points():
    import ratsdf
    lib = _hip_lib()
    for s in SYMS:
        assert hasattr(lib.dll, s), f"libratsdf.so does not export {s}"
    assert sorted("ratsdf_" + s for s in ratsdf._abi.FUSE_SYMBOLS) == sorted(SYMS)
    text = (ROOT / "include" / "ratsdf_fuse.h").read_text()
    for s in SYMS:
        assert s + "(" in text
    # none of them in ratsdf.h: the oracle exports whatever that header declares
    assert "ratsdf_fuse" not in (ROOT / "include" / "ratsdf.h").read_text()


def test_stats_layout_matches_the_dtype(tmp_path):
    from ratsdf._abi import FUSE_STATS
    src = tmp_path / "layout.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "ratsdf_fuse.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(ratsdf_fuse_stats), offsetof(ratsdf_fuse_stats, blocks_seen),
         offsetof(ratsdf_fuse_stats, blocks_allocated), offsetof(ratsdf_fuse_stats, blocks_skipped),
         offsetof(ratsdf_fuse_stats, voxels_copied), offsetof(ratsdf_fuse_stats, voxels_averaged));
  return 0;
}
''')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert FUSE_STATS.names == FIELDS
    assert got == [FUSE_STATS.itemsize] + [FUSE_STATS.fields[k][1] for k in FIELDS]
    assert got[0] == 40
    assert all(FUSE_STATS.fields[k][0] == np.dtype("<i8") for k in FIELDS)


def test_oracle_reports_not_implemented(make_oracle, tmp_path):
    import ratsdf
    from ratsdf._abi import RGBW_DTYPE
    a, b = make_oracle(0.01, 0.06), make_oracle(0.01, 0.06)
    calls = (lambda: a.fuse_map(b),
             lambda: a.fuse_blocks(np.zeros((1, 3), np.int16), np.zeros((1, 512), np.float32),
                                   np.zeros((1, 512), RGBW_DTYPE), np.zeros((1, 512), np.float32)),
             lambda: a.fuse_blocks_device(0, 0, 0),
             lambda: a.fuse_map_file(tmp_path / "none.map"))
    for call in calls:
        with pytest.raises(ratsdf.RatsdfError) as ei:
            call()
        assert ei.value.status == 6


def test_file_refusals_are_decided_on_the_host(tmp_path, oracle_lib):
    """ratsdf_fuse_map_file validates the file before it touches the engine or the device: a missing, truncated or
    damaged file is RATSDF_ERR_BAD_ARGUMENT on a machine without a GPU (where no engine handle can exist, so the handle
    is NULL here and a good file is refused for THAT, after its validation -- the good file's acceptance, a wrong voxel
    size and the unchanged map are checked on the GPU, tests/test_gpu_fuse.py)."""
    import mapfile_ref
    import ratsdf
    from ratsdf._abi import Engine
    import fuse_ref
    fn = _hip_lib().fn["fuse_map_file"]
    e = Engine(oracle_lib, 0.02, 0.12, block_bits=12, bucket_bits=12, threads=4)
    fuse_ref.integrate_frames([e], (0,))
    good = tmp_path / "good.map"
    good.write_bytes(mapfile_ref.from_dumps(e))
    e.close()
    assert ratsdf.map_file_info(good)["n_blocks"] > 0
    data = good.read_bytes()
    (tmp_path / "short.map").write_bytes(data[:len(data) // 2])
    flipped = bytearray(data)
    flipped[len(data) // 2] ^= 0x10
    (tmp_path / "flipped.map").write_bytes(bytes(flipped))
    stats = np.full(1, -1, dtype=_stats_dtype())
    for name in ("missing.map", "short.map", "flipped.map", "good.map"):
        assert fn(None, str(tmp_path / name).encode(), stats.ctypes.data) == 1, name
    assert fn(None, None, None) == 1
    assert all(int(stats[0][k]) == -1 for k in FIELDS)  # a refused call writes no statistics


def _stats_dtype():
    from ratsdf._abi import FUSE_STATS
    return FUSE_STATS


def test_null_handles_are_refused_without_a_device():
    lib = _hip_lib()
    assert lib.fn["fuse_map"](None, None, None) == 1
    assert lib.fn["fuse_blocks"](None, 0, None, None, None, None, None) == 1
    assert lib.fn["fuse_blocks_device"](None, 0, None, None, None) == 1
