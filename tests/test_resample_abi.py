"""The transformed-fusion ABI (include/ratsdf_resample.h) without a GPU: exports, header and binding in step, the
oracle's not-implemented status, and calls without a device that fail with a status."""
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMS = ("ratsdf_resample_blocks_device", "ratsdf_fuse_map_transformed")
POSE = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def _hip_lib():
    import ratsdf
    if not ratsdf.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return ratsdf.library()


def test_hip_library_exports_the_entry_points():
    import ratsdf
    lib = _hip_lib()
    for s in SYMS:
        assert hasattr(lib.dll, s), f"libratsdf.so does not export {s}"
    assert sorted("ratsdf_" + s for s in ratsdf._abi.RESAMPLE_SYMBOLS) == sorted(SYMS)
    text = (ROOT / "include" / "ratsdf_resample.h").read_text()
    for s in SYMS:
        assert s + "(" in text
    assert '#include "ratsdf_fuse.h"' in text
    # none of them in ratsdf.h: the oracle exports whatever that header declares
    assert "resample" not in (ROOT / "include" / "ratsdf.h").read_text()
    assert "fuse_map_transformed" not in (ROOT / "include" / "ratsdf.h").read_text()


def test_header_compiles_as_c(tmp_path):
    import subprocess
    src = tmp_path / "use.c"
    src.write_text('#include "ratsdf_resample.h"\n'
                   "int main(void) { ratsdf_pose p = {0, 0, 0, 1, 0, 0, 0}; ratsdf_fuse_stats s; (void)p; (void)s;\n"
                   "  return (void*)ratsdf_fuse_map_transformed == (void*)ratsdf_resample_blocks_device; }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}", str(src), "-o",
                    str(tmp_path / "use.o")], check=True)


def test_oracle_reports_not_implemented(make_oracle):
    import ratsdf
    a, b = make_oracle(0.01, 0.06), make_oracle(0.01, 0.06)
    for call in (lambda: a.fuse_map_transformed(b, POSE), lambda: a.resample_blocks_device(POSE, 0, 0, 0)):
        with pytest.raises(ratsdf.RatsdfError) as ei:
            call()
        assert ei.value.status == 6


def test_calls_without_a_device_fail_with_a_status():
    """no engine handle can exist on a machine without a GPU: NULL handles, with and without a pose, are refused
    (RATSDF_ERR_BAD_ARGUMENT), and a refused call writes no statistics"""
    import ctypes as C
    import ratsdf
    lib = _hip_lib()
    pose = ratsdf._abi._as_pose(POSE)
    stats = np.full(1, -1, dtype=ratsdf._abi.FUSE_STATS)
    fuse, resample = lib.fn["fuse_map_transformed"], lib.fn["resample_blocks_device"]
    assert fuse(None, None, None, None) == 1
    assert fuse(None, None, C.byref(pose), stats.ctypes.data) == 1
    assert resample(None, C.byref(pose), 0, None, None, None) == 1
    assert resample(None, None, 4, None, None, None) == 1
    assert all(int(stats[0][k]) == -1 for k in ratsdf._abi.FUSE_STATS.names)
