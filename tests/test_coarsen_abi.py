"""The coarsening ABI (include/ratsdf_coarsen.h) without a GPU: exports, header and binding in step, the oracle's
not-implemented status, and calls without a device that fail with a status."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMS = ("ratsdf_coarsen_blocks_device", "ratsdf_fuse_map_coarsened")


def _hip_lib():
    import ratsdf
    if not ratsdf.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return ratsdf.library()


def test_header_symbols_equal_the_binding_and_are_apart_from_the_core():
    import ratsdf
    text = (ROOT / "include" / "ratsdf_coarsen.h").read_text()
    declared = sorted(set(re.findall(r"^int (ratsdf_\w+)\(", text, flags=re.M)))
    assert declared == sorted(SYMS) == sorted("ratsdf_" + s for s in ratsdf._abi.COARSEN_SYMBOLS)
    assert '#include "ratsdf_fuse.h"' in text
    every_other = (ratsdf._abi.SYMBOLS + ratsdf._abi.MAP_SYMBOLS + ratsdf._abi.SAMPLE_SYMBOLS + ratsdf._abi.ESDF_SYMBOLS
                   + ratsdf._abi.FUSE_SYMBOLS + ratsdf._abi.RESAMPLE_SYMBOLS + ratsdf._abi.SURFACE_SYMBOLS)
    assert not set(ratsdf._abi.COARSEN_SYMBOLS) & set(every_other)
    # none of them in ratsdf.h: the oracle exports whatever that header declares
    assert "coarsen" not in (ROOT / "include" / "ratsdf.h").read_text()


def test_hip_library_exports_the_entry_points():
    lib = _hip_lib()
    for s in SYMS:
        assert hasattr(lib.dll, s), f"libratsdf.so does not export {s}"


def test_header_compiles_as_c(tmp_path):
    import subprocess
    src = tmp_path / "use.c"
    src.write_text('#include "ratsdf_coarsen.h"\n'
                   "int main(void) { ratsdf_fuse_stats s; (void)s;\n"
                   "  return (void*)ratsdf_fuse_map_coarsened == (void*)ratsdf_coarsen_blocks_device; }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}", str(src), "-o",
                    str(tmp_path / "use.o")], check=True)


def test_oracle_reports_not_implemented(make_oracle):
    import ratsdf
    a, b = make_oracle(0.02, 0.06), make_oracle(0.01, 0.06)
    for call in (lambda: a.fuse_map_coarsened(b), lambda: b.coarsen_blocks_device(0, 0, 0), lambda: b.coarsened()):
        with pytest.raises(ratsdf.RatsdfError) as ei:
            call()
        assert ei.value.status == 6
    with pytest.raises(ValueError):
        b.coarsened(levels=0)


def test_calls_without_a_device_fail_with_a_status():
    """no engine handle can exist on a machine without a GPU: NULL handles are refused (RATSDF_ERR_BAD_ARGUMENT), and a
    refused call writes no statistics"""
    import ratsdf
    lib = _hip_lib()
    stats = np.full(1, -1, dtype=ratsdf._abi.FUSE_STATS)
    fuse, coarsen = lib.fn["fuse_map_coarsened"], lib.fn["coarsen_blocks_device"]
    assert fuse(None, None, None) == 1
    assert fuse(None, None, stats.ctypes.data) == 1
    assert coarsen(None, 0, None, None, None) == 1
    assert coarsen(None, 4, None, None, None) == 1
    assert all(int(stats[0][k]) == -1 for k in ratsdf._abi.FUSE_STATS.names)
