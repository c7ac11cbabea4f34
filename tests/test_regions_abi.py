"""The regions ABI (include/ratsdf_regions.h) without a GPU: exports, header and binding in step, the oracle's
not-implemented status, and calls without a device that fail with a status."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _hip_lib():
    import ratsdf
    if not ratsdf.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return ratsdf.library()


def test_header_symbols_equal_the_binding_and_are_apart_from_every_other_table():
    import ratsdf
    from ratsdf import _abi
    text = (ROOT / "include" / "ratsdf_regions.h").read_text()
    declared = re.findall(r"^int ratsdf_(\w+)\(", text, flags=re.M)
    assert declared == _abi.REGIONS_SYMBOLS == ["regions", "regions_device"]
    tables = [n for n in dir(_abi) if n.endswith("SYMBOLS") and n != "REGIONS_SYMBOLS"]
    assert {"SYMBOLS", "ESDF_SYMBOLS", "SURFACE_SYMBOLS", "SURFACE_MESH_SYMBOLS", "COARSEN_SYMBOLS"} <= set(tables)
    for name in tables:
        assert not set(_abi.REGIONS_SYMBOLS) & set(getattr(_abi, name)), name
    # nothing of it in ratsdf.h: the oracle exports whatever that header declares
    assert "region" not in (ROOT / "include" / "ratsdf.h").read_text()
    for name in ("REGION_DTYPE", "RegionsParams"):
        assert name in ratsdf.__all__ and getattr(ratsdf, name) is getattr(_abi, name)
    assert callable(ratsdf.Engine.regions) and callable(ratsdf.Engine.regions_device)


def test_hip_library_exports_the_entry_points():
    from ratsdf import _abi
    lib = _hip_lib()
    for s in _abi.REGIONS_SYMBOLS:
        assert hasattr(lib.dll, "ratsdf_" + s), f"libratsdf.so does not export ratsdf_{s}"


def test_header_compiles_as_c_with_the_declared_sizes(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include "ratsdf_regions.h"\n'
                   "typedef char region_is_32[sizeof(ratsdf_region) == 32 ? 1 : -1];\n"
                   "typedef char params_are_16[sizeof(ratsdf_regions_params) == 16 ? 1 : -1];\n"
                   "typedef char lo_at_16[offsetof(ratsdf_region, lo) == 16 ? 1 : -1];\n"
                   "typedef char hi_at_22[offsetof(ratsdf_region, hi) == 22 ? 1 : -1];\n"
                   "typedef char reserved_at_28[offsetof(ratsdf_region, reserved) == 28 ? 1 : -1];\n"
                   "int main(void) { ratsdf_region r; ratsdf_regions_params p; (void)r; (void)p;\n"
                   "  return (void*)ratsdf_regions == (void*)ratsdf_regions_device; }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}", str(src), "-o",
                    str(tmp_path / "use.o")], check=True)


def test_binding_structures_are_as_declared():
    from ratsdf import _abi
    header = (ROOT / "include" / "ratsdf_regions.h").read_text()
    body = re.search(r"typedef struct ratsdf_regions_params \{(.*?)\}", header, flags=re.S).group(1)
    fields = re.findall(r"^\s*(float|uint32_t)\s+(\w+);", body, flags=re.M)
    assert [n for _, n in fields] == [n for n, _ in _abi.RegionsParams._fields_]
    assert [{"float": C.c_float, "uint32_t": C.c_uint32}[t] for t, _ in fields] == \
        [t for _, t in _abi.RegionsParams._fields_]
    assert C.sizeof(_abi.RegionsParams) == 16
    d = _abi.REGION_DTYPE
    assert d.itemsize == 32
    assert [d.fields[k][1] for k in ("root", "voxels", "frontier", "faces", "lo", "hi", "reserved")] == \
        [0, 4, 8, 12, 16, 22, 28]
    body = re.search(r"typedef struct ratsdf_region \{(.*?)\} ratsdf_region;", header, flags=re.S).group(1)
    names = re.findall(r"\b(\w+)(?:\[3\])?[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == list(d.names)


def test_oracle_reports_not_implemented(make_oracle):
    import ratsdf
    from ratsdf import _abi
    e = make_oracle(0.02, 0.12)
    for s in _abi.REGIONS_SYMBOLS:
        assert not hasattr(e.lib.dll, "ratsdf_oracle_" + s)
    for call in (lambda: e.regions([0, 0, 0], [8, 8, 8]), lambda: e.regions([0, 0, 0], [8, 8, 8], with_labels=False),
                 lambda: e.regions_device([0, 0, 0], [8, 8, 8], 0, 0, 0, 0)):
        with pytest.raises(ratsdf.RatsdfError) as ei:
            call()
        assert ei.value.status == 6


def test_calls_without_a_device_fail_with_a_status():
    """no engine handle can exist on a machine without a GPU: NULL handles are refused (RATSDF_ERR_BAD_ARGUMENT), and a
    refused call writes nothing"""
    from ratsdf import _abi
    lib = _hip_lib()
    box = [(C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(2, 2, 2)]
    params = _abi.RegionsParams(0.0, 0.0, 2, 0)
    labels = np.full(8, -5, dtype=np.int32)
    out, n = C.c_void_p(0x1234), C.c_size_t(77)
    assert lib.fn["regions"](None, *box, C.byref(params), labels.ctypes.data, C.byref(out), C.byref(n)) == 1
    assert out.value == 0x1234 and n.value == 77 and np.all(labels == -5)
    assert lib.fn["regions"](None, None, None, None, None, None, None) == 1
    count = np.full(1, -3, dtype=np.int64)
    assert lib.fn["regions_device"](None, *box, C.byref(params), None, None, 0, count.ctypes.data) == 1
    assert lib.fn["regions_device"](None, None, None, None, None, None, 0, None) == 1
    assert count[0] == -3
