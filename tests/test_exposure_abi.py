"""The exposure ABI (ratsdf_exposure*, include/ratsdf_surface.h) without a GPU: exports, header and binding in step, the
oracle's not-implemented status, and calls without a device that fail with a status."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "ratsdf_surface.h"


def _hip_lib():
    import ratsdf
    if not ratsdf.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return ratsdf.library()


def test_header_symbols_equal_the_binding():
    import ratsdf
    from ratsdf import _abi
    text = HEADER.read_text()
    declared = re.findall(r"^int ratsdf_(\w+)\(", text, flags=re.M)
    assert declared == _abi.SURFACE_SYMBOLS == ["surface_points", "surface_points_device", "exposure", "exposure_device"]
    # nothing of it in ratsdf.h: the oracle exports whatever that header declares
    assert "exposure" not in (ROOT / "include" / "ratsdf.h").read_text().lower()
    for name in ("ExposureParams", "LAMP_DTYPE", "LAMP_RECORD_DTYPE", "EXPOSURE_SUMMARY_DTYPE",
                 "EXPOSURE_UNKNOWN_OCCUPIED", "EXPOSURE_ACCUMULATE", "EXPOSURE_MAX_LAMPS"):
        assert name in ratsdf.__all__ and getattr(ratsdf, name) is getattr(_abi, name)
    for method in ("exposure", "exposure_device", "surface_exposure"):
        assert callable(getattr(ratsdf.Engine, method))
    # the constants are the header's
    for name, value in re.findall(r"^#define RATSDF_(EXPOSURE_\w+) (\w+)", text, flags=re.M):
        assert getattr(_abi, name) == int(value.rstrip("u"), 0), name
    assert _abi.EXPOSURE_UNKNOWN_OCCUPIED == _abi.ESDF_UNKNOWN_OCCUPIED


def test_hip_library_exports_the_entry_points():
    lib = _hip_lib()
    for s in ("exposure", "exposure_device"):
        assert hasattr(lib.dll, "ratsdf_" + s), f"libratsdf.so does not export ratsdf_{s}"


def test_header_compiles_as_c_with_the_declared_sizes(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include "ratsdf_surface.h"\n'
                   "typedef char lamp_is_16[sizeof(ratsdf_lamp) == 16 ? 1 : -1];\n"
                   "typedef char params_are_32[sizeof(ratsdf_exposure_params) == 32 ? 1 : -1];\n"
                   "typedef char flags_at_16[offsetof(ratsdf_exposure_params, flags) == 16 ? 1 : -1];\n"
                   "typedef char record_is_16[sizeof(ratsdf_lamp_record) == 16 ? 1 : -1];\n"
                   "typedef char summary_is_32[sizeof(ratsdf_exposure_summary) == 32 ? 1 : -1];\n"
                   "typedef char accepted_at_16[offsetof(ratsdf_exposure_summary, lamps_accepted) == 16 ? 1 : -1];\n"
                   "typedef char limit_is_64[RATSDF_EXPOSURE_MAX_LAMPS == 64 ? 1 : -1];\n"
                   "int main(void) { ratsdf_exposure_params p; ratsdf_exposure_summary s; (void)p; (void)s;\n"
                   "  return (void*)ratsdf_exposure == (void*)ratsdf_exposure_device; }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}", str(src), "-o",
                    str(tmp_path / "use.o")], check=True)


def _fields(struct):
    """[(type, name, array length or None)] of a struct of the header"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER.read_text(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(t, n, int(k) if k else None)
            for t, n, k in re.findall(r"^\s*(float|uint32_t|int32_t|int64_t)\s+(\w+)(?:\[(\d+)\])?;", body, flags=re.M)]


def test_binding_structures_are_as_declared():
    from ratsdf import _abi
    ctype = {"float": C.c_float, "uint32_t": C.c_uint32, "int32_t": C.c_int32}
    fields = _fields("ratsdf_exposure_params")
    assert [n for _, n, _ in fields] == [n for n, _ in _abi.ExposureParams._fields_]
    assert [ctype[t] * k if k else ctype[t] for t, _, k in fields] == [t for _, t in _abi.ExposureParams._fields_]
    assert C.sizeof(_abi.ExposureParams) == 32
    code = {"float": "<f4", "uint32_t": "<u4", "int32_t": "<i4", "int64_t": "<i8"}
    for struct, dtype, offsets in (("ratsdf_lamp", _abi.LAMP_DTYPE, [0, 12]),
                                   ("ratsdf_lamp_record", _abi.LAMP_RECORD_DTYPE, [0, 4, 8, 12]),
                                   ("ratsdf_exposure_summary", _abi.EXPOSURE_SUMMARY_DTYPE, [0, 8, 12, 16, 20])):
        fields = _fields(struct)
        assert [n for _, n, _ in fields] == list(dtype.names), struct
        assert [dtype.fields[n][0].base.str for _, n, _ in fields] == [code[t] for t, _, _ in fields], struct
        assert [dtype.fields[n][0].shape for _, n, _ in fields] == [(k,) if k else () for _, _, k in fields], struct
        assert [dtype.fields[n][1] for n in dtype.names] == offsets, struct
    assert _abi.LAMP_DTYPE.itemsize == 16 and _abi.LAMP_RECORD_DTYPE.itemsize == 16
    assert _abi.EXPOSURE_SUMMARY_DTYPE.itemsize == 32


def test_oracle_reports_not_implemented(make_oracle):
    import ratsdf
    from ratsdf import _abi
    e = make_oracle(0.02, 0.12)
    for s in ("exposure", "exposure_device"):
        assert not hasattr(e.lib.dll, "ratsdf_oracle_" + s)
    points = np.zeros(2, dtype=_abi.SURFACE_DTYPE)
    lamps = np.zeros(1, dtype=_abi.LAMP_DTYPE)
    for call in (lambda: e.exposure([0, 0, 0], [8, 8, 8], points, lamps),
                 lambda: e.exposure([0, 0, 0], [8, 8, 8], points[:0], lamps[:0], dose=[], with_mask=True),
                 lambda: e.exposure_device([0, 0, 0], [8, 8, 8], 0, 0, 0, 0, 0, 0, 0, 0)):
        with pytest.raises(ratsdf.RatsdfError) as ei:
            call()
        assert ei.value.status == 6


def test_calls_without_a_device_fail_with_a_status():
    """no engine handle can exist on a machine without a GPU: NULL handles are refused (RATSDF_ERR_BAD_ARGUMENT), and a
    refused call writes nothing"""
    from ratsdf import _abi
    lib = _hip_lib()
    box = [(C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(2, 2, 2)]
    params = _abi.ExposureParams(0.0, float("inf"), 0.0, 0.5, 0, (C.c_uint32 * 3)(0, 0, 0))
    points = np.zeros(2, dtype=_abi.SURFACE_DTYPE)
    lamps = np.zeros(1, dtype=_abi.LAMP_DTYPE)
    dose = np.full(2, 0x5A5A5A5A, dtype=np.uint32)
    mask = np.full(2, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    table = np.full(4, 0x5A5A5A5A, dtype=np.uint32)
    summary = np.full(8, 0x5A5A5A5A, dtype=np.uint32)
    for symbol in ("exposure", "exposure_device"):
        assert lib.fn[symbol](None, *box, C.byref(params), points.ctypes.data, 2, lamps.ctypes.data, 1,
                              dose.ctypes.data, mask.ctypes.data, table.ctypes.data, summary.ctypes.data) == 1
        assert lib.fn[symbol](None, None, None, None, None, 0, None, 0, None, None, None, None) == 1
    assert np.all(dose == 0x5A5A5A5A) and np.all(mask == 0x5A5A5A5A5A5A5A5A) and np.all(table == 0x5A5A5A5A)
    assert np.all(summary == 0x5A5A5A5A)
