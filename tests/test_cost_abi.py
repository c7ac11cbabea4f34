"""The cost-to-go ABI (include/ratsdf_cost.h) without a GPU: exports, header and binding in step, the oracle's
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
    text = (ROOT / "include" / "ratsdf_cost.h").read_text()
    declared = re.findall(r"^int ratsdf_(\w+)\(", text, flags=re.M)
    assert declared == _abi.COST_SYMBOLS == ["cost_to_go", "cost_to_go_device"]
    tables = [n for n in dir(_abi) if n.endswith("SYMBOLS") and n != "COST_SYMBOLS"]
    assert {"SYMBOLS", "ESDF_SYMBOLS", "REGIONS_SYMBOLS", "SURFACE_MESH_SYMBOLS", "COARSEN_SYMBOLS"} <= set(tables)
    for name in tables:
        assert not set(_abi.COST_SYMBOLS) & set(getattr(_abi, name)), name
    # nothing of it in ratsdf.h: the oracle exports whatever that header declares
    main = (ROOT / "include" / "ratsdf.h").read_text().lower()
    assert "cost_to_go" not in main and "ratsdf_cost" not in main
    for name in ("COST_SUMMARY_DTYPE", "CostParams", "COST_NONE", "COST_AT_GOAL", "COST_NO_STEP", "descend",
                 "COST_UNKNOWN_OCCUPIED", "COST_THROUGH_UNKNOWN", "COST_FACES_ONLY", "COST_CONTINUE"):
        assert name in ratsdf.__all__ and getattr(ratsdf, name) is getattr(_abi, name)
    assert callable(ratsdf.Engine.cost_to_go) and callable(ratsdf.Engine.cost_to_go_device)
    # the constants are the header's
    for name, value in re.findall(r"^#define RATSDF_(COST_\w+) (\w+)", text, flags=re.M):
        assert getattr(_abi, name) == int(value.rstrip("u"), 0), name
    assert _abi.COST_UNKNOWN_OCCUPIED == _abi.ESDF_UNKNOWN_OCCUPIED


def test_hip_library_exports_the_entry_points():
    from ratsdf import _abi
    lib = _hip_lib()
    for s in _abi.COST_SYMBOLS:
        assert hasattr(lib.dll, "ratsdf_" + s), f"libratsdf.so does not export ratsdf_{s}"


def test_header_compiles_as_c_with_the_declared_sizes(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include "ratsdf_cost.h"\n'
                   "typedef char params_are_16[sizeof(ratsdf_cost_params) == 16 ? 1 : -1];\n"
                   "typedef char summary_is_32[sizeof(ratsdf_cost_summary) == 32 ? 1 : -1];\n"
                   "typedef char pending_at_16[offsetof(ratsdf_cost_summary, pending) == 16 ? 1 : -1];\n"
                   "typedef char reserved_at_24[offsetof(ratsdf_cost_summary, reserved) == 24 ? 1 : -1];\n"
                   "typedef char none_is_all_ones[RATSDF_COST_NONE == 0xFFFFFFFFu ? 1 : -1];\n"
                   "int main(void) { ratsdf_cost_params p; ratsdf_cost_summary s; (void)p; (void)s;\n"
                   "  return (void*)ratsdf_cost_to_go == (void*)ratsdf_cost_to_go_device; }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}", str(src), "-o",
                    str(tmp_path / "use.o")], check=True)


def test_binding_structures_are_as_declared():
    from ratsdf import _abi
    header = (ROOT / "include" / "ratsdf_cost.h").read_text()
    ctype = {"float": C.c_float, "uint32_t": C.c_uint32, "int32_t": C.c_int32}
    body = re.search(r"typedef struct ratsdf_cost_params \{(.*?)\}", header, flags=re.S).group(1)
    fields = re.findall(r"^\s*(float|uint32_t|int32_t)\s+(\w+);", body, flags=re.M)
    assert [n for _, n in fields] == [n for n, _ in _abi.CostParams._fields_]
    assert [ctype[t] for t, _ in fields] == [t for _, t in _abi.CostParams._fields_]
    assert C.sizeof(_abi.CostParams) == 16
    d = _abi.COST_SUMMARY_DTYPE
    assert d.itemsize == 32
    body = re.search(r"typedef struct ratsdf_cost_summary \{(.*?)\} ratsdf_cost_summary;", header, flags=re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|int32_t)\s+(\w+)(?:\[2\])?;", body, flags=re.M)
    assert [n for _, n in fields] == list(d.names)
    assert [d.fields[n][0].base.str for _, n in fields] == [{"int32_t": "<i4", "uint32_t": "<u4"}[t] for t, _ in fields]
    assert [d.fields[n][1] for n in d.names] == [0, 4, 8, 12, 16, 20, 24]


def test_oracle_reports_not_implemented(make_oracle):
    import ratsdf
    from ratsdf import _abi
    e = make_oracle(0.02, 0.12)
    for s in _abi.COST_SYMBOLS:
        assert not hasattr(e.lib.dll, "ratsdf_oracle_" + s)
    for call in (lambda: e.cost_to_go([0, 0, 0], [8, 8, 8], [[1, 1, 1]]),
                 lambda: e.cost_to_go([0, 0, 0], [8, 8, 8], [], with_next=True),
                 lambda: e.cost_to_go_device([0, 0, 0], [8, 8, 8], 0, 0, 0, 0, 0, rounds=1)):
        with pytest.raises(ratsdf.RatsdfError) as ei:
            call()
        assert ei.value.status == 6


def test_calls_without_a_device_fail_with_a_status():
    """no engine handle can exist on a machine without a GPU: NULL handles are refused (RATSDF_ERR_BAD_ARGUMENT), and a
    refused call writes nothing"""
    from ratsdf import _abi
    lib = _hip_lib()
    box = [(C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(2, 2, 2)]
    params = _abi.CostParams(0.0, 0.0, 0, 0)
    goals = np.array([[0, 0, 0]], dtype=np.int32)
    cost = np.full(8, 0x5A5A5A5A, dtype=np.uint32)
    nxt = np.full(8, 0x5A, dtype=np.uint8)
    summary = np.full(8, 0x5A5A5A5A, dtype=np.uint32)
    assert lib.fn["cost_to_go"](None, *box, C.byref(params), goals.ctypes.data, 1, cost.ctypes.data, nxt.ctypes.data,
                                summary.ctypes.data) == 1
    assert lib.fn["cost_to_go"](None, None, None, None, None, 0, None, None, None) == 1
    params.rounds = 1
    assert lib.fn["cost_to_go_device"](None, *box, C.byref(params), None, 0, None, None, None) == 1
    assert lib.fn["cost_to_go_device"](None, None, None, None, None, 0, None, None, None) == 1
    assert np.all(cost == 0x5A5A5A5A) and np.all(nxt == 0x5A) and np.all(summary == 0x5A5A5A5A)
