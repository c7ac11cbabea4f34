"""The ABI of the label score against a mesh (include/ratsdf_score_mesh.h) without a GPU: exports, header and binding
in step, the symbol tables disjoint, struct sizes and offsets compiled as C99, the oracle's not-implemented status,
and calls without a device that fail with a status and write nothing."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["labelmesh_create", "labelmesh_create_device", "labelmesh_info_get", "labelmesh_destroy", "score_mesh",
         "score_mesh_device"]


def _hip_lib():
    import ratsdf
    if not ratsdf.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return ratsdf.library()


def test_header_symbols_equal_the_binding_and_are_apart_from_every_other_table():
    import ratsdf
    from ratsdf import _abi
    text = (ROOT / "include" / "ratsdf_score_mesh.h").read_text()
    declared = re.findall(r"^int ratsdf_(\w+)\(", text, flags=re.M)
    assert declared == _abi.SCORE_MESH_SYMBOLS == NAMES
    assert '#include "ratsdf_score.h"' in text
    tables = [n for n in dir(_abi) if n.endswith("SYMBOLS") and n != "SCORE_MESH_SYMBOLS"]
    assert {"SYMBOLS", "ESDF_SYMBOLS", "SURFACE_SYMBOLS", "REGIONS_SYMBOLS", "SCORE_SYMBOLS"} <= set(tables)
    for name in tables:
        assert not set(_abi.SCORE_MESH_SYMBOLS) & set(getattr(_abi, name)), name
    # nothing of it in ratsdf.h (the oracle exports whatever that header declares) nor in ratsdf_score.h
    for header in ("ratsdf.h", "ratsdf_score.h"):
        other = (ROOT / "include" / header).read_text()
        assert "labelmesh" not in other and "score_mesh" not in other
    for name in ("LabelMesh", "LabelMeshInfo"):
        assert name in ratsdf.__all__ and getattr(ratsdf, name) is getattr(_abi, name)
    for m in ("label_mesh", "score_mesh", "score_mesh_device"):
        assert callable(getattr(ratsdf.Engine, m))
    assert _abi.LABELMESH_MAX_REFS == int(re.search(r"#define RATSDF_LABELMESH_MAX_REFS\s+(\d+)", text).group(1))
    for m in ("info", "close", "__enter__", "__exit__"):
        assert hasattr(_abi.LabelMesh, m)


def test_hip_library_exports_the_entry_points():
    from ratsdf import _abi
    lib = _hip_lib()
    for s in _abi.SCORE_MESH_SYMBOLS:
        assert hasattr(lib.dll, "ratsdf_" + s), f"libratsdf.so does not export ratsdf_{s}"


def test_header_compiles_as_c_with_the_declared_sizes(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include "ratsdf_score_mesh.h"\n'
                   "typedef char info_is_72[sizeof(ratsdf_labelmesh_info) == 72 ? 1 : -1];\n"
                   "typedef char vertices_at_0[offsetof(ratsdf_labelmesh_info, vertices) == 0 ? 1 : -1];\n"
                   "typedef char triangles_at_8[offsetof(ratsdf_labelmesh_info, triangles) == 8 ? 1 : -1];\n"
                   "typedef char kept_at_16[offsetof(ratsdf_labelmesh_info, kept) == 16 ? 1 : -1];\n"
                   "typedef char mixed_at_24[offsetof(ratsdf_labelmesh_info, mixed) == 24 ? 1 : -1];\n"
                   "typedef char refs_at_32[offsetof(ratsdf_labelmesh_info, refs) == 32 ? 1 : -1];\n"
                   "typedef char cell_at_40[offsetof(ratsdf_labelmesh_info, cell) == 40 ? 1 : -1];\n"
                   "typedef char origin_at_44[offsetof(ratsdf_labelmesh_info, origin) == 44 ? 1 : -1];\n"
                   "typedef char cells_at_56[offsetof(ratsdf_labelmesh_info, cells) == 56 ? 1 : -1];\n"
                   "typedef char reserved_at_68[offsetof(ratsdf_labelmesh_info, reserved) == 68 ? 1 : -1];\n"
                   "typedef char params_are_32[sizeof(ratsdf_score_params) == 32 ? 1 : -1];\n"
                   "typedef char score_is_4160[sizeof(ratsdf_label_score) == 4160 ? 1 : -1];\n"
                   "typedef char label_is_8[sizeof(ratsdf_voxel_label) == 8 ? 1 : -1];\n"
                   "typedef char cap_is_2_25[RATSDF_LABELMESH_MAX_REFS == (1 << 25) ? 1 : -1];\n"
                   "int main(void) { ratsdf_labelmesh_info i; (void)i;\n"
                   "  return (void*)ratsdf_score_mesh == (void*)ratsdf_score_mesh_device; }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}", str(src), "-o",
                    str(tmp_path / "use.o")], check=True)


def test_binding_structure_is_as_declared():
    from ratsdf import _abi
    header = (ROOT / "include" / "ratsdf_score_mesh.h").read_text()
    ctype = {"float": C.c_float, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "int32_t": C.c_int32}
    body = re.search(r"typedef struct ratsdf_labelmesh_info \{(.*?)\}", header, flags=re.S).group(1)
    fields = re.findall(r"^\s*(float|uint32_t|int64_t|int32_t)\s+(\w+)(?:\[(\d)\])?;", body, flags=re.M)
    binding = _abi.LabelMeshInfo
    assert [n for _, n, _ in fields] == [n for n, _ in binding._fields_]
    assert [ctype[t] * int(k) if k else ctype[t] for t, _, k in fields] == [t for _, t in binding._fields_]
    assert C.sizeof(binding) == 72
    assert (binding.refs.offset, binding.cell.offset, binding.origin.offset, binding.cells.offset) == (32, 40, 44, 56)


def test_oracle_reports_not_implemented(make_oracle):
    import ratsdf
    from ratsdf import _abi
    e = make_oracle(0.02, 0.12)
    for s in _abi.SCORE_MESH_SYMBOLS:
        assert not hasattr(e.lib.dll, "ratsdf_oracle_" + s)
    pts, lab, tri = np.zeros((3, 3), np.float32), np.ones(3, np.uint8), np.arange(3, dtype=np.int32).reshape(1, 3)
    fake = _abi.LabelMesh(e.lib, C.c_void_p(0))
    for call in (lambda: e.label_mesh(pts, lab, tri), lambda: e.score_mesh(fake, max_dist=0.3),
                 lambda: e.score_mesh(fake, max_dist=0.3, per_voxel=True),
                 lambda: e.score_mesh_device(fake, 0, 0, 0, 0, max_dist=0.3), lambda: fake.info):
        with pytest.raises(ratsdf.RatsdfError) as ei:
            call()
        assert ei.value.status == 6


def test_calls_without_a_device_fail_with_a_status():
    """no engine handle can exist on a machine without a GPU: NULL handles are refused (RATSDF_ERR_BAD_ARGUMENT), and a
    refused call writes nothing"""
    from ratsdf import _abi
    lib = _hip_lib()
    pts, lab = np.zeros((4, 3), np.float32), np.ones(4, np.uint8)
    tri = np.array([[0, 1, 2], [1, 2, 3]], dtype=np.int32)
    h = C.c_void_p(0x1234)
    assert lib.fn["labelmesh_create"](None, pts.ctypes.data, lab.ctypes.data, 4, tri.ctypes.data, 2, 0.0,
                                      C.byref(h)) == 1
    assert lib.fn["labelmesh_create_device"](None, None, None, 0, None, 0, 0.0, C.byref(h)) == 1
    assert h.value == 0x1234
    info = _abi.LabelMeshInfo(triangles=-1)
    assert lib.fn["labelmesh_info_get"](None, C.byref(info)) == 1 and info.triangles == -1
    assert lib.fn["labelmesh_destroy"](None) == 1
    params = _abi.ScoreParams(0.1, 0.3, 0.5, 0, 0)
    out = np.full(520, -5, dtype=np.int64)
    p, n = C.c_void_p(0x1234), C.c_size_t(77)
    assert lib.fn["score_mesh"](None, None, C.byref(params), out.ctypes.data, C.byref(p), C.byref(n)) == 1
    assert lib.fn["score_mesh"](None, None, None, None, None, None) == 1
    assert p.value == 0x1234 and n.value == 77 and np.all(out == -5)
    count = np.full(1, -3, dtype=np.int64)
    assert lib.fn["score_mesh_device"](None, None, C.byref(params), out.ctypes.data, None, 0, count.ctypes.data) == 1
    assert lib.fn["score_mesh_device"](None, None, None, None, None, 0, None) == 1
    assert count[0] == -3 and np.all(out == -5)
