"""The surface-mesh entry points in the library, the binding and the header (no GPU needed)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def test_surface_mesh_symbols_equal_the_header_and_the_library_exports_them():
    import ratsdf
    from ratsdf import _abi
    header = (ROOT / "include" / "ratsdf_surface_mesh.h").read_text()
    declared = re.findall(r"^int ratsdf_(\w+)\(", header, flags=re.M)
    assert declared == _abi.SURFACE_MESH_SYMBOLS
    assert not set(_abi.SURFACE_MESH_SYMBOLS) & set(_abi.SYMBOLS)      # ratsdf.h's table stays ratsdf.h's
    assert not set(_abi.SURFACE_MESH_SYMBOLS) & set(_abi.SURFACE_SYMBOLS)
    assert "ratsdf_surface_mesh" not in (ROOT / "include" / "ratsdf.h").read_text()
    lib = ratsdf.library()
    for s in _abi.SURFACE_MESH_SYMBOLS:
        assert hasattr(lib.dll, "ratsdf_" + s), s


def test_oracle_reports_not_implemented(make_oracle):
    import ratsdf
    from ratsdf import _abi
    e = make_oracle(0.02, 0.12)
    for s in _abi.SURFACE_MESH_SYMBOLS:
        assert not hasattr(e.lib.dll, "ratsdf_oracle_" + s)
    for call in (lambda: e.surface_mesh([0, 0, 0], [8, 8, 8]),
                 lambda: e.surface_mesh_device([0, 0, 0], [8, 8, 8], 0, 0, 0, 0, 0)):
        try:
            call()
            raise AssertionError("the oracle has no surface mesh")
        except ratsdf.RatsdfError as err:
            assert err.status == 6


def test_struct_sizes_are_as_declared():
    from ratsdf import _abi
    header = (ROOT / "include" / "ratsdf_surface_mesh.h").read_text()
    body = re.search(r"typedef struct ratsdf_surface_mesh_params \{(.*?)\}", header, flags=re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|uint32_t)\s+(\w+);", body, flags=re.M)
    assert [n for _, n in fields] == [n for n, _ in _abi.SurfaceMeshParams._fields_]
    assert [{"int32_t": C.c_int32, "uint32_t": C.c_uint32}[t] for t, _ in fields] == \
        [t for _, t in _abi.SurfaceMeshParams._fields_]
    assert C.sizeof(_abi.SurfaceMeshParams) == 16
    d = _abi.SURFACE_DTYPE                                             # the vertex record is ratsdf_surface_point
    assert d.itemsize == 32 and [d.fields[k][1] for k in ("pos", "normal", "prob", "rgbw")] == [0, 12, 24, 28]
    assert np.dtype("<i4").itemsize * 3 == 12                          # an index triple
