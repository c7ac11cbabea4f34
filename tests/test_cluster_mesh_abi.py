"""The clustered-mesh entry points in the library, the binding and the header (no GPU needed)."""
import ctypes as C
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_cluster_mesh_symbols_equal_the_header_and_the_library_exports_them():
    import ratsdf
    from ratsdf import _abi
    header = (ROOT / "include" / "ratsdf_cluster_mesh.h").read_text()
    declared = re.findall(r"^int ratsdf_(\w+)\(", header, flags=re.M)
    assert declared == _abi.CLUSTER_MESH_SYMBOLS
    assert not set(_abi.CLUSTER_MESH_SYMBOLS) & set(_abi.SYMBOLS)      # ratsdf.h's table stays ratsdf.h's
    assert not set(_abi.CLUSTER_MESH_SYMBOLS) & set(_abi.SURFACE_MESH_SYMBOLS)
    assert "ratsdf_cluster_mesh" not in (ROOT / "include" / "ratsdf.h").read_text()
    assert "ratsdf_cluster_mesh" not in (ROOT / "include" / "ratsdf_surface_mesh.h").read_text()
    lib = ratsdf.library()
    for s in _abi.CLUSTER_MESH_SYMBOLS:
        assert hasattr(lib.dll, "ratsdf_" + s), s


def test_oracle_reports_not_implemented(make_oracle):
    import ratsdf
    from ratsdf import _abi
    e = make_oracle(0.02, 0.12)
    for s in _abi.CLUSTER_MESH_SYMBOLS:
        assert not hasattr(e.lib.dll, "ratsdf_oracle_" + s)
    for call in (lambda: e.cluster_mesh([0, 0, 0], [8, 8, 8]),
                 lambda: e.cluster_mesh_device([0, 0, 0], [8, 8, 8], 0, 0, 0, 0, 0)):
        try:
            call()
            raise AssertionError("the oracle has no clustered mesh")
        except ratsdf.RatsdfError as err:
            assert err.status == 6


def test_struct_sizes_are_as_declared():
    from ratsdf import _abi
    header = (ROOT / "include" / "ratsdf_cluster_mesh.h").read_text()
    body = re.search(r"typedef struct ratsdf_cluster_mesh_params \{(.*?)\}", header, flags=re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|uint32_t)\s+(\w+);", body, flags=re.M)
    assert [n for _, n in fields] == [n for n, _ in _abi.ClusterMeshParams._fields_] == \
        ["min_weight", "factor", "flags", "reserved"]
    assert [{"int32_t": C.c_int32, "uint32_t": C.c_uint32}[t] for t, _ in fields] == \
        [t for _, t in _abi.ClusterMeshParams._fields_]
    assert C.sizeof(_abi.ClusterMeshParams) == 16
    assert _abi.SURFACE_DTYPE.itemsize == 32                           # the vertex record is ratsdf_surface_point
