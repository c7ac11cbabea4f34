"""The binding's ABI table agrees with every prototype the headers under include/ declare: the symbols, their
order, the number of arguments, each argument's class and the return type."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
PROTOTYPE = re.compile(r"\b(int|const char\s*\*)\s*ratsdf_(\w+)\s*\(([^;{]*?)\)\s*;")
# the *_SYMBOLS list of every header
TABLES = {"ratsdf.h": "SYMBOLS", "ratsdf_map.h": "MAP_SYMBOLS", "ratsdf_sample.h": "SAMPLE_SYMBOLS",
          "ratsdf_esdf.h": "ESDF_SYMBOLS", "ratsdf_fuse.h": "FUSE_SYMBOLS", "ratsdf_resample.h": "RESAMPLE_SYMBOLS",
          "ratsdf_coarsen.h": "COARSEN_SYMBOLS", "ratsdf_surface.h": "SURFACE_SYMBOLS",
          "ratsdf_surface_mesh.h": "SURFACE_MESH_SYMBOLS", "ratsdf_cluster_mesh.h": "CLUSTER_MESH_SYMBOLS",
          "ratsdf_regions.h": "REGIONS_SYMBOLS", "ratsdf_cost.h": "COST_SYMBOLS", "ratsdf_score.h": "SCORE_SYMBOLS",
          "ratsdf_score_mesh.h": "SCORE_MESH_SYMBOLS"}
SCALARS = {"float": (C.c_float,), "int": (C.c_int, C.c_int32), "int32_t": (C.c_int, C.c_int32),
           "int64_t": (C.c_int64,), "uint32_t": (C.c_uint32,), "size_t": (C.c_size_t,)}


def prototypes(header):
    """[(symbol, returns a string, [argument text])] of a header, in file order"""
    text = header.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = []
    for ret, name, args in PROTOTYPE.findall(text):
        args = " ".join(args.split())
        out.append((name, ret != "int", [] if args in ("", "void") else [a.strip() for a in args.split(",")]))
    return out


def is_pointer(ctype):
    return ctype in (C.c_void_p, C.c_char_p) or issubclass(ctype, C._Pointer)


def agrees(arg, ctype):
    """the class of one declared argument against its ctypes type"""
    if "*" in arg or "[" in arg:
        return is_pointer(ctype)
    words = [w for w in arg.split() if w != "const"]
    return ctype in SCALARS[words[0]]        # (the last word is the argument's name)


@pytest.fixture(scope="module")
def lib():
    import ratsdf
    if not ratsdf.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return ratsdf.library()


HEADERS = sorted((ROOT / "include").glob("ratsdf*.h"))


def test_every_header_has_its_table():
    assert sorted(h.name for h in HEADERS) == sorted(TABLES)
    assert sum(len(prototypes(h)) for h in HEADERS) >= 88


@pytest.mark.parametrize("header", HEADERS, ids=lambda h: h.name)
def test_symbols_follow_the_header(header):
    from ratsdf import _abi
    declared = [name for name, _, _ in prototypes(header)]
    table = getattr(_abi, TABLES[header.name])
    assert isinstance(table, list)
    if header.name == "ratsdf.h":
        assert sorted(table) == sorted(declared) and len(table) == len(declared)
    else:
        assert table == declared


@pytest.mark.parametrize("header", HEADERS, ids=lambda h: h.name)
def test_argtypes_and_restype_follow_the_prototypes(lib, header):
    for name, returns_string, args in prototypes(header):
        assert name in lib.fn, name
        f = lib.fn[name]
        assert f.restype is (C.c_char_p if returns_string else C.c_int), name
        assert len(f.argtypes) == len(args), (name, args, f.argtypes)
        for arg, ctype in zip(args, f.argtypes):
            assert agrees(arg, ctype), (name, arg, ctype)


def test_the_binding_holds_nothing_else(lib):
    from ratsdf import _abi
    names = [s for table in TABLES.values() for s in getattr(_abi, table)]
    assert len(names) == len(set(names))
    assert set(names) == set(lib.fn)
