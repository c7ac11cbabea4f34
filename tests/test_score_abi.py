"""The label-score ABI (include/ratsdf_score.h) without a GPU: exports, header and binding in step, struct sizes and
offsets compiled as C99, the oracle's not-implemented status, calls without a device that fail with a status, and the
figures of the LabelScore result."""
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
    text = (ROOT / "include" / "ratsdf_score.h").read_text()
    declared = re.findall(r"^int ratsdf_(\w+)\(", text, flags=re.M)
    assert declared == _abi.SCORE_SYMBOLS == ["labelset_create", "labelset_create_device", "labelset_info_get",
                                              "labelset_destroy", "score_labels", "score_labels_device"]
    tables = [n for n in dir(_abi) if n.endswith("SYMBOLS") and n != "SCORE_SYMBOLS"]
    assert {"SYMBOLS", "ESDF_SYMBOLS", "SURFACE_SYMBOLS", "REGIONS_SYMBOLS", "COARSEN_SYMBOLS"} <= set(tables)
    for name in tables:
        assert not set(_abi.SCORE_SYMBOLS) & set(getattr(_abi, name)), name
    # nothing of it in ratsdf.h: the oracle exports whatever that header declares
    core = (ROOT / "include" / "ratsdf.h").read_text()
    assert "labelset" not in core and "score" not in core
    for name in ("LABEL_SCORE_DTYPE", "VOXEL_LABEL_DTYPE", "ScoreParams", "LabelSet", "LabelScore", "LABEL_IGNORE",
                 "LABEL_LOW", "LABEL_HIGH"):
        assert name in ratsdf.__all__ and getattr(ratsdf, name) is getattr(_abi, name)
    assert (ratsdf.LABEL_IGNORE, ratsdf.LABEL_LOW, ratsdf.LABEL_HIGH) == tuple(
        int(re.search(rf"#define RATSDF_LABEL_{n}\s+(\d+)", text).group(1)) for n in ("IGNORE", "LOW", "HIGH"))
    for m in ("label_set", "score_labels", "score_labels_device"):
        assert callable(getattr(ratsdf.Engine, m))


def test_hip_library_exports_the_entry_points():
    from ratsdf import _abi
    lib = _hip_lib()
    for s in _abi.SCORE_SYMBOLS:
        assert hasattr(lib.dll, "ratsdf_" + s), f"libratsdf.so does not export ratsdf_{s}"


def test_header_compiles_as_c_with_the_declared_sizes(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include "ratsdf_score.h"\n'
                   "typedef char info_is_48[sizeof(ratsdf_labelset_info) == 48 ? 1 : -1];\n"
                   "typedef char cell_at_16[offsetof(ratsdf_labelset_info, cell) == 16 ? 1 : -1];\n"
                   "typedef char origin_at_20[offsetof(ratsdf_labelset_info, origin) == 20 ? 1 : -1];\n"
                   "typedef char cells_at_32[offsetof(ratsdf_labelset_info, cells) == 32 ? 1 : -1];\n"
                   "typedef char params_are_32[sizeof(ratsdf_score_params) == 32 ? 1 : -1];\n"
                   "typedef char weight_at_12[offsetof(ratsdf_score_params, min_weight) == 12 ? 1 : -1];\n"
                   "typedef char reserved_at_20[offsetof(ratsdf_score_params, reserved) == 20 ? 1 : -1];\n"
                   "typedef char score_is_4160[sizeof(ratsdf_label_score) == 4160 ? 1 : -1];\n"
                   "typedef char confusion_at_32[offsetof(ratsdf_label_score, confusion) == 32 ? 1 : -1];\n"
                   "typedef char hist_at_64[offsetof(ratsdf_label_score, hist) == 64 ? 1 : -1];\n"
                   "typedef char label_is_8[sizeof(ratsdf_voxel_label) == 8 ? 1 : -1];\n"
                   "typedef char dist2_at_4[offsetof(ratsdf_voxel_label, dist2) == 4 ? 1 : -1];\n"
                   "int main(void) { ratsdf_label_score s; ratsdf_score_params p; (void)s; (void)p;\n"
                   "  return (void*)ratsdf_score_labels == (void*)ratsdf_score_labels_device; }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}", str(src), "-o",
                    str(tmp_path / "use.o")], check=True)


def test_binding_structures_are_as_declared():
    from ratsdf import _abi
    header = (ROOT / "include" / "ratsdf_score.h").read_text()
    ctype = {"float": C.c_float, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "int32_t": C.c_int32}
    for struct, binding in (("ratsdf_score_params", _abi.ScoreParams), ("ratsdf_labelset_info", _abi.LabelSetInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\}" % struct, header, flags=re.S).group(1)
        fields = re.findall(r"^\s*(float|uint32_t|int64_t|int32_t)\s+(\w+)(?:\[(\d)\])?;", body, flags=re.M)
        assert [n for _, n, _ in fields] == [n for n, _ in binding._fields_]
        assert [ctype[t] * int(k) if k else ctype[t] for t, _, k in fields] == [t for _, t in binding._fields_]
    assert C.sizeof(_abi.ScoreParams) == 32 and C.sizeof(_abi.LabelSetInfo) == 48
    d = _abi.LABEL_SCORE_DTYPE
    assert d.itemsize == 4160
    assert [d.fields[k][1] for k in d.names] == [0, 8, 16, 24, 32, 64]
    body = re.search(r"typedef struct ratsdf_label_score \{(.*?)\} ratsdf_label_score;", header, flags=re.S).group(1)
    names = re.findall(r"\b(\w+)(?:\[\d+\])*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == list(d.names)
    v = _abi.VOXEL_LABEL_DTYPE
    assert v.itemsize == 8 and [v.fields[k][1] for k in v.names] == [0, 4] and v.names == ("nearest", "dist2")


def test_oracle_reports_not_implemented(make_oracle):
    import ratsdf
    from ratsdf import _abi
    e = make_oracle(0.02, 0.12)
    for s in _abi.SCORE_SYMBOLS:
        assert not hasattr(e.lib.dll, "ratsdf_oracle_" + s)
    pts, lab = np.zeros((2, 3), np.float32), np.ones(2, np.uint8)
    fake = _abi.LabelSet(e.lib, C.c_void_p(0))
    for call in (lambda: e.label_set(pts, lab), lambda: e.score_labels(fake, max_dist=0.3),
                 lambda: e.score_labels(fake, max_dist=0.3, per_voxel=True),
                 lambda: e.score_labels_device(fake, 0, 0, 0, 0, max_dist=0.3), lambda: fake.info):
        with pytest.raises(ratsdf.RatsdfError) as ei:
            call()
        assert ei.value.status == 6


def test_calls_without_a_device_fail_with_a_status():
    """no engine handle can exist on a machine without a GPU: NULL handles are refused (RATSDF_ERR_BAD_ARGUMENT), and a
    refused call writes nothing"""
    from ratsdf import _abi
    lib = _hip_lib()
    pts, lab = np.zeros((4, 3), np.float32), np.ones(4, np.uint8)
    h = C.c_void_p(0x1234)
    assert lib.fn["labelset_create"](None, pts.ctypes.data, lab.ctypes.data, 4, 0.0, C.byref(h)) == 1
    assert lib.fn["labelset_create_device"](None, None, None, 0, 0.0, C.byref(h)) == 1
    assert h.value == 0x1234
    info = _abi.LabelSetInfo(points=-1)
    assert lib.fn["labelset_info_get"](None, C.byref(info)) == 1 and info.points == -1
    assert lib.fn["labelset_destroy"](None) == 1
    params = _abi.ScoreParams(0.1, 0.3, 0.5, 0, 0)
    out = np.full(520, -5, dtype=np.int64)
    p, n = C.c_void_p(0x1234), C.c_size_t(77)
    assert lib.fn["score_labels"](None, None, C.byref(params), out.ctypes.data, C.byref(p), C.byref(n)) == 1
    assert lib.fn["score_labels"](None, None, None, None, None, None) == 1
    assert p.value == 0x1234 and n.value == 77 and np.all(out == -5)
    count = np.full(1, -3, dtype=np.int64)
    assert lib.fn["score_labels_device"](None, None, C.byref(params), out.ctypes.data, None, 0, count.ctypes.data) == 1
    assert lib.fn["score_labels_device"](None, None, None, None, None, 0, None) == 1
    assert count[0] == -3 and np.all(out == -5)


def test_label_score_figures_curve_and_sum():
    from ratsdf import LABEL_SCORE_DTYPE, LabelScore
    r = np.zeros((), dtype=LABEL_SCORE_DTYPE)
    r["voxels"], r["selected"], r["unmatched"], r["unannotated"] = 1024, 40, 3, 7
    r["confusion"] = [6, 4, 2, 18]                          # TP, FP, FN, TN
    r["hist"][1, 200], r["hist"][1, 10], r["hist"][0, 130], r["hist"][0, 3] = 6, 2, 4, 18
    s = LabelScore(r)
    assert (s.voxels, s.selected, s.unmatched, s.unannotated, s.confusion) == (1024, 40, 3, 7, (6, 4, 2, 18))
    assert s.iou == 6 / (6 + 4 + 2 + 1e-15) and s.precision == 6 / (10 + 1e-15) and s.recall == 6 / (8 + 1e-15)
    assert s.accuracy == 24 / 30
    c = s.pr_curve()
    assert len(c["cutoff"]) == 256 and c["cutoff"][128] == 0.5
    assert (c["tp"][128], c["fp"][128], c["fn"][128], c["tn"][128]) == (6, 4, 2, 18)
    assert (c["tp"][0], c["fp"][0], c["fn"][0], c["tn"][0]) == (8, 22, 0, 0)
    assert (c["tp"][201], c["fp"][201], c["fn"][201], c["tn"][201]) == (0, 0, 8, 22)
    assert c["iou"][128] == s.iou and c["recall"][0] == 8 / (8 + 1e-15)
    both = s + s
    assert both.confusion == (12, 8, 4, 36) and both.voxels == 2048 and int(both.hist.sum()) == 60
    assert both == LabelScore(both.record) and both != s
    empty = LabelScore(np.zeros((), dtype=LABEL_SCORE_DTYPE))
    assert empty.iou == 0.0 and np.isnan(empty.accuracy)
