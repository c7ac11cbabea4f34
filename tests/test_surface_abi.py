"""The surface-point entry points in the library, the binding and the header (no GPU needed)."""
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def test_surface_symbols_equal_the_header_and_the_library_exports_them():
    import ratsdf
    from ratsdf import _abi
    header = (ROOT / "include" / "ratsdf_surface.h").read_text()
    declared = re.findall(r"^int ratsdf_(\w+)\(", header, flags=re.M)
    assert declared == _abi.SURFACE_SYMBOLS
    assert not set(_abi.SURFACE_SYMBOLS) & set(_abi.SYMBOLS)           # ratsdf.h's table stays ratsdf.h's
    lib = ratsdf.library()
    for s in _abi.SURFACE_SYMBOLS:
        assert hasattr(lib.dll, "ratsdf_" + s), s


def test_oracle_reports_not_implemented(make_oracle):
    import ratsdf
    from ratsdf import _abi
    e = make_oracle(0.02, 0.12)
    for s in _abi.SURFACE_SYMBOLS:
        assert not hasattr(e.lib.dll, "ratsdf_oracle_" + s)
    for call in (lambda: e.surface_points([0, 0, 0], [8, 8, 8]),
                 lambda: e.surface_points_device([0, 0, 0], [8, 8, 8], 0, 0, 0)):
        try:
            call()
            raise AssertionError("the oracle has no surface points")
        except ratsdf.RatsdfError as err:
            assert err.status == 6


def test_record_layout():
    from ratsdf import _abi
    d = _abi.SURFACE_DTYPE
    assert d.itemsize == 32 and [d.fields[k][1] for k in ("pos", "normal", "prob", "rgbw")] == [0, 12, 24, 28]
    assert np.dtype(_abi.SurfaceParams).itemsize == 16
