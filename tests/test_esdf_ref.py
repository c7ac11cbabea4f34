"""The ESDF (include/ratsdf_esdf.h) without a GPU: the restatement (tests/esdf_ref.py) against the O(n^2) definition,
the library's exports, the oracle's not-implemented status, and ratsdf.h staying free of the new symbols."""
import re
from pathlib import Path

import numpy as np
import pytest

import esdf_ref as ref

ROOT = Path(__file__).resolve().parent.parent
SYMS = ("ratsdf_esdf", "ratsdf_esdf_device")


def _masks():
    rng = np.random.default_rng(21)
    yield np.zeros((5, 6, 7), dtype=bool)                      # empty O
    yield np.ones((4, 3, 5), dtype=bool)                       # all obstacles: box \ O empty
    for p in (0.01, 0.1, 0.5, 0.9):
        yield rng.random((9, 7, 11)) < p
    yield rng.random((1, 13, 17)) < 0.05                       # dims of 1 on an axis
    yield rng.random((12, 1, 9)) < 0.05
    yield rng.random((10, 8, 1)) < 0.05
    yield rng.random((1, 1, 40)) < 0.1                         # thin 1 x 1 x n lines, each axis
    yield rng.random((1, 40, 1)) < 0.1
    yield rng.random((40, 1, 1)) < 0.1
    yield np.ones((1, 1, 1), dtype=bool)
    yield np.zeros((1, 1, 1), dtype=bool)
    one = np.zeros((7, 9, 11), dtype=bool)
    one[3, 0, 10] = True
    yield one


def test_restatement_matches_the_definition():
    for o in _masks():
        for vs in (0.01, 0.005):
            a = ref.field(o, vs)
            b = ref.field(o, vs, d2_fn=ref.brute_d2)
            assert ref.same_bytes(a, b), o.shape
            assert np.all(np.signbit(a) == o)
            assert np.all((a == 0) == False)  # noqa: E712 -- no voxel sits at distance 0


def test_states_and_flags():
    rng = np.random.default_rng(22)
    state = rng.integers(0, 3, size=(6, 7, 8)).astype(np.uint8)
    a = ref.esdf(state, 0.01)
    b = ref.esdf(state, 0.01, unknown_occupied=True)
    assert np.all(np.signbit(a) == (state == ref.OCCUPIED))
    assert np.all(np.signbit(b) == (state != ref.FREE))
    # a single obstacle: the field is exactly sqrtf(i^2 + j^2 + k^2) * vs
    o = np.zeros((5, 6, 7), dtype=bool)
    o[2, 3, 4] = True
    z, y, x = np.meshgrid(np.arange(5), np.arange(6), np.arange(7), indexing="ij")
    want = np.sqrt(((x - 4) ** 2 + (y - 3) ** 2 + (z - 2) ** 2).astype(np.float32)) * np.float32(0.02)
    want[2, 3, 4] = -(np.sqrt(np.float32(1)) * np.float32(0.02))
    assert ref.same_bytes(ref.field(o, 0.02), want)


def test_hip_library_exports_the_esdf_entry_points():
    import ratsdf
    if not ratsdf.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = ratsdf.library()
    for s in SYMS:
        assert hasattr(lib.dll, s), f"libratsdf.so does not export {s}"
    assert sorted("ratsdf_" + s for s in ratsdf._abi.ESDF_SYMBOLS) == sorted(SYMS)
    text = (ROOT / "include" / "ratsdf_esdf.h").read_text()
    for s in SYMS:
        assert s + "(" in text


def test_ratsdf_h_does_not_declare_them():
    import ratsdf
    text = (ROOT / "include" / "ratsdf.h").read_text()
    for s in SYMS:
        assert not re.search(r"\b" + s + r"\s*\(", text)
    assert not set(ratsdf._abi.ESDF_SYMBOLS) & set(ratsdf._abi.SYMBOLS)


def test_oracle_reports_not_implemented(make_oracle):
    import ratsdf
    e = make_oracle(0.01, 0.06)
    with pytest.raises(ratsdf.RatsdfError) as ei:
        e.esdf([0, 0, 0], [8, 8, 8])
    assert ei.value.status == 6
    with pytest.raises(ratsdf.RatsdfError) as ei:
        e.esdf_device([0, 0, 0], [8, 8, 8], 0)
    assert ei.value.status == 6
    with pytest.raises(ValueError):
        e.esdf([0, 0], [8, 8, 8])


def test_voxel_box():
    from ratsdf import voxel_box
    vs = 0.01
    o, d = voxel_box([-0.105, 0.0, 0.3], [0.2, 0.0, 0.3], vs)
    lo = np.floor(np.array([-0.105, 0.0, 0.3], dtype=np.float32) / np.float32(vs)).astype(int)
    hi = np.floor(np.array([0.2, 0.0, 0.3], dtype=np.float32) / np.float32(vs)).astype(int)
    assert o == list(lo) and d == list(hi - lo + 1)
    assert d[1] == 1 and d[2] == 1
    with pytest.raises(ValueError):
        voxel_box([0, 0, 0], [-1, 0, 0], vs)
    with pytest.raises(ValueError):
        voxel_box([np.nan, 0, 0], [1, 1, 1], vs)
