"""The point-sampling ABI (include/ratsdf_sample.h) without a GPU: exports, the record's layout against the binding's
SAMPLE_DTYPE, and the oracle's not-implemented status."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMS = ("ratsdf_sample_points", "ratsdf_sample_points_device")


def test_hip_library_exports_the_sampling_entry_points():
    import ratsdf
    if not ratsdf.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = ratsdf.library()
    for s in SYMS:
        assert hasattr(lib.dll, s), f"libratsdf.so does not export {s}"
    assert sorted("ratsdf_" + s for s in ratsdf._abi.SAMPLE_SYMBOLS) == sorted(SYMS)
    text = (ROOT / "include" / "ratsdf_sample.h").read_text()
    for s in SYMS:
        assert s + "(" in text


def test_record_layout_matches_the_dtype(tmp_path):
    from ratsdf._abi import SAMPLE_ALLOCATED, SAMPLE_DTYPE, SAMPLE_NEAREST, SAMPLE_OBSERVED
    src = tmp_path / "layout.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "ratsdf_sample.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(ratsdf_sample), offsetof(ratsdf_sample, tsdf),
         offsetof(ratsdf_sample, grad), offsetof(ratsdf_sample, prob), offsetof(ratsdf_sample, rgbw),
         offsetof(ratsdf_sample, min_weight), offsetof(ratsdf_sample, flags), offsetof(ratsdf_sample, reserved),
         RATSDF_SAMPLE_ALLOCATED, RATSDF_SAMPLE_OBSERVED, RATSDF_SAMPLE_NEAREST);
  return 0;
}
''')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    f = SAMPLE_DTYPE.fields
    want = [SAMPLE_DTYPE.itemsize] + [f[k][1] for k in ("tsdf", "grad", "prob", "rgbw", "min_weight", "flags",
                                                          "reserved")] + [SAMPLE_ALLOCATED, SAMPLE_OBSERVED,
                                                                          SAMPLE_NEAREST]
    assert got == want
    assert got[0] == 32


def test_oracle_reports_not_implemented(make_oracle):
    import ratsdf
    from ratsdf._abi import SAMPLE_DTYPE
    e = make_oracle(0.01, 0.06)
    with pytest.raises(ratsdf.RatsdfError) as ei:
        e.sample_points(np.zeros((5, 3), dtype=np.float32))
    assert ei.value.status == 6
    with pytest.raises(ratsdf.RatsdfError) as ei:
        e.sample_points_device(0, 0, 0)
    assert ei.value.status == 6
    with pytest.raises(ValueError):
        e.sample_points(np.zeros((5, 2), dtype=np.float32))
    assert SAMPLE_DTYPE.itemsize == 32
