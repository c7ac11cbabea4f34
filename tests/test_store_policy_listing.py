"""Which store instructions the shipped frame kernels use for the two bulk streams (no GPU needed: hipcc cross-compiles).

RATSDF_WT_STORES (ra-slam_amd/csrc/kernels_alloc.h) selects plain or write-through (`sc1`) stores for the voxel
update's three pool streams and for the candidate pass's texels.  The results are the same either way, so no parity
test notices when a refactor puts the other flavour back; this one reads the device listing (`make listing`, with line
information) and checks that the stores compiled from those source lines carry the flavour the default implies."""
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "ra-slam_amd" / "csrc"
KERNELS = {
    "k_integrate<2,false>": "_ZN6ratsdf11k_integrateILi2ELb0EEE",
    "k_integrate_g<2,false>": "_ZN6ratsdf13k_integrate_gILi2ELb0EEE",
    "k_front_g<false>": "_ZN6ratsdf9k_front_gILb0EEE",
}
STORE = re.compile(r"^\s*((?:global|buffer|flat)_store_dword(?:x[234])?)\b(.*)$")


def source_lines(name, needle, span=1):
    """1-based numbers of the lines of csrc/<name> that contain `needle` (and the span - 1 lines after each)"""
    out = set()
    for i, line in enumerate((CSRC / name).read_text().splitlines(), 1):
        if needle in line:
            out.update(range(i, i + span))
    assert out, f"{name}: no line contains {needle!r} (the test's markers need an update)"
    return out


@pytest.fixture(scope="session")
def listing():
    r = subprocess.run(["make", "-C", str(CSRC), "listing"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    text = (CSRC / "build" / "engine_g.s").read_text()
    files = {int(m.group(1)): m.group(2) for m in re.finditer(r'^\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]+)"', text, re.M)}
    kernels = {}
    for kname, sym in KERNELS.items():
        m = re.search(r"^" + re.escape(sym) + r"\w*:.*?\n(.*?)^\.Lfunc_end", text, re.S | re.M)
        assert m, f"{kname} is not in the listing"
        stores, loc = [], (None, 0)
        for line in m.group(1).splitlines():
            l = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", line)
            if l:
                loc = (files.get(int(l.group(1))), int(l.group(2)))
                continue
            s = STORE.match(line)
            if s:
                stores.append((loc[0], loc[1], s.group(1), "sc1" in s.group(2).split(";")[0].split()))
        kernels[kname] = stores
    return kernels


def default_flavour():
    m = re.search(r"^#define RATSDF_WT_STORES (\d+)", (CSRC / "kernels_alloc.h").read_text(), re.M)
    assert m
    return int(m.group(1))


def stores_from(stores, name, lines):
    return [(op, sc1) for f, l, op, sc1 in stores if f == name and l in lines]


@pytest.mark.parametrize("kernel", ["k_integrate<2,false>", "k_integrate_g<2,false>"])
def test_voxel_stores(listing, kernel):
    wt = bool(default_flavour() & 1)
    plain_at = source_lines("kernels_integrate.h", "reinterpret_cast<uint2*>(p)[0] = make_uint2(v[0], v[1]);")
    wt_at = source_lines("kernels_alloc.h", "__hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v0", 2)
    plain = stores_from(listing[kernel], "kernels_integrate.h", plain_at)
    through = stores_from(listing[kernel], "kernels_alloc.h", wt_at)
    want, other = (through, plain) if wt else (plain, through)
    assert other == [], f"{kernel}: voxel stores of the flavour the default does not select: {other}"
    # tsdf, probability, colour + weight: one 8-byte store per lane each
    assert len(want) == 3 and all(op.endswith("_store_dwordx2") and sc1 == wt for op, sc1 in want), (kernel, want)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_texel_stores(listing, kernel):
    wt = bool(default_flavour() & 2)
    plain_at = source_lines("kernels_cand.h", "J.texA[pix] = make_float4(d, r, ln, wn);") | \
        source_lines("kernels_cand.h", "J.texB[pix] = c;")
    wt_at = source_lines("kernels_alloc.h", "__builtin_amdgcn_raw_buffer_store_b128(", 3) | \
        source_lines("kernels_alloc.h", "__hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);")
    plain = stores_from(listing[kernel], "kernels_cand.h", plain_at)
    through = stores_from(listing[kernel], "kernels_alloc.h", wt_at)
    want, other = (through, plain) if wt else (plain, through)
    assert other == [], f"{kernel}: texel stores of the flavour the default does not select: {other}"
    # texA: 16 bytes per pixel, texB: 4
    assert sorted(op.split("_store_")[1] for op, _ in want) == ["dword", "dwordx4"], (kernel, want)
    assert all(sc1 == wt for _, sc1 in want), (kernel, want)
