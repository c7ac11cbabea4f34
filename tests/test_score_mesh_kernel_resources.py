"""Compile-time resource guard for the kernels of the label score against a mesh (kernels_score_mesh.h; no GPU needed:
hipcc cross-compiles).

None may spill.  The values pinned here are the ones the cross-compile gives and DESIGN.md 4 "Label score against a
mesh" records.  The join holds a chunk of 256 forty-eight-byte triangle records (12 288 bytes), the 512 best keys of a
block's voxels (4 096), two run tables of 512 words (4 096), the scan's 32 words, its 520 counters and the list of
selected voxels (1 024) in LDS: 23 968 bytes with padding; its 101 registers give 4 waves per SIMD, one workgroup per
SIMD, so LDS does not limit it.  The build kernels keep 8 waves; the bounds pass holds its ten partial words in LDS, the
reference count its 64-bit sum."""
from test_kernel_resources import resource_usage

KERNELS = {"k_mesh_bounds": (40, 40, 8), "k_mesh_refs": (8, 40, 8), "k_mesh_cellsILb0EE": (0, 40, 8),
           "k_mesh_cellsILb1EE": (0, 40, 8), "k_score_mesh": (23968, 104, 4)}   # name: (LDS bytes, VGPRs, waves per SIMD)


def test_score_mesh_kernels_exist_do_not_spill_and_keep_their_occupancy():
    usage = resource_usage()
    for name, (lds, vgprs, waves) in KERNELS.items():
        plain = name.split("I")[0] if name.startswith("k_mesh_cells") else name
        tail = name[len(plain):] if plain != name else "E"
        found = [v for n, v in usage.items() if f"{len(plain)}{plain}{tail}" in n]
        assert len(found) == 1, (name, sorted(usage))
        res = found[0]
        assert res["ScratchSize"] == 0, f"{name}: {res}"
        assert res["Occupancy"] == waves, f"{name}: {res}"
        assert res["LDS"] == lds, f"{name}: {res}"
        assert res["VGPRs"] <= vgprs, f"{name}: {res}"
