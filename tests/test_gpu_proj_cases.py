"""The projection at the head of the frame update and the visibility test of the HIP engine (integrate_block in
kernels_integrate.h, block_visible<false> in device_math.h / kernels_visible.h) on the crafted poses, intrinsics and
image borders of tests/proj_cases.py: the same blocks go into a HIP engine and an oracle engine with import_blocks, the
same frames follow, and the maps are compared after every frame (after the batch, where the frames go as one batch).
tests/test_proj_cases.py shows without a GPU that the cases reach what they are named for and that the oracle does what
the numpy restatement says.

The bars are those of tests/test_gpu_update_cases.py, whose helpers do the comparing: live block positions and the frame
statistics equal; weight and colour exact (most imported voxels have weight 0, so their colour after a frame IS the
picked pixel); tsdf bit for bit wherever the oracle's is zero or normal, within parity.TOL where it is subnormal; the
probability within parity.TOL with NaN in the same voxels; a voxel that a frame does not update keeps all three words
bit for bit.

Observed on an MI355X (printed by the tests): see DESIGN.md 4 "Frames under crafted poses, intrinsics and borders".
"""
import numpy as np
import pytest

import proj_cases as pc
from test_gpu_update_cases import after_the_batch, frame_by_frame, import_case, pointers, upload

pytestmark = pytest.mark.gpu


def engines_of(cs, make_engine, make_oracle):
    gpu, cpu = make_engine(cs.vs, cs.trunc, **pc.CFG), make_oracle(cs.vs, cs.trunc, threads=4, **pc.CFG)
    import_case((gpu, cpu), cs)
    return gpu, cpu


def reached(cs):
    """what the case's frames reach, for the printed figures"""
    out = []
    for fr in cs.frames:
        H, W = fr.shape
        pr = pc.predict(cs.blocks[0], fr)
        out.append(f"{int((pr.upd & (pc.exact_halves(pr.proj.qu) | pc.exact_halves(pr.proj.qv))).sum())} updating voxels "
                   f"on exact halves, {pc.mixed_pairs(pr.proj)} mixed pairs, {int((pr.upd & (pr.proj.pcz < 0)).sum())} "
                   f"updates behind the camera, {int((~pr.vis).sum())} blocks not visible")
    return "; ".join(f"frame {i}: {t}" for i, t in enumerate(out))


def summary(what, cs, figures):
    print(f"{what}: worst tsdf difference {max(f['tsdf'] for f in figures):.3e}, worst probability difference "
          f"{max(f['prob'] for f in figures):.3e}; {reached(cs)}")


@pytest.mark.parametrize("fam,fn,a", pc.ALL, ids=pc.IDS)
def test_frames_from_host_memory(fam, fn, a, make_engine, make_oracle):
    cs = fn(*a)
    gpu, cpu = engines_of(cs, make_engine, make_oracle)
    figures = frame_by_frame(gpu, cpu, cs, lambda i, fr: gpu.integrate(*fr.args()), f"{cs.name}[integrate]", pc)
    summary(f"{cs.name}[integrate]", cs, figures)


@pytest.mark.parametrize("fam,fn,a", pc.ALL, ids=pc.IDS)
def test_frames_from_device_memory(fam, fn, a, make_engine, make_oracle):
    cs = fn(*a)
    gpu, cpu = engines_of(cs, make_engine, make_oracle)
    dev = upload(cs)

    def send(i, fr):
        H, W = fr.shape
        gpu.integrate_device(*pointers(dev[i]), H, W, fr.md, fr.intr, fr.pose)
    figures = frame_by_frame(gpu, cpu, cs, send, f"{cs.name}[integrate_device]", pc)
    summary(f"{cs.name}[integrate_device]", cs, figures)


def batch_of(engine_or_group, cases, devs):
    """the frames of every member's case as one batch, each frame with its own intrinsics and pose (cases / devs: one
    per member; a single engine: lists of one)"""
    one = len(cases) == 1 and not hasattr(engine_or_group, "engines")
    n = len(cases[0].frames)
    H, W = cases[0].frames[0].shape
    assert all(len(cs.frames) == n and all(fr.shape == (H, W) for fr in cs.frames) for cs in cases)
    ptr = [[pointers(d[i]) for d in devs] for i in range(n)]
    col = lambda j: [(r[0][j] if one else [m[j] for m in r]) for r in ptr]
    per = lambda get: [(get(cases[0].frames[i]) if one else [get(cs.frames[i]) for cs in cases]) for i in range(n)]
    return engine_or_group.make_batch(col(0), col(1), col(2), col(3), H, W, cases[0].frames[0].md,
                                      per(lambda fr: fr.intr), per(lambda fr: fr.pose))


@pytest.mark.parametrize("graph", ["1", "0"])
def test_a_batch_of_three_cameras_over_one_map(graph, monkeypatch, make_engine, make_oracle):
    """halves under the third of a turn, plane b and an oblique camera as ONE batch over one imported map: every frame
    carries its own pose and intrinsics; graph "1": one replay of a captured graph, "0": every frame by itself"""
    cs = pc.batch_case()
    assert len({fr.pose for fr in cs.frames}) == 3 and len({fr.intr for fr in cs.frames}) == 3
    monkeypatch.setenv("RATSDF_GRAPH", graph)
    gpu, cpu = make_engine(cs.vs, cs.trunc, **pc.CFG), make_oracle(cs.vs, cs.trunc, threads=4, **pc.CFG)
    monkeypatch.delenv("RATSDF_GRAPH")
    import_case((gpu, cpu), cs)
    dev = upload(cs)
    gpu.integrate_device_batch(batch_of(gpu, [cs], [dev]))
    figures = after_the_batch(gpu, cpu, cs, f"batch[RATSDF_GRAPH={graph}]", pc)
    summary(f"batch[RATSDF_GRAPH={graph}]", cs, [figures])


def test_a_group_of_two_engines_under_different_poses(make_engine, make_oracle):
    """plane b and the v = 0 border case (a group's members share the voxel size: 2^-6 m) as the two members of a group:
    every frame of the batch has another pose and other intrinsics per member"""
    import ratsdf
    cases = [pc.plane("b"), pc.borders("v0", False)]
    assert all(a.pose != b.pose and a.intr != b.intr for a, b in zip(cases[0].frames, cases[1].frames))
    pairs = [engines_of(cs, make_engine, make_oracle) for cs in cases]
    devs = [upload(cs) for cs in cases]
    group = ratsdf.Group([g for g, _ in pairs])
    try:
        group.integrate_device_batch(batch_of(group, cases, devs))
        group.synchronize()
        for (g, o), cs in zip(pairs, cases):
            figures = after_the_batch(g, o, cs, f"{cs.name}[group of two]", pc)
            summary(f"{cs.name}[group of two]", cs, [figures])
    finally:
        group.close()


def other_voxels_per_lane(make_engine, make_oracle, families=("halves", "plane", "far")):
    """the halves, plane and far families frame by frame (tests/diagnostic_build_cases.py: RATSDF_VPL=1 and 4, the scalar
    loop with f2i(roundf()) and, at four voxels per lane, its one guard over four divisors)"""
    for fam in families:
        for cs in pc.family(fam):
            gpu, cpu = engines_of(cs, make_engine, make_oracle)
            frame_by_frame(gpu, cpu, cs, lambda i, fr: gpu.integrate(*fr.args()), f"{cs.name}[scalar loop]", pc)
