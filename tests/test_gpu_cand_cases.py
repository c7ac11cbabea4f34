"""The candidate pass of the HIP engine (kernels_cand.h: cand_pixel_work under cand_inline_role, cand_pixels_role and
the share arithmetic of cand_shares.h) on the crafted frames of tests/cand_cases.py: the same frames go into a HIP engine
and an oracle engine through every entry point, and the maps are compared after every frame (after the batch, where
the frames go as one batch).  tests/test_cand_cases.py shows without a GPU that every case reaches what it is named for.

The bar is the project's (parity.py): frame statistics, directory, free list, weights and colours exact, tsdf and
probability within parity.TOL; the totals equal; no sticky error.  A block that a frame allocates and carves away in
the same frame (the far cases) is pinned by the free list's order and by deleted_blocks.

Entry points: integrate and integrate_device (the in-line form: no look-ahead), integrate_device_batch with
RATSDF_GRAPH 1 and 0 (frames after the first get their candidate pass from the look-ahead shares), and a Group of two
engines whose members get different scenes of one size (share A takes the whole pass there).

Observed on an MI355X: see DESIGN.md 4 "Crafted frames for the candidate pass".
"""
import numpy as np
import pytest

import cand_cases as cc
from parity import assert_maps_equal, assert_stats_equal

pytestmark = pytest.mark.gpu

SMALL = ([cc.ragged(W, H) for W, H in cc.RAGGED_SMALL] + [cc.steps_case(t) for t in cc.STEP_TRUNCS] +
         [cc.far_case(n) for n in cc.FAR])
# the ranks of a sharded map run in one test
SHARDED = ([[cc.shard_case(c, b, r) for r in range(c)] for c, b in cc.SHARDS] +
           [[cc.far_case(n, cc.sharded3(r)) for r in range(3)] for n in ("wrap1cm", "wrapx1cm")])
GROUPS = [[cc.ragged(W, H, v) for v in (0, 1)] for W, H in ((17, 5), (250, 157), (353, 97))] + \
         [[cc.steps_case(25, v) for v in (0, 1)]]
HD_GROUP = [cc.ragged(1000, 600, v) for v in (0, 1)]
names = lambda cs: cs.name if isinstance(cs, cc.Case) else cs[0].name.split("/")[0].replace("rank0", "") + "*"


def engines(cs, make_engine, make_oracle):
    return (make_engine(cs.vs, cs.trunc, **cs.engine_kw()),
            make_oracle(cs.vs, cs.trunc, threads=8 if cs.W * cs.H >= 500000 else 2, **cs.engine_kw()))


def check(gpu, cpu, what):
    gpu.synchronize()  # raises on a sticky error
    assert_stats_equal(gpu, cpu)
    worst = assert_maps_equal(gpu, cpu)
    st = cpu.last_frame_stats()
    print(f"{what}: allocated {st['allocated_blocks']}, deleted {st['deleted_blocks']}, updated voxels "
          f"{st['updated_voxels']}, active {st['active_blocks']}; worst tsdf difference {worst['tsdf']:.2e}, "
          f"probability {worst['prob']:.2e}")


def totals_equal(gpu, cpu):
    assert gpu.totals() == cpu.totals(), (gpu.totals(), cpu.totals())


def upload(cs):
    import torch
    dev = torch.device("cuda", 0)
    out = [{k: torch.from_numpy(np.array(getattr(fr, k))).to(dev) for k in ("rgb", "depth", "ht", "lt")}
           for fr in cs.frames]
    torch.cuda.synchronize()
    return out


def pointers(d):
    return (d["rgb"].data_ptr(), d["depth"].data_ptr(), d["ht"].data_ptr(), d["lt"].data_ptr())


def from_host(cs, make_engine, make_oracle):
    gpu, cpu = engines(cs, make_engine, make_oracle)
    for i, fr in enumerate(cs.frames):
        gpu.integrate(*fr.args())
        cpu.integrate(*fr.args())
        check(gpu, cpu, f"{cs.name}[integrate] frame {i}")
    totals_equal(gpu, cpu)


def from_device(cs, make_engine, make_oracle):
    gpu, cpu = engines(cs, make_engine, make_oracle)
    dev = upload(cs)
    for i, fr in enumerate(cs.frames):
        gpu.integrate_device(*pointers(dev[i]), cs.H, cs.W, fr.md, fr.intr, fr.pose)
        cpu.integrate(*fr.args())
        check(gpu, cpu, f"{cs.name}[integrate_device] frame {i}")
    totals_equal(gpu, cpu)


def batch_of(engine_or_group, cases, devs):
    """the frames of every member's case as one batch (devs: one upload per member)"""
    n, one = len(cases[0].frames), len(cases) == 1
    col = lambda j: [(pointers(devs[0][i])[j] if one else [pointers(d[i])[j] for d in devs]) for i in range(n)]
    per = lambda attr: [(getattr(cases[0].frames[i], attr) if one else [getattr(c.frames[i], attr) for c in cases])
                        for i in range(n)]
    c0 = cases[0]
    return engine_or_group.make_batch(col(0), col(1), col(2), col(3), c0.H, c0.W, c0.frames[0].md, per("intr"), per("pose"))


def as_a_batch(cs, graph, monkeypatch, make_engine, make_oracle, env=None):
    """env: further switches of the diagnostic build, read like RATSDF_GRAPH when the engine is created"""
    env = dict(env or {}, RATSDF_GRAPH=graph)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gpu, cpu = engines(cs, make_engine, make_oracle)
    for k in env:
        monkeypatch.delenv(k)
    dev = upload(cs)
    gpu.integrate_device_batch(batch_of(gpu, [cs], [dev]))
    for fr in cs.frames:
        cpu.integrate(*fr.args())
    check(gpu, cpu, f"{cs.name}[batch, {' '.join(f'{k}={v}' for k, v in sorted(env.items()))}]")
    totals_equal(gpu, cpu)


def as_a_group(cases, make_engine, make_oracle):
    import ratsdf
    pairs = [engines(cs, make_engine, make_oracle) for cs in cases]
    devs = [upload(cs) for cs in cases]
    group = ratsdf.Group([g for g, _ in pairs])
    try:
        group.integrate_device_batch(batch_of(group, cases, devs))
        group.synchronize()
        for (gpu, cpu), cs in zip(pairs, cases):
            for fr in cs.frames:
                cpu.integrate(*fr.args())
            check(gpu, cpu, f"{cs.name}[group of {len(cases)}]")
            totals_equal(gpu, cpu)
    finally:
        group.close()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", SMALL, ids=names)
def test_frames_from_host_memory(cs, make_engine, make_oracle):
    from_host(cs, make_engine, make_oracle)


@pytest.mark.parametrize("cs", SMALL, ids=names)
def test_frames_from_device_memory(cs, make_engine, make_oracle):
    from_device(cs, make_engine, make_oracle)


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("cs", SMALL, ids=names)
def test_frames_as_one_batch(cs, graph, monkeypatch, make_engine, make_oracle):
    """graph "1": one replay of a captured graph, "0": every frame launched by itself; either way the frames after the
    first get their candidate pass from the look-ahead shares of the frame before"""
    as_a_batch(cs, graph, monkeypatch, make_engine, make_oracle)


@pytest.mark.parametrize("ranks", SHARDED, ids=names)
def test_every_rank_of_a_sharded_map(ranks, monkeypatch, make_engine, make_oracle):
    """each rank through integrate, integrate_device and both batch forms"""
    for cs in ranks:
        from_host(cs, make_engine, make_oracle)
        from_device(cs, make_engine, make_oracle)
        for graph in ("1", "0"):
            as_a_batch(cs, graph, monkeypatch, make_engine, make_oracle)


@pytest.mark.parametrize("cases", GROUPS, ids=names)
def test_a_group_of_two_engines_with_different_scenes(cases, make_engine, make_oracle):
    as_a_group(cases, make_engine, make_oracle)


def test_a_group_of_the_two_wrap_cases(make_engine, make_oracle):
    """one member's samples wrap in z, the other's in x, in one launch"""
    as_a_group([cc.far_case("wrap1cm"), cc.far_case("wrapx1cm")], make_engine, make_oracle)


@pytest.mark.parametrize("name", [n for n in cc.FAR if n != "mixed"])
def test_blocks_carved_in_their_own_frame_are_named_by_the_directory_delta(name, make_engine, make_oracle):
    """In these cases every block a frame allocates is carved away by the same frame, so no dump shows where it was.
    The engine's log of deleted positions does (ratsdf_export_directory_delta_device).  Premise on the oracle: frame 0
    deletes what it allocates.  Then the logged positions are as many as the oracle deleted, and they are the restated
    samples' blocks that pass the frustum test, per directory bucket the first in raster order (a count that
    tests/test_cand_cases.py pins to the oracle's)."""
    import torch
    from ratsdf._abi import BLOCK_DTYPE
    cs = cc.far_case(name)
    gpu, cpu = engines(cs, make_engine, make_oracle)
    fr = cs.frames[0]
    cpu.integrate(*fr.args())
    st = cpu.last_frame_stats()
    assert st["allocated_blocks"] == st["deleted_blocks"] > 0 and st["active_blocks"] == 0
    dev = torch.device("cuda", 0)
    cap = 4096
    payload = torch.zeros(cap * 3, dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    gpu.export_directory_delta_device(0, 0, 0)  # the record starts with the first call
    gpu.integrate(*fr.args())
    gpu.export_directory_delta_device(payload.data_ptr(), cap, counts.data_ptr())
    gpu.synchronize()
    added, deleted = (int(v) for v in counts.cpu().numpy())
    rows = payload.cpu().numpy()[:(added + deleted) * 3].view(BLOCK_DTYPE)
    assert deleted == st["deleted_blocks"] and added + deleted <= cap, (added, deleted, st)
    gone = rows[added:]
    got = np.unique(cc.block_key(np.stack([gone["x"], gone["y"], gone["z"]], axis=1)))
    winners, distinct = cc.first_frame_winners(cs, fr)
    want = np.unique(cc.block_key(winners))
    print(f"{name}: the delta names {deleted} deleted positions ({added} added); the restatement has {distinct} blocks "
          f"in {len(want)} buckets")
    assert len(got) == deleted and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# the ragged sizes around 600 000 pixels: once per entry point
@pytest.mark.parametrize("size", cc.RAGGED_HD, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hd_frames_from_host_memory(size, make_engine, make_oracle):
    from_host(cc.ragged(*size), make_engine, make_oracle)


@pytest.mark.parametrize("size", cc.RAGGED_HD, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hd_frames_from_device_memory(size, make_engine, make_oracle):
    from_device(cc.ragged(*size), make_engine, make_oracle)


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("size", cc.RAGGED_HD, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hd_frames_as_one_batch(size, graph, monkeypatch, make_engine, make_oracle):
    """1000x600 and 1001x601: the whole look-ahead pass is share A's, and the last 10 of the 2394 super-tiles do not
    fill a group of 16; the last frame has depth only there"""
    as_a_batch(cc.ragged(*size), graph, monkeypatch, make_engine, make_oracle)


def test_hd_group_of_two_engines_with_different_scenes(make_engine, make_oracle):
    as_a_group(HD_GROUP, make_engine, make_oracle)
