"""The store flavours of the two bulk streams (RATSDF_WT_STORES, ra-slam_amd/csrc/kernels_alloc.h): the voxel update's
three pool streams and the candidate pass's texels may leave L2 as write-through stores, and a wave of the update may
store whole lines.  Whatever flavour the library was built with, memory must hold the same bytes, and a later launch
on the same stream must see every one of them.  The cases are the ones in which the flavours differ in what a wave
does: waves in which only some lanes store (holes, image edges), fresh blocks (every lane stores) and their carving,
the probability stream that is first not stored and then stored, reads on the same engine without a synchronise in
between, and a group.  160x120 frames; 2 cm voxels unless noted."""
import numpy as np
import pytest
import torch

from parity import assert_heap_equal, assert_maps_equal, assert_stats_equal
from ratsdf import synthetic

pytestmark = pytest.mark.gpu

VS, MD = 0.02, 4.0


def upload(frames):
    dev = torch.device("cuda", 0)
    out = [{k: torch.from_numpy(f[k]).to(dev) for k in ("rgb", "depth", "ht", "lt")} for f in frames]
    torch.cuda.synchronize()
    return out


def device_batch(gpu, frames, dev, sem=None):
    """the frames as one device batch; sem[i] False makes frame i TSDF-only (NULL ht / lt)"""
    n = len(frames)
    sem = [True] * n if sem is None else sem
    h, w = frames[0]["depth"].shape
    ptr = lambda key, on: [dev[i][key].data_ptr() if on[i] else None for i in range(n)]
    return gpu.make_batch(ptr("rgb", [True] * n), ptr("depth", [True] * n), ptr("ht", sem), ptr("lt", sem), h, w, MD,
                          [f["intrinsics"] for f in frames], [f["pose"] for f in frames])


def oracle_frames(cpu, frames, sem=None):
    for i, f in enumerate(frames):
        on = sem is None or sem[i]
        cpu.integrate(f["rgb"], f["depth"], f["ht"] if on else None, f["lt"] if on else None, MD, f["intrinsics"],
                      f["pose"])


@pytest.mark.parametrize("graph", ["1", "0"])
def test_partial_lane_stores(graph, monkeypatch, make_engine, make_oracle):
    """8 noisy frames with holes: at the holes and the image's edges only some lanes of a wave store.  As one device
    batch (graph replay, or its plain launch loop) and frame by frame; all three against the oracle."""
    monkeypatch.setenv("RATSDF_GRAPH", graph)
    batch = make_engine(VS, 6 * VS)
    monkeypatch.delenv("RATSDF_GRAPH")
    single, cpu = make_engine(VS, 6 * VS), make_oracle(VS, 6 * VS)
    frames = synthetic.stream("room", 8, scale=0.25, noise=True, holes=True)
    dev = upload(frames)
    batch.integrate_device_batch(device_batch(batch, frames, dev))
    h, w = frames[0]["depth"].shape
    for f, d in zip(frames, dev):
        single.integrate_device(d["rgb"].data_ptr(), d["depth"].data_ptr(), d["ht"].data_ptr(), d["lt"].data_ptr(),
                                h, w, MD, f["intrinsics"], f["pose"])
    oracle_frames(cpu, frames)
    for gpu in (batch, single):
        assert_stats_equal(gpu, cpu)
        assert_maps_equal(gpu, cpu)


def test_fresh_blocks_then_carving(make_engine, make_oracle):
    """the first frame of a view (every block new: all 64 lanes of every wave store, the probability included), then a
    frame from behind the surface's free side that carves some of them; the pool's free list after each"""
    gpu, cpu = make_engine(VS, 6 * VS), make_oracle(VS, 6 * VS)
    first = synthetic.frame("room", 0, scale=0.25)
    # the same view with the surface pushed back: the blocks in front of it now lie in free space
    carve = dict(first)
    carve["depth"] = np.where(first["depth"] > 0, np.minimum(first["depth"] + 0.4, MD - 0.05), 0).astype(np.float32)
    deleted = 0
    for f in (first, carve, carve):
        for e in (gpu, cpu):
            e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], MD, f["intrinsics"], f["pose"])
        assert_stats_equal(gpu, cpu)
        assert_heap_equal(gpu, cpu)
        assert_maps_equal(gpu, cpu)
        deleted += cpu.last_frame_stats()["deleted_blocks"]
    assert deleted > 0, "the case carves nothing"


def test_probability_unstored_then_stored(make_engine, make_oracle):
    """three TSDF-only frames (existing blocks' probability neither loaded nor stored), then three semantic ones (it
    is), in one batch and across batches"""
    for split in (None, 3):
        gpu, cpu = make_engine(VS, 6 * VS), make_oracle(VS, 6 * VS)
        frames = synthetic.stream("room", 6, scale=0.25, noise=True, holes=True)
        sem = [False] * 3 + [True] * 3
        dev = upload(frames)
        parts = [(0, 6)] if split is None else [(0, split), (split, 6)]
        for lo, hi in parts:
            gpu.integrate_device_batch(device_batch(gpu, frames[lo:hi], dev[lo:hi], sem[lo:hi]))
            oracle_frames(cpu, frames[lo:hi], sem[lo:hi])
            assert_stats_equal(gpu, cpu)
            assert_maps_equal(gpu, cpu)


def test_same_engine_reads_see_every_store(make_engine, make_oracle):
    """5 mm voxels: one view integrated four times in one batch (every block updated in four consecutive frames), then
    dump_voxels, sample_points and a 160x120 ray cast on the same engine with no synchronise in between.  The same
    three reads after a synchronise must return the same bytes, and the map must be the oracle's."""
    vs = 0.005
    gpu, cpu = make_engine(vs, 6 * vs), make_oracle(vs, 6 * vs)
    f = synthetic.frame("room", 0, scale=0.25, noise=True, holes=True)
    frames = [f] * 4
    dev = upload(frames)
    h, w = f["depth"].shape
    rng = np.random.default_rng(7)
    gpu.integrate_device_batch(device_batch(gpu, frames, dev))

    def reads():
        _, blocks = gpu.dump_directory()
        idx = blocks["idx"][:: max(1, len(blocks) // 64)]
        t, c, p = gpu.dump_voxels(idx)
        sel = blocks[:: max(1, len(blocks) // 64)]
        centres = (np.stack([sel["x"], sel["y"], sel["z"]], 1).astype(np.float32) * 8 + 3.5) * np.float32(vs)
        pts = centres + rng_offsets
        s = gpu.sample_points(pts.astype(np.float32))
        rgba, normal = gpu.raycast(f["intrinsics"], h, w, f["pose"], MD)
        return [t.tobytes(), c.tobytes(), p.tobytes(), s.tobytes(), rgba.tobytes(), normal.tobytes()]

    _, blocks0 = gpu.dump_directory()
    rng_offsets = rng.uniform(-1.5 * vs, 1.5 * vs, (len(blocks0[:: max(1, len(blocks0) // 64)]), 3)).astype(np.float32)
    before = reads()
    gpu.synchronize()
    after = reads()
    for name, a, b in zip(("tsdf", "rgbw", "probability", "samples", "rgba", "normal"), before, after):
        assert a == b, f"{name}: a read behind the batch differs from the same read after a synchronise"
    assert np.frombuffer(before[4], np.uint8).any(), "the ray cast hit nothing"
    oracle_frames(cpu, frames)
    assert_stats_equal(gpu, cpu)
    assert_maps_equal(gpu, cpu)


def test_group_of_two(make_engine, make_oracle):
    """two members through ratsdf_group_*: two batches, each member against its own oracle"""
    import ratsdf
    streams = [synthetic.stream(sc, 5, scale=0.25, noise=True, holes=True) for sc in ("room", "sphere")]
    devs = [upload(fr) for fr in streams]
    engines = [make_engine(VS, 6 * VS) for _ in streams]
    oracles = [make_oracle(VS, 6 * VS) for _ in streams]
    group = ratsdf.Group(engines)
    h, w = streams[0][0]["depth"].shape
    for lo, hi in ((0, 2), (2, 5)):
        rows = lambda key: [[devs[s][i][key].data_ptr() for s in range(2)] for i in range(lo, hi)]
        group.integrate_device_batch(group.make_batch(
            rows("rgb"), rows("depth"), rows("ht"), rows("lt"), h, w, MD,
            [[streams[s][i]["intrinsics"] for s in range(2)] for i in range(lo, hi)],
            [[streams[s][i]["pose"] for s in range(2)] for i in range(lo, hi)]))
        for s in range(2):
            oracle_frames(oracles[s], streams[s][lo:hi])
            assert_stats_equal(engines[s], oracles[s])
            assert_maps_equal(engines[s], oracles[s])
    group.close()
