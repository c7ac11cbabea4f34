"""Batches that mix frames with semantics and TSDF-only frames, on every batch entry point of the HIP engine.

Semantics are decided frame by frame (modules/tsdf_module.cc:27-31): a NULL entry in a batch's ht / lt tables makes
that one frame TSDF-only.  Inside a batch the candidate pass of frame i+1 rides in frame i's launches, the update skips
the probability while no frame has had semantics (FrameParams::segm_live), host frames share a 16-slot staging ring
whose ht / lt bytes outlive the frame that wrote them, and a group steps several members whose patterns differ.
Every call is compared with the frame-by-frame oracle: directory, free list, voxels, frame statistics and totals.
The patterns are in tests/mixed_cases.py; tests/test_mixed_semantics.py checks that each of them tells the plausible
wrong patterns apart."""
import numpy as np
import pytest
import torch

from mixed_cases import (GRAPH_REPLAY, GROUP, PATTERNS, apply, oracle_run, pinned_pattern, semantic_frames,
                         staging_pattern)
from parity import assert_maps_equal, assert_stats_equal

pytestmark = pytest.mark.gpu

VS, MD = 0.02, 4.0


def upload(frames):
    """every frame's four images in HBM (ht / lt too: the pattern decides which pointers a batch passes)"""
    dev = torch.device("cuda", 0)
    out = [{k: torch.from_numpy(f[k]).to(dev) for k in ("rgb", "depth", "ht", "lt")} for f in frames]
    torch.cuda.synchronize()
    return out


def device_batch(gpu, frames, dev, pattern, lo):
    """frames lo .. lo+len(pattern)-1 as one ratsdf_integrate_device_batch, NULL ht / lt where the pattern says so"""
    idx = range(lo, lo + len(pattern))
    h, w = frames[lo]["depth"].shape
    ht = [dev[i]["ht"].data_ptr() if k in "SH" else None for i, k in zip(idx, pattern)]
    lt = [dev[i]["lt"].data_ptr() if k == "S" else None for i, k in zip(idx, pattern)]
    return gpu.make_batch([dev[i]["rgb"].data_ptr() for i in idx], [dev[i]["depth"].data_ptr() for i in idx], ht, lt,
                          h, w, MD, [frames[i]["intrinsics"] for i in idx], [frames[i]["pose"] for i in idx])


def check(gpu, cpu):
    assert_maps_equal(gpu, cpu)
    assert_stats_equal(gpu, cpu)
    assert gpu.totals() == cpu.totals(), (gpu.totals(), cpu.totals())


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_device_batch(pattern, graph, monkeypatch, make_engine, make_oracle):
    """one batch on a fresh map (NNNSSN: the first semantic frame arrives mid-batch, segm_live flips inside one launch
    sequence; NSSN: frame 0's candidates come from the graph's own k_cand_g, frame 1's from the look-ahead), then the
    same pattern again on the live map"""
    monkeypatch.setenv("RATSDF_GRAPH", graph)
    gpu, cpu = make_engine(VS, 6 * VS), make_oracle(VS, 6 * VS)
    monkeypatch.delenv("RATSDF_GRAPH")
    n = len(pattern)
    frames = semantic_frames("room", 2 * n)
    dev = upload(frames)
    for lo in (0, n):
        gpu.integrate_device_batch(device_batch(gpu, frames, dev, pattern, lo))
        oracle_run(cpu, apply(frames[lo:lo + n], pattern), MD)
        check(gpu, cpu)


@pytest.mark.parametrize("graph", ["1", "0"])
def test_device_batches_of_different_patterns_on_one_engine(graph, monkeypatch, make_engine, make_oracle):
    """three 4-frame batches back to back: with graphs, ONE graph captured for (H, W, 4) replays all three, and each
    frame's semantics must come from the replay's job table, not from the capture"""
    monkeypatch.setenv("RATSDF_GRAPH", graph)
    gpu, cpu = make_engine(VS, 6 * VS), make_oracle(VS, 6 * VS)
    monkeypatch.delenv("RATSDF_GRAPH")
    frames = semantic_frames("room", 4 * len(GRAPH_REPLAY))
    dev = upload(frames)
    for b, pattern in enumerate(GRAPH_REPLAY):
        gpu.integrate_device_batch(device_batch(gpu, frames, dev, pattern, 4 * b))
        oracle_run(cpu, apply(frames[4 * b:4 * b + 4], pattern), MD)
        check(gpu, cpu)


def test_device_batch_640x480(make_engine, make_oracle):
    """the production launch geometry: 640x480 frames, 5 mm voxels, S N S N"""
    vs = 0.005
    gpu, cpu = make_engine(vs, 6 * vs), make_oracle(vs, 6 * vs, threads=16)
    frames = semantic_frames("room", 4, scale=1.0)
    dev = upload(frames)
    gpu.integrate_device_batch(device_batch(gpu, frames, dev, "SNSN", 0))
    oracle_run(cpu, apply(frames, "SNSN"), MD)
    check(gpu, cpu)


def test_host_batch_through_the_staging_ring(make_engine, make_oracle):
    """ratsdf_integrate_batch from ordinary host memory: 40 frames in one call (the 16-slot ring wraps twice), then a
    call that starts in the middle of the ring"""
    gpu, cpu = make_engine(VS, 6 * VS), make_oracle(VS, 6 * VS)
    frames = semantic_frames("room", 51)
    pattern = staging_pattern(51)
    mixed = apply(frames, pattern)
    for lo, hi in ((0, 40), (40, 51)):
        gpu.integrate_batch(mixed[lo:hi], MD)
        oracle_run(cpu, mixed[lo:hi], MD)
        check(gpu, cpu)


def test_pinned_host_batch_breaks_runs_at_tsdf_only_frames(make_engine, make_oracle):
    """ratsdf_integrate_batch(pinned) on side-by-side blocks of one host_alloc arena, every third frame TSDF-only:
    those frames break the runs that go up in one copy, and the frames after them must still land in their own slots.
    A TSDF-only frame's block holds other images in its ht / lt place (1 - ht, ht), which nothing may read."""
    gpu, cpu = make_engine(VS, 6 * VS), make_oracle(VS, 6 * VS)
    n = 40
    frames = semantic_frames("room", n)
    pattern = pinned_pattern(n)
    h, w = frames[0]["depth"].shape
    npx = h * w
    arena = gpu.host_alloc((n * npx * 16,), np.uint8)
    blocks = []
    for i, (f, k) in enumerate(zip(frames, pattern)):
        blk = arena[i * npx * 16:(i + 1) * npx * 16]
        g = dict(f)
        g["depth"] = blk[:npx * 4].view(np.float32).reshape(h, w)
        g["ht"] = blk[npx * 4:npx * 8].view(np.float32).reshape(h, w)
        g["lt"] = blk[npx * 8:npx * 12].view(np.float32).reshape(h, w)
        g["rgb"] = blk[npx * 12:npx * 15].reshape(h, w, 3)
        for key in ("rgb", "depth", "ht", "lt"):
            g[key][...] = f[key]
        if k != "S":
            g["ht"][...], g["lt"][...] = f["lt"], f["ht"]
        blocks.append(g)
    pinned = apply(blocks, pattern)
    gpu.integrate_batch(pinned, MD, pinned=True)
    oracle_run(cpu, apply(frames, pattern), MD)
    check(gpu, cpu)
    # the same blocks again from a call that starts at another slot of the ring
    gpu.integrate_batch(pinned[:20], MD, pinned=True)
    oracle_run(cpu, apply(frames[:20], pattern[:20]), MD)
    check(gpu, cpu)
    gpu.host_free(arena)


def test_group_members_with_different_patterns(make_engine, make_oracle):
    """ratsdf_group_integrate_device_batch over three members: one all S, one all N (its segm_live stays 0 while the
    others' is live), one alternating; batches of 3 and of 5 frames; each member against its own oracle"""
    import ratsdf
    patterns = [p for _, p in GROUP]
    streams = [semantic_frames(sc, len(p)) for sc, p in GROUP]
    devs = [upload(fr) for fr in streams]
    engines = [make_engine(VS, 6 * VS) for _ in streams]
    oracles = [make_oracle(VS, 6 * VS) for _ in streams]
    group = ratsdf.Group(engines)
    h, w = streams[0][0]["depth"].shape
    s_all = range(len(streams))
    for lo, hi in ((0, 3), (3, 8)):
        rows = lambda key, kinds: [[devs[s][f][key].data_ptr() if patterns[s][f] in kinds else None for s in s_all]
                                   for f in range(lo, hi)]
        group.integrate_device_batch(group.make_batch(
            rows("rgb", "SNH"), rows("depth", "SNH"), rows("ht", "SH"), rows("lt", "S"), h, w, MD,
            [[streams[s][f]["intrinsics"] for s in s_all] for f in range(lo, hi)],
            [[streams[s][f]["pose"] for s in s_all] for f in range(lo, hi)]))
        for s in s_all:
            oracle_run(oracles[s], apply(streams[s][lo:hi], patterns[s][lo:hi]), MD)
            check(engines[s], oracles[s])
    _, blocks = engines[1].dump_directory()
    assert np.all(engines[1].dump_voxels(blocks["idx"])[2] == np.float32(0.5))
    group.close()
