"""The staging ring of the host-image entry points at every ring position and from all three kinds of source, and the
order in which an engine's and a group's streams, events and graphs are given back (ra-slam_amd/csrc/stage_ring.inc,
stage_plan.h, hip_handles.h).  The schedule's arithmetic is tested on the host alone (tests/test_stage_plan.py); here
the same calls run against real copies, events and launches."""
import numpy as np
import pytest

from parity import assert_maps_equal
from ratsdf import synthetic

pytestmark = pytest.mark.gpu

SLOTS = 16       # kStageSlots
H, W = 32, 48


def small_frame(i, semantic=True):
    """a 48 x 32 cut of a 64 x 48 frame (the principal point stays where it was: off the cut's centre)"""
    f = synthetic.frame("room", i, scale=0.1, noise=True, holes=True)
    g = dict(f, width=W, height=H)
    for k in ("rgb", "depth", "ht", "lt"):
        g[k] = np.ascontiguousarray(f[k][:H, :W]) if semantic or k in ("rgb", "depth") else None
    return g


def test_ring_positions_and_all_three_kinds_of_source(make_engine, make_oracle):
    """Five single calls (so that the batches do not begin at slot 0), a pageable batch, a page-locked batch of
    separate images, a page-locked batch of blocks that lie side by side at the ring's stride -- it begins at slot 11:
    its second run is cut at the ring's end -- and three more single calls; each batch is 2 x 16 + 3 frames, so the ring
    wraps twice inside it.  Nothing is waited for between the calls.  Same map as the oracle's after the same frames."""
    vs, md = 0.04, 4.0
    gpu, cpu = make_engine(vs, 6 * vs), make_oracle(vs, 6 * vs)
    n = 2 * SLOTS + 3
    npx = H * W
    frames = iter(range(10 ** 6))
    done = []

    def single(count):
        for _ in range(count):
            f = small_frame(next(frames), semantic=len(done) % 2 == 1)  # TSDF-only and semantic, alternating
            gpu.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], md, f["intrinsics"], f["pose"])
            done.append(f)

    def into(f, **views):  # the frame with its images copied into the given page-locked views
        g = dict(f)
        for k, v in views.items():
            v[...] = f[k]
            g[k] = v
        return g

    single(5)
    # 1. pageable
    batch = [small_frame(next(frames)) for _ in range(n)]
    gpu.integrate_batch(batch, md)
    done += batch
    # 2. page-locked, every kind of image in an arena of its own: no frame is a packed block
    arenas = dict(depth=gpu.host_alloc((n, H, W), np.float32), ht=gpu.host_alloc((n, H, W), np.float32),
                  lt=gpu.host_alloc((n, H, W), np.float32), rgb=gpu.host_alloc((n, H, W, 3), np.uint8))
    batch = [into(small_frame(next(frames)), **{k: a[i] for k, a in arenas.items()}) for i in range(n)]
    gpu.integrate_batch(batch, md, pinned=True)
    done += batch
    # 3. page-locked blocks depth | ht | lt | rgb, 16 bytes per pixel, side by side
    assert (5 + 2 * n) % SLOTS == 11
    arena = gpu.host_alloc((n * npx * 16,), np.uint8)

    def block(i):
        blk = arena[i * npx * 16:(i + 1) * npx * 16]
        return dict(depth=blk[:npx * 4].view(np.float32).reshape(H, W),
                    ht=blk[npx * 4:npx * 8].view(np.float32).reshape(H, W),
                    lt=blk[npx * 8:npx * 12].view(np.float32).reshape(H, W), rgb=blk[npx * 12:npx * 15].reshape(H, W, 3))
    batch = [into(small_frame(next(frames)), **block(i)) for i in range(n)]
    gpu.integrate_batch(batch, md, pinned=True)
    done += batch
    single(3)
    assert len(done) == 5 + 3 * n + 3
    for f in done:
        cpu.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], md, f["intrinsics"], f["pose"])
    assert_maps_equal(gpu, cpu)
    assert gpu.totals() == cpu.totals()
    for a in list(arenas.values()) + [arena]:
        gpu.host_free(a)


def test_engines_and_a_group_are_given_back_cleanly():
    """What an engine and a group hold when they go: a captured batch graph with its tables, the staging ring with
    its streams and events, both timers' events.  Every call returns RATSDF_OK; a second engine comes and goes after."""
    import ratsdf
    import torch
    lib = ratsdf.library()
    vs, md = 0.02, 4.0
    dev = torch.device("cuda", 0)
    frames = synthetic.stream("room", 3, scale=0.25)
    h, w = frames[0]["depth"].shape
    d = [{k: torch.from_numpy(f[k]).to(dev) for k in ("rgb", "depth", "ht", "lt")} for f in frames]
    torch.cuda.synchronize()
    ptr = lambda key, count: [d[i][key].data_ptr() for i in range(count)]
    a, b = ratsdf.TSDFGrid(vs, 6 * vs), ratsdf.TSDFGrid(vs, 6 * vs)
    # (every call below raises unless it returns RATSDF_OK)
    a.integrate_device_batch(a.make_batch(ptr("rgb", 3), ptr("depth", 3), ptr("ht", 3), ptr("lt", 3), h, w, md,
                                          [f["intrinsics"] for f in frames], [f["pose"] for f in frames]))
    a.profile_enable(True)
    a.integrate_batch(frames, md)
    group = ratsdf.Group([a, b])
    group.profile_enable(True)
    rows = lambda key: [[d[f][key].data_ptr()] * 2 for f in range(2)]
    group.integrate_device_batch(group.make_batch(rows("rgb"), rows("depth"), rows("ht"), rows("lt"), h, w, md,
                                                  [[frames[f]["intrinsics"]] * 2 for f in range(2)],
                                                  [[frames[f]["pose"]] * 2 for f in range(2)]))
    assert lib.fn["group_destroy"](group._h) == 0
    group._h = None
    for e in (a, b):
        assert lib.fn["destroy"](e._h) == 0
        e._h = None
    c = ratsdf.TSDFGrid(vs, 6 * vs)
    assert lib.fn["destroy"](c._h) == 0
    c._h = None
