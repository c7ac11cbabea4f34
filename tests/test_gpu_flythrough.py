"""The long 1280x720 / 2 mm fly-through (one pass of the 'room' camera, no frame seen twice, ~100 k blocks by frame
210) on several HIP engines in lockstep with ONE CPU oracle.  The engines differ only in how the frames reach them and
what reads the map between frames:

  stats     integrate_device one frame at a time, a statistics read after every frame (which settles the frame's
            carve tail with k_settle; the round-5 bench run)
  save      the same, plus save_map every 30 frames (tools/mapfile_probe.py's checkpoints)
  selects   the same, plus the other select-based reads every 30 frames: dump_directory, query over the map bounds,
            export_directory_device
  batch     integrate_device_batch in batches of 30 with graphs on (the product's launch mode): frames run back to
            back, each carve tail done inside the next frame's launches; read at batch boundaries only
  probe     integrate_device + synchronize and save_map every 30 frames, nothing read in between: exactly
            tools/mapfile_probe.py
  unread    integrate_device only, nothing read but the checks every 30 frames

After every frame the per-frame engines must match the oracle's statistics; at every 30-frame boundary every engine
must match its directory and free list and pass parity.assert_pool_consistent (no pool block named twice, lost or
both free and named); voxels are compared in full at frame 210 and at the end, totals at the end.  An engine that
differs is reported with its variant and the first frame that differs, and is dropped from the rest of the pass so
that the others still run to the end.

The deferred variants are the ones that caught the release role's list-order defect: with frame 193's
carve tail inside frame 194's launches, some of its head / chain deletes' free-list slots went unwritten and frame
194 handed out pool blocks still in use.  The last test saves the grown map, resumes it in a fresh engine and runs
the saver, the resumed engine and the oracle 20 more frames."""
import hashlib

import numpy as np
import pytest
import torch

import ratsdf
from parity import (assert_directory_equal, assert_heap_equal, assert_maps_equal, assert_pool_consistent,
                    assert_stats_equal)
from ratsdf import synthetic

pytestmark = pytest.mark.gpu

CAM, VS, MD = "l515_720p", 0.002, 4.0
FRAMES = 240        # the probe's save after frame 210 was the first one refused
EVERY = 30          # the probe's checkpoint period = the batch variant's batch size
FULL = (210, FRAMES)
MORE = 20           # frames after the checkpoint of the grown map
ORACLE_THREADS = 16


def frames(lo, hi):
    return [synthetic.frame("room", i, cam=CAM, noise=True, holes=True) for i in range(lo, hi)]


def upload(chunk):
    dev = torch.device("cuda", 0)
    out = [{k: torch.from_numpy(f[k]).to(dev) for k in ("rgb", "depth", "ht", "lt")} for f in chunk]
    torch.cuda.synchronize()
    return out


def feed(e, f, d):
    h, w = f["depth"].shape
    e.integrate_device(d["rgb"].data_ptr(), d["depth"].data_ptr(), d["ht"].data_ptr(), d["lt"].data_ptr(), h, w, MD,
                       f["intrinsics"], f["pose"])


def feed_batch(e, chunk, dev):
    h, w = chunk[0]["depth"].shape
    e.integrate_device_batch(e.make_batch([d["rgb"].data_ptr() for d in dev], [d["depth"].data_ptr() for d in dev],
                                          [d["ht"].data_ptr() for d in dev], [d["lt"].data_ptr() for d in dev], h, w,
                                          MD, [f["intrinsics"] for f in chunk], [f["pose"] for f in chunk]))


def map_bounds(cpu):
    """metres, one block of margin around every block of the oracle's map"""
    _, b = cpu.dump_directory()
    lo = [(int(b[k].min()) - 1) * 8 * VS for k in "xyz"]
    hi = [(int(b[k].max()) + 2) * 8 * VS for k in "xyz"]
    return (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])


def other_selects(e, cpu):
    """the select-based reads other than save_map, each checked for what it returns"""
    _, blocks = assert_directory_equal(e, cpu)
    q = e.query(map_bounds(cpu))
    assert len(q) == 512 * len(blocks), f"query over the map bounds: {len(q)} voxels, {len(blocks)} blocks"
    del q
    cap = len(blocks) + 1024
    buf = torch.zeros(cap * 3, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    e.export_directory_device(buf.data_ptr(), cap, cnt.data_ptr())
    e.synchronize()
    n = int(cnt.item())
    assert n == len(blocks), f"export_directory_device: {n} entries, directory {len(blocks)}"
    assert np.array_equal(buf.cpu().numpy()[:n * 3].view(ratsdf.BLOCK_DTYPE), blocks), "export_directory_device"


class Variant:
    def __init__(self, name, per_frame, every_frame_stats, boundary=None):
        self.name, self.per_frame, self.stats, self.boundary = name, per_frame, every_frame_stats, boundary
        self.engine = ratsdf.TSDFGrid(VS, 6 * VS)
        self.failure = None

    def check(self, frame, what, fn):
        """fn() raises AssertionError on a difference: the variant is reported with this frame and dropped"""
        if self.failure is not None:
            return
        try:
            fn()
        except (AssertionError, ratsdf.RatsdfError) as err:
            self.failure = f"{self.name}: first difference after frame {frame} ({what}): {err}"
            self.engine.close()
            self.engine = None


def _save(path):
    return lambda e, cpu: e.save_map(path)


@pytest.fixture(scope="module")
def flythrough(oracle_lib, tmp_path_factory):
    from ratsdf._abi import Engine
    tmp = tmp_path_factory.mktemp("flythrough")
    cpu = Engine(oracle_lib, VS, 6 * VS, threads=ORACLE_THREADS)
    variants = [Variant("stats", True, True), Variant("save", True, True, _save(tmp / "save.map")),
                Variant("selects", True, True, other_selects), Variant("batch", False, False),
                Variant("probe", True, False, _save(tmp / "probe.map")), Variant("unread", True, False)]
    for lo in range(0, FRAMES, EVERY):
        chunk = frames(lo, lo + EVERY)
        dev = upload(chunk)
        for i, (f, d) in enumerate(zip(chunk, dev)):
            cpu.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], MD, f["intrinsics"], f["pose"])
            for v in variants:
                if v.engine is None or not v.per_frame:
                    continue
                feed(v.engine, f, d)
                if v.stats:
                    v.check(lo + i + 1, "frame statistics", lambda: assert_stats_equal(v.engine, cpu))
                elif v.boundary is not None:
                    v.engine.synchronize()
        n = lo + EVERY
        for v in variants:
            if v.engine is None:
                continue
            if not v.per_frame:  # the batch's frames ran back to back: its last frame's statistics
                v.check(n, f"batch of frames {lo + 1} - {n}", lambda: feed_batch(v.engine, chunk, dev))
                v.check(n, f"statistics of the batch of frames {lo + 1} - {n}", lambda: assert_stats_equal(v.engine, cpu))
            if v.boundary is not None:
                v.check(n, "select-based read", lambda: v.boundary(v.engine, cpu))
            v.check(n, "directory", lambda: assert_directory_equal(v.engine, cpu))
            v.check(n, "free list", lambda: assert_heap_equal(v.engine, cpu))
            v.check(n, "pool", lambda: assert_pool_consistent(v.engine))
            if n in FULL:
                v.check(n, "voxels", lambda: assert_maps_equal(v.engine, cpu))
            if n == FRAMES:
                v.check(n, "totals", lambda: _totals_equal(v.engine, cpu))
            if v.engine is not None:
                v.engine.synchronize()  # nothing of this chunk is still read from `dev`
        del dev
    yield dict(cpu=cpu, variants={v.name: v for v in variants}, tmp=tmp)
    for v in variants:
        if v.engine is not None:
            v.engine.close()
    cpu.close()


def _totals_equal(a, b):
    ta, tb = a.totals(), b.totals()
    assert ta == tb, f"totals {ta} != {tb}"


def test_flythrough_matches_the_oracle_on_every_path(flythrough):
    bad = [v.failure for v in flythrough["variants"].values() if v.failure is not None]
    assert not bad, f"{len(bad)} of {len(flythrough['variants'])} variants differ from the oracle:\n" + "\n".join(bad)


def _digest(e):
    """the whole map -- directory, free list, every live block's voxels -- as one hash"""
    h = hashlib.sha256()
    ei, blocks = e.dump_directory()
    nf, heap = e.dump_heap()
    for a in (ei, blocks, np.int64(nf), heap[:nf]):
        h.update(np.ascontiguousarray(a).view(np.uint8))
    for lo in range(0, len(blocks), 8192):
        for a in e.dump_voxels(blocks["idx"][lo:lo + 8192]):
            h.update(a.view(np.uint8))
    return h.hexdigest()


def test_grown_map_checkpoint_resumes_exactly(flythrough, make_engine):
    """the fly-through map after 240 frames (~120 k blocks, past the probe's refusal at 210) is saved, saving changes
    nothing, a fresh engine loads it, and the saver, the resumed engine and the oracle agree 20 frames later"""
    v = flythrough["variants"]["stats"]
    if v.engine is None:
        pytest.fail(f"no grown map to checkpoint: {v.failure}")
    gpu, cpu = v.engine, flythrough["cpu"]
    path = flythrough["tmp"] / "grown.map"
    before = _digest(gpu)
    gpu.save_map(path)
    assert _digest(gpu) == before, "saving changed the map"
    assert ratsdf.map_file_info(path)["n_blocks"] == cpu.num_active_blocks()
    resumed = make_engine(VS, 6 * VS)
    resumed.load_map(path)
    assert _digest(resumed) == before, "the loaded map differs from the saved one"
    chunk = frames(FRAMES, FRAMES + MORE)
    dev = upload(chunk)
    for i, (f, d) in enumerate(zip(chunk, dev)):
        cpu.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], MD, f["intrinsics"], f["pose"])
        for name, e in (("saver", gpu), ("resumed", resumed)):
            feed(e, f, d)
            try:
                assert_stats_equal(e, cpu)
            except AssertionError as err:
                raise AssertionError(f"{name}: frame {FRAMES + i + 1}: {err}") from None
    for name, e in (("saver", gpu), ("resumed", resumed)):
        try:
            assert_maps_equal(e, cpu)
            if e is gpu:  # (a loaded map's totals start again from zero)
                _totals_equal(e, cpu)
        except AssertionError as err:
            raise AssertionError(f"{name} after frame {FRAMES + MORE}: {err}") from None


def test_deferred_carve_tails_with_many_head_and_chain_deletes(make_engine, make_oracle):
    """The release role's path on a small map: 640x480 / 5 mm frames into a 4096-entry hash table (~75 % full), so
    every frame from the 20th on carves 150 - 280 blocks and dozens of them are list heads or chain nodes -- more
    queued head / chain deletes than one wave holds, which is what made the release workgroups file them in
    different orders.  Frames go in 8-frame graph batches, so every carve tail runs inside the next frame's
    launches; directory, free list and pool are checked after every batch, the whole map at the end."""
    vs, cfg = 0.005, dict(block_bits=16, bucket_bits=11)
    gpu, cpu = make_engine(vs, 6 * vs, **cfg), make_oracle(vs, 6 * vs, threads=ORACLE_THREADS, **cfg)
    for lo in range(0, 40, 8):
        chunk = [synthetic.frame("room", i, noise=True, holes=True) for i in range(lo, lo + 8)]
        dev = upload(chunk)
        gpu.integrate_device_batch(gpu.make_batch(
            [d["rgb"].data_ptr() for d in dev], [d["depth"].data_ptr() for d in dev],
            [d["ht"].data_ptr() for d in dev], [d["lt"].data_ptr() for d in dev], 480, 640, MD,
            [f["intrinsics"] for f in chunk], [f["pose"] for f in chunk]))
        for f in chunk:
            cpu.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], MD, f["intrinsics"], f["pose"])
        try:
            assert_pool_consistent(gpu)
            assert_directory_equal(gpu, cpu)
            assert_heap_equal(gpu, cpu)
        except AssertionError as err:
            raise AssertionError(f"after frame {lo + 8}: {err}") from None
    assert cpu.totals()["deleted_blocks"] > 2000
    assert_maps_equal(gpu, cpu)
    _totals_equal(gpu, cpu)
