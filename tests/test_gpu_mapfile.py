"""Map checkpoints on the MI355X (ratsdf_save_map / ratsdf_load_map): a map saved after A frames and loaded into an
engine continues bit-exactly -- the result after B more frames equals the CPU oracle after A + B frames; saving
changes nothing; the file holds the oracle's state; an oracle-made file loads; refused loads leave the map alone."""
import numpy as np
import pytest

import mapfile_ref as ref
from parity import assert_maps_equal, assert_stats_equal
from ratsdf import synthetic

pytestmark = pytest.mark.gpu

VS = 0.02


def _run(engines, frames):
    for f in frames:
        for e in engines:
            e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])


def _snapshot(e):
    ei, blocks = e.dump_directory()
    nf, heap = e.dump_heap()
    t, c, p = e.dump_voxels(blocks["idx"])
    return ei, blocks, nf, heap[:nf].copy(), t, c, p


def _same_snapshot(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y


@pytest.fixture(scope="module")
def churn():
    """a stream that allocates and carves on both sides of the cut"""
    return synthetic.stream("sphere", 24, scale=0.25, noise=True, holes=True)


def test_resume_is_exact_and_saving_changes_nothing(tmp_path, churn, make_engine, make_oracle):
    A = 12
    gpu, cpu = make_engine(VS, 6 * VS), make_oracle(VS, 6 * VS, threads=8)
    _run([gpu, cpu], churn[:A])
    before = _snapshot(gpu)
    path = tmp_path / "a.map"
    gpu.save_map(path)
    assert not (tmp_path / "a.map.tmp").exists()
    _same_snapshot(before, _snapshot(gpu))  # saving is read-only for the map

    # 3. the file is the oracle's state after A frames
    m = ref.parse(path.read_bytes())
    ei, blocks = cpu.dump_directory()
    live = m["blocks"]["idx"] >= 0
    assert np.array_equal(m["entry_index"][live], ei)
    for f in ("x", "y", "z", "offset", "idx"):
        assert np.array_equal(m["blocks"][f][live], blocks[f])
    assert np.all(m["blocks"]["offset"][~live] != 0) and np.all(m["blocks"]["idx"][~live] == -1)
    nf, heap = cpu.dump_heap()
    assert m["num_free"] == nf and np.array_equal(m["heap"], heap[:nf])
    assert 0 <= m["free_low"] <= nf and np.all(blocks["idx"] >= m["free_low"])
    t, c, p = cpu.dump_voxels(blocks["idx"])
    assert np.array_equal(m["rgbw"], c)
    assert np.max(np.abs(m["tsdf"] - t)) <= 1e-4 and np.max(np.abs(m["prob"] - p)) <= 1e-4
    assert m["segm_live"] == 1
    assert np.array_equal(m["free_rgbw"], cpu.dump_voxels(heap[m["free_low"]:nf])[1])
    info = __import__("ratsdf").map_file_info(path)
    assert info["n_blocks"] == len(ei) and info["voxel_size"] == np.float32(VS)

    # 1. a fresh engine resumes from the file; 2. the engine that saved goes on as if nothing happened
    resumed = make_engine(VS, 6 * VS)
    resumed.load_map(path)
    assert_maps_equal(resumed, gpu)
    deleted = 0
    for f in churn[A:]:
        for e in (gpu, resumed, cpu):
            e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
        assert_stats_equal(resumed, cpu)
        assert_stats_equal(gpu, cpu)
        deleted += resumed.last_frame_stats()["deleted_blocks"]
    assert deleted > 0
    assert_maps_equal(resumed, cpu)
    assert_maps_equal(gpu, cpu)


def test_oracle_made_file_loads(tmp_path, churn, make_engine, make_oracle):
    A = 10
    cpu = make_oracle(VS, 6 * VS, threads=8)
    _run([cpu], churn[:A])
    path = tmp_path / "oracle.map"
    path.write_bytes(ref.from_dumps(cpu))
    gpu = make_engine(VS, 6 * VS)
    gpu.load_map(path)
    assert_maps_equal(gpu, cpu)
    for f in churn[A:]:
        _run([gpu, cpu], [f])
        assert_stats_equal(gpu, cpu)
    assert_maps_equal(gpu, cpu)


def _upload(frames):
    import torch
    dev = torch.device("cuda", 0)
    return [{k: torch.from_numpy(f[k]).to(dev) for k in ("rgb", "depth", "ht", "lt")} for f in frames]


def test_load_replaces_a_live_map_of_a_group_member(tmp_path, churn, make_engine, make_oracle):
    """the engine has a map of its own, belongs to a group and has replayed a captured batch graph: after the load
    both paths go on matching the oracle (no buffer of the engine was reallocated)"""
    import ratsdf
    room = synthetic.stream("room", 6, scale=0.25, noise=True, holes=True)
    A = 8
    src, cpu = make_engine(VS, 6 * VS), make_oracle(VS, 6 * VS, threads=8)
    _run([src, cpu], churn[:A])
    path = tmp_path / "src.map"
    src.save_map(path)

    gpu, other = make_engine(VS, 6 * VS), make_engine(VS, 6 * VS)
    d_room, d_churn = _upload(room), _upload(churn)
    h, w = room[0]["depth"].shape

    def batch(eng, frames, dev):
        return eng.make_batch([d["rgb"].data_ptr() for d in dev], [d["depth"].data_ptr() for d in dev],
                              [d["ht"].data_ptr() for d in dev], [d["lt"].data_ptr() for d in dev], h, w, 4.0,
                              [f["intrinsics"] for f in frames], [f["pose"] for f in frames])

    gpu.integrate_device_batch(batch(gpu, room[:3], d_room[:3]))
    gpu.integrate_device_batch(batch(gpu, room[3:6], d_room[3:6]))  # the same graph, replayed
    group = ratsdf.Group([gpu, other])
    rows = lambda key, lo, hi: [[d_room[f][key].data_ptr()] * 2 for f in range(lo, hi)]
    group.integrate_device_batch(group.make_batch(rows("rgb", 0, 2), rows("depth", 0, 2), rows("ht", 0, 2),
                                                  rows("lt", 0, 2), h, w, 4.0,
                                                  [[room[f]["intrinsics"]] * 2 for f in range(2)],
                                                  [[room[f]["pose"]] * 2 for f in range(2)]))
    group.synchronize()
    assert gpu.num_active_blocks() > 0

    gpu.load_map(path)
    assert_maps_equal(gpu, cpu)
    # on: a graph-replayed batch of the shape captured before, then a group batch with the other member
    gpu.integrate_device_batch(batch(gpu, churn[A:A + 3], d_churn[A:A + 3]))
    _run([cpu], churn[A:A + 3])
    assert_stats_equal(gpu, cpu)
    assert_maps_equal(gpu, cpu)
    lo, hi = A + 3, A + 5
    group.integrate_device_batch(group.make_batch(
        [[d_churn[f]["rgb"].data_ptr(), d_room[0]["rgb"].data_ptr()] for f in range(lo, hi)],
        [[d_churn[f]["depth"].data_ptr(), d_room[0]["depth"].data_ptr()] for f in range(lo, hi)],
        [[d_churn[f]["ht"].data_ptr(), d_room[0]["ht"].data_ptr()] for f in range(lo, hi)],
        [[d_churn[f]["lt"].data_ptr(), d_room[0]["lt"].data_ptr()] for f in range(lo, hi)], h, w, 4.0,
        [[churn[f]["intrinsics"], room[0]["intrinsics"]] for f in range(lo, hi)],
        [[churn[f]["pose"], room[0]["pose"]] for f in range(lo, hi)]))
    group.synchronize()
    _run([cpu], churn[lo:hi])
    assert_maps_equal(gpu, cpu)
    group.close()


def test_tsdf_only_map_keeps_its_probabilities(tmp_path, make_engine, make_oracle):
    """a map that has never seen ht / lt is saved with segm_live = 0 and continues without touching the
    probabilities (every one stays exactly 0.5); a map holding imported blocks carries segm_live = 1"""
    frames = synthetic.stream("sphere", 8, scale=0.25, semantic=False)
    gpu, cpu = make_engine(VS, 6 * VS), make_oracle(VS, 6 * VS, threads=8)
    _run([gpu, cpu], frames[:4])
    path = tmp_path / "tsdf.map"
    gpu.save_map(path)
    assert ref.parse(path.read_bytes())["segm_live"] == 0
    resumed = make_engine(VS, 6 * VS)
    resumed.load_map(path)
    _run([resumed, cpu], frames[4:])
    assert_maps_equal(resumed, cpu)
    _, blocks = resumed.dump_directory()
    _, _, prob = resumed.dump_voxels(blocks["idx"])
    assert prob.size and np.all(prob == np.float32(0.5))

    imp = make_engine(VS, 6 * VS)
    t, c, p = cpu.dump_voxels(blocks["idx"][:5])
    pos = np.stack([blocks["x"][:5], blocks["y"][:5], blocks["z"][:5]], axis=1)
    imp.import_blocks(pos, t, c, p)
    path2 = tmp_path / "imported.map"
    imp.save_map(path2)
    m = ref.parse(path2.read_bytes())
    assert m["segm_live"] == 1 and len(m["tsdf"]) == 5


def test_refused_loads_leave_the_map_untouched(tmp_path, churn, make_engine):
    import ratsdf
    gpu = make_engine(VS, 6 * VS)
    _run([gpu], churn[:4])
    good = tmp_path / "good.map"
    gpu.save_map(good)
    _run([gpu], churn[4:7])
    before = _snapshot(gpu)
    data = good.read_bytes()
    m = ref.parse(data)
    cfg = ref.engine_config(gpu)
    remake = lambda **kw: ref.build({**cfg, **kw}, m["entry_index"], m["blocks"], m["heap"], m["free_low"],
                                    m["segm_live"], m["tsdf"], m["rgbw"], m["prob"], m["free_rgbw"])
    corrupt = bytearray(data)
    corrupt[m["voxel_offset"] + 100] ^= 1
    bad = {"voxel size": remake(voxel_size=0.01), "truncation": remake(truncation=0.1),
           "block bits": remake(block_bits=17), "bucket bits": remake(bucket_bits=20),
           "shard count": remake(shard_count=2), "shard slab": remake(shard_slab_bits=3),
           "corrupted": bytes(corrupt), "truncated": data[:-100]}
    for what, blob in bad.items():
        p = tmp_path / "bad.map"
        p.write_bytes(blob)
        with pytest.raises(ratsdf.RatsdfError) as ei:
            gpu.load_map(p)
        assert ei.value.status == 1, what
        _same_snapshot(before, _snapshot(gpu))
    with pytest.raises(ratsdf.RatsdfError):
        gpu.load_map(tmp_path / "absent.map")
    _same_snapshot(before, _snapshot(gpu))
    # a failed save leaves the earlier file as it was
    with pytest.raises(ratsdf.RatsdfError):
        gpu.save_map(tmp_path / "no_such_dir" / "x.map")
    assert good.read_bytes() == data


def test_offline_eval_resumes_from_a_saved_map(tmp_path, make_oracle):
    """ratsdf_offline_eval: frames [0, 6) in one run == frames [0, 3) with --save-map, then --load-map with
    --first-frame 3 -- the two DownloadAll files are byte-identical and hold the oracle's map"""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root / "oracle"))
    import dataset_oracle as O
    from make_dataset import write_folder
    from ratsdf import pose as P
    from test_dataset_reader import build
    write_folder(tmp_path / "ds", n=6, scale=0.25, factor=1000.0, scene="room")
    lib = root / "ra-slam_amd" / "csrc" / "build" / "libratsdf.so"
    run = lambda *a: subprocess.run([str(build()), str(tmp_path / "ds"), "--lib", str(lib), *map(str, a)],
                                    capture_output=True, text=True, timeout=600)
    a, b, m = tmp_path / "a.bin", tmp_path / "b.bin", tmp_path / "cut.map"
    for args in (("--voxel", "0.02", "--download-all", a), ("--voxel", "0.02", "--frames", 3, "--save-map", m),
                 ("--voxel", "0.02", "--load-map", m, "--first-frame", 3, "--download-all", b)):
        r = run(*args)
        assert r.returncode == 0, r.stdout + r.stderr
    assert a.read_bytes() == b.read_bytes()
    r = run("--voxel", "0.01", "--load-map", m, "--first-frame", 3)  # the file's voxel size is not --voxel
    assert r.returncode != 0 and "voxel size" in r.stderr
    REC = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("tsdf", "<f4"), ("prob", "<f4")])
    got = np.fromfile(b, dtype=REC)
    ds = O.read_folder(tmp_path / "ds")
    cpu = make_oracle(0.02, 0.12)
    for i in range(6):
        rgb, depth = ds["frame"](i)
        cpu.integrate(rgb, depth, None, None, 6.0, ds["intrinsics"], P.compose(ds["extrinsics"], ds["poses"][i]))
    exp = cpu.gather_valid_semantic()
    assert len(got) == len(exp) and len(got) > 1000
    key = lambda x: np.lexsort((x["z"], x["y"], x["x"]))
    g, e = got[key(got)], exp[key(exp)]
    for f in ("x", "y", "z"):
        assert np.array_equal(g[f], e[f]), f
    assert np.max(np.abs(g["tsdf"] - e["tsdf"])) <= 1e-4
