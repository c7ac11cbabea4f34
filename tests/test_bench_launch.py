"""`python bench.py --gpus N` with no launcher around it starts its N ranks itself (child processes through
torch.distributed.run, rendezvous on 127.0.0.1), forwards rank 0's JSON line and exits with the ranks' status.

Without a GPU the ranks cannot integrate anything (the engine has no CPU path), so the CPU test checks the
launch itself: N ranks really start with RANK / WORLD_SIZE set, each refuses for the right reason, and the
failure reaches the caller's exit status.  On the GPU box the same entry runs the N = 2 control flow end to end
(both ranks on the one device, gloo instead of RCCL: RATSDF_BENCH_DEVICE / RATSDF_BENCH_BACKEND)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _run(args, extra_env, timeout):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.pop("LOCAL_RANK", None)
    env.update(extra_env)
    return subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, capture_output=True, text=True,
                          timeout=timeout, env=env, cwd=str(ROOT))


def test_gpus_n_starts_n_ranks_and_propagates_their_status():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: covered by test_two_ranks_through_the_plain_entry_point")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], {}, 300)
    out = r.stdout + r.stderr
    assert r.returncode != 0, out[-2000:]
    # both ranks started and stopped at the engine's "no GPU" refusal (not at an argument or rendezvous error)
    assert out.count("needs an MI355X") >= 2, out[-2000:]
    assert "launch N > 1 with" not in out


@pytest.mark.gpu
def test_two_ranks_through_the_plain_entry_point():
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--reps", "1", "--frames-per-step", "12",
              "--cpu-frames", "0", "--host-frames", "0", "--no-secondary", "--streams", "0"],
             {"RATSDF_BENCH_DEVICE": "0", "RATSDF_BENCH_BACKEND": "gloo"}, 600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]          # ONE JSON line, rank 0's
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["config"]["streams"] == 2
    assert d["directory_blocks_all_ranks"] > 0          # the directory exchange ran


@pytest.mark.gpu
def test_one_stream_over_two_subvolume_ranks_through_the_plain_entry_point(tmp_path):
    """BASELINE configs[3] end to end through `python bench.py --gpus 2 --shard`: rank 0 owns the stream, the frames
    reach rank 1 by broadcast (inside the timed region), each rank integrates its subvolume (checked against the
    sharded CPU oracle on the bytes it received), the directory deltas are all-gathered, and every block of the
    union sits on its owner and nowhere else.  Both ranks on the one device, gloo instead of RCCL.  (The parity check
    is part of --full.)"""
    r = _run(["--gpus", "2", "--shard", "--steps", "2", "--warmup", "1", "--reps", "1", "--frames-per-step", "12",
              "--bcast-chunk", "4", "--cpu-frames", "4", "--full", "--dump-outputs", str(tmp_path / "out")],
             {"RATSDF_BENCH_DEVICE": "0", "RATSDF_BENCH_BACKEND": "gloo"}, 600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["scaling"] == "strong" and d["n_gpus"] == 2 and d["config"]["streams"] == 1 and d["value"] > 0
    fb = d["frame_broadcast"]
    assert fb["in_timed_region"] and fb["chunk_frames"] == 4 and fb["frames_ahead"] == 8 and fb["broadcast_gbps"] > 0
    assert fb["bytes_per_frame"] == 640 * 480 * 15 + 64
    # the directory exchange ran, and the union of the ranks' block sets is what check_sharded_directories expects:
    # every block on its owner, on no other rank
    assert d["directory_blocks_all_ranks"] == d["directory_union_blocks"] > 0
    assert len(d["shards"]) == 2 and all(s["active_blocks"] > 0 for s in d["shards"])
    assert sum(s["active_blocks"] for s in d["shards"]) == d["directory_union_blocks"]
    assert d["parity"]["frames"] == 4 and d["parity"]["max_abs_tsdf"] == 0.0 and d["parity"]["max_abs_prob"] < 1e-4
    # --dump-outputs writes rank 0's subvolume: its blocks, each owned by rank 0 (floormod(block.x >> 2, 2) == 0)
    dump = _load_dump(tmp_path / "out")
    x = dump["blocks"][:, 0].astype(np.int64)
    assert len(x) == d["dump_outputs"]["active_blocks"] == d["shards"][0]["active_blocks"]
    assert np.all((x >> 2) % 2 == 0) and dump["tsdf"].shape == (d["dump_outputs"]["blocks_with_voxels"], 512)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["streams", "shard"])
def test_the_multi_rank_code_path_over_rccl_with_a_group_of_one(mode):
    """The calls an 8-GPU run makes, over RCCL itself: RCCL refuses two ranks on one device, so the one-GPU box takes
    bench.py's N > 1 path with a process group of ONE rank (RATSDF_BENCH_ONE_RANK_GROUP=1): init_process_group("nccl",
    device_id=...), the directory exchange on device tensors (all_gather_into_tensor), barrier, all_reduce(MAX) of the
    step time -- and, with --shard, the frame broadcast on its side stream and all_gather_object of the shard table."""
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--reps", "1", "--frames-per-step", "12", "--cpu-frames", "4"]
    args += ["--shard", "--bcast-chunk", "4", "--full"] if mode == "shard" else ["--host-frames", "0", "--no-secondary",
                                                                                  "--streams", "0"]
    r = _run(args, {"RATSDF_BENCH_ONE_RANK_GROUP": "1"}, 600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["value"] > 0
    assert d["directory_blocks_all_ranks"] > 0          # the RCCL all-gather of the directory ran
    if mode == "shard":
        assert d["scaling"] == "strong" and d["frame_broadcast"]["backend"] == "nccl"
        assert d["frame_broadcast"]["in_timed_region"] and d["frame_broadcast"]["broadcast_gbps"] > 0
        assert d["directory_union_blocks"] == d["directory_blocks_all_ranks"] and len(d["shards"]) == 1
        assert d["parity"]["frames"] == 4 and d["parity"]["max_abs_tsdf"] == 0.0
    else:
        assert d["config"]["streams"] == 1 and d["config"]["directory_allgather_every_frames"] == 12


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load_dump(d):
    return {p.stem: np.load(p) for p in sorted(Path(d).glob("*.npy"))}


def test_dump_outputs_writes_the_map_sorted_and_sampled(tmp_path, make_oracle, monkeypatch):
    """bench.dump_outputs on the CPU oracle (same C ABI as the engine): float arrays only, blocks in coordinate
    order, voxels equal to dump_voxels of those blocks; a map above DUMP_MAX_BLOCKS is sampled, the same way twice."""
    from ratsdf import synthetic
    bench = _bench_module()
    e = make_oracle(0.02, 0.12)
    for i in range(2):
        f = synthetic.frame("room", i, scale=0.25)
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
    info = bench.dump_outputs(e, tmp_path / "all")
    d = _load_dump(tmp_path / "all")
    assert set(d) == {"blocks", "sample_index", "tsdf", "prob", "weight", "rgb"}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    n = e.num_active_blocks()
    assert n > 8 and info["active_blocks"] == info["blocks_with_voxels"] == n
    assert d["blocks"].shape == (n, 3) and d["tsdf"].shape == (n, 512) and d["rgb"].shape == (n, 512, 3)
    assert info["bytes"] == sum(a.nbytes for a in d.values()) <= bench.DUMP_LIMIT_BYTES
    keys = [tuple(r) for r in d["blocks"]]
    assert keys == sorted(keys) and len(set(keys)) == n
    _, blk = e.dump_directory()
    pos = {(int(b["x"]), int(b["y"]), int(b["z"])): int(b["idx"]) for b in blk}
    idx = [pos[k] for k in keys]
    tsdf, rgbw, prob = e.dump_voxels(idx)
    assert np.array_equal(d["tsdf"], tsdf) and np.array_equal(d["prob"], prob)
    assert np.array_equal(d["weight"], rgbw["weight"].astype(np.float32))
    assert np.array_equal(d["rgb"][..., 1], rgbw["g"].astype(np.float32))
    assert d["weight"].max() > 0

    monkeypatch.setattr(bench, "DUMP_MAX_BLOCKS", 5)
    bench.dump_outputs(e, tmp_path / "s1")
    bench.dump_outputs(e, tmp_path / "s2")
    s1, s2 = _load_dump(tmp_path / "s1"), _load_dump(tmp_path / "s2")
    assert s1["tsdf"].shape == (5, 512) and np.array_equal(s1["blocks"], d["blocks"])
    sel = s1["sample_index"].astype(int)
    assert np.array_equal(s1["tsdf"], d["tsdf"][sel]) and np.array_equal(s1["rgb"], d["rgb"][sel])
    for k in s1:
        assert np.array_equal(s1[k], s2[k]), k


@pytest.mark.gpu
def test_bench_dump_outputs_is_the_map_of_the_timed_steps(tmp_path):
    """`bench.py --dump-outputs`: what it writes is the map of the warm-up and the K timed steps, equal to the CPU
    oracle fed the same frames; `steps` / `ms_per_step` in the line describe those K steps."""
    from oracle_binding import load_oracle
    from ratsdf._abi import Engine
    bench = _bench_module()
    B, steps, warmup = 12, 2, 1
    r = _run(["--steps", str(steps), "--warmup", str(warmup), "--reps", "1", "--frames-per-step", str(B),
              "--cpu-frames", "0", "--host-frames", "0", "--no-secondary", "--streams", "0",
              "--dump-outputs", str(tmp_path / "out")], {}, 600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["reps"] == 1
    d = _load_dump(tmp_path / "out")
    assert line["dump_outputs"]["bytes"] == sum(a.nbytes for a in d.values()) <= bench.DUMP_LIMIT_BYTES
    frames = bench.make_stream("room", "scannet", (B + 1) // 2, phase=0)[:B]
    cpu = Engine(load_oracle(), 0.005, 6 * 0.005, threads=8)     # bench.py's voxel and truncation
    for _ in range(warmup + steps):
        for f in frames:
            cpu.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
    _, blk = cpu.dump_directory()
    keys = sorted((int(b["x"]), int(b["y"]), int(b["z"])) for b in blk)
    assert [tuple(int(v) for v in row) for row in d["blocks"]] == keys
    pos = {(int(b["x"]), int(b["y"]), int(b["z"])): int(b["idx"]) for b in blk}
    tsdf, rgbw, prob = cpu.dump_voxels([pos[keys[i]] for i in d["sample_index"].astype(int)])
    cpu.close()
    assert np.max(np.abs(d["tsdf"] - tsdf)) <= 1e-4 and np.max(np.abs(d["prob"] - prob)) <= 1e-4
    assert np.array_equal(d["weight"], rgbw["weight"].astype(np.float32))
    assert np.array_equal(d["rgb"], np.stack([rgbw["r"], rgbw["g"], rgbw["b"]], axis=-1).astype(np.float32))


FULL_ONLY_KEYS = ("parity", "cpu_baseline", "host_enqueue_us_per_frame", "host_enqueue_frac", "synchronous_frame_path",
                  "host_image_path", "pinned_h2d_path", "tsdf_system_path", "tsdf_only", "multi_stream", "secondary",
                  "flythrough")


@pytest.mark.gpu
def test_a_plain_run_times_the_steps_and_leaves_every_other_leg_to_full():
    """Without --full the run sets up, warms up, times the steps and prints the line: every other leg and check is
    null, whatever their own options say (here their defaults).  With --full the same options bring them back."""
    common = ["--steps", "2", "--warmup", "1", "--reps", "1", "--frames-per-step", "12"]
    r = _run(common, {}, 600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["roofline"]["launches"] > 0          # measured inside the timed region: part of a plain run
    assert {k: d[k] for k in FULL_ONLY_KEYS} == {k: None for k in FULL_ONLY_KEYS}

    r = _run(common + ["--full", "--cpu-frames", "12", "--host-frames", "0", "--no-secondary", "--streams", "0"], {}, 600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["parity"]["frames"] == 12 and d["parity"]["max_abs_tsdf"] == 0.0
    assert d["cpu_baseline"]["value"] > 0 and d["host_enqueue_us_per_frame"] > 0


@pytest.mark.gpu
def test_a_plain_flythrough_run_leaves_parity_and_event_passes_to_full():
    """--config flythrough: a plain run times the graph passes alone; --full adds the oracle over the whole pass and
    the per-frame event passes."""
    r = _run(["--config", "flythrough", "--flythrough-frames", "8"], {}, 600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    f = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["flythrough"]
    assert f["frames_per_s"] > 0 and f["parity"] is None and f["frame_period_us"] is None and f["k_integrate_us"] is None
    r = _run(["--config", "flythrough", "--flythrough-frames", "8", "--full"], {}, 600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    f = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["flythrough"]
    assert f["parity"]["frames"] == 8 and f["parity"]["max_abs_tsdf"] == 0.0
    assert f["frame_period_us"]["p50"] > 0 and f["k_integrate_us"]["p50"] > 0


def test_full_is_off_unless_given():
    bench = _bench_module()
    for config in bench.CONFIG_DEFAULTS:
        assert not bench.parse(["--config", config]).full and bench.parse(["--config", config, "--full"]).full


def test_options_given_are_taken_as_given_under_every_config():
    """--steps / --warmup / --reps (and the other options with per-config defaults) set what they name under every
    --config, the config's default value included (`--config bigmap --steps 60` runs 60 timed steps); only options
    not given take the config's defaults."""
    bench = _bench_module()
    for config, dflt in bench.CONFIG_DEFAULTS.items():
        a = bench.parse(["--config", config])
        assert {k: getattr(a, k) for k in dflt} == dflt, config
        given = dict(steps=60, warmup=3, reps=5, frames_per_step=90, cpu_frames=1080, flythrough_frames=180)
        a = bench.parse(["--config", config] + [x for k, v in given.items() for x in (f"--{k.replace('_', '-')}", str(v))])
        assert {k: getattr(a, k) for k in given} == given, config
        a = bench.parse(["--config", config, "--steps", "7", "--warmup", "0", "--reps", "1"])
        assert (a.steps, a.warmup, a.reps) == (7, 0, 1), config
    assert bench.CONFIG_DEFAULTS["bigmap"]["steps"] != 60   # (the case the old "== 60 means not given" test got wrong)
