"""Mixed semantic / TSDF-only streams on the CPU: the batch entry point of the Python binding keeps semantics per
frame, and every stream the batch-path tests use (tests/mixed_cases.py) can fail -- the frame-by-frame oracle's map
for the stream's pattern lies away from the maps of the plausible wrong patterns (every frame TSDF-only, every frame
with its predecessor's setting, every frame semantic) by far more than the parity tolerance."""
import numpy as np
import pytest

from mixed_cases import (FRAMECAST, GRAPH_REPLAY, GROUP, PATTERNS, apply, distinguishes, oracle_run, pinned_pattern,
                         semantic_frames, staging_pattern, wrong_patterns)
from parity import TOL, assert_maps_equal

VS, MD = 0.02, 4.0

# (scene, pattern, scale, voxel size): the whole stream of each GPU test, batches concatenated
STREAMS = ([("room", p + p, 0.25, VS) for p in PATTERNS] +
           [("room", "".join(GRAPH_REPLAY), 0.25, VS), ("room", staging_pattern(51), 0.25, VS),
            ("room", pinned_pattern(40), 0.25, VS), ("room", FRAMECAST, 0.25, VS)] +
           [(sc, p, 0.25, VS) for sc, p in GROUP] +
           [("room", "SNSN", 1.0, 0.005)])


def test_wrong_patterns():
    assert wrong_patterns("SNSN") == ["NNNN", "SSNS", "SSSS"]
    assert wrong_patterns("SSSS") == ["NNNN"]
    assert wrong_patterns("NNNN") == ["SSSS"]
    assert wrong_patterns("SHNS") == ["NNNN", "SSHN", "SSSS"]   # (H is TSDF-only: HHHH would be the right map)


@pytest.mark.parametrize("scene,pattern,scale,vs", STREAMS, ids=[f"{s[0]}-{s[1]}-{s[3]}" for s in STREAMS])
def test_stream_tells_wrong_patterns_apart(scene, pattern, scale, vs, make_oracle):
    frames = semantic_frames(scene, len(pattern), scale=scale)
    gaps = distinguishes(make_oracle, frames, pattern, vs, MD, threads=16 if scale == 1.0 else 0)
    assert gaps and all(g > 100 * TOL for g in gaps.values()), gaps


def test_oracle_batch_keeps_semantics_per_frame(make_oracle):
    """Engine.integrate_batch (ratsdf_integrate_batch's pointer tables) with every second frame TSDF-only: the tables
    must carry the semantic frames' images and NULL for the others, not drop the semantics of the whole batch"""
    frames = apply(semantic_frames("room", 6), "SNSNSN")
    batch, single = make_oracle(VS, 6 * VS), make_oracle(VS, 6 * VS)
    batch.integrate_batch(frames, MD)
    oracle_run(single, frames, MD)
    w = assert_maps_equal(batch, single)
    assert w["prob"] == 0.0 and w["tsdf"] == 0.0
    assert batch.totals() == single.totals()
    _, blocks = batch.dump_directory()
    assert np.any(batch.dump_voxels(blocks["idx"])[2] != np.float32(0.5))
    # a frame with ht but no lt is TSDF-only (the table entry of lt is NULL)
    frames = apply(semantic_frames("room", 4), "SHNS")
    batch, single = make_oracle(VS, 6 * VS), make_oracle(VS, 6 * VS)
    batch.integrate_batch(frames, MD)
    oracle_run(single, frames, MD)
    w = assert_maps_equal(batch, single)
    assert w["prob"] == 0.0 and w["tsdf"] == 0.0
