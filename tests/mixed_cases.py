"""Streams that mix frames with semantics and TSDF-only frames, for the batch paths' tests.

The reference decides semantics frame by frame (modules/tsdf_module.cc:27-31): a frame without ht or lt is fused
with all-ones images, which leave the probability where it is.  A pattern is a string with one letter per frame:

    S   ht and lt given: the frame updates the probability
    N   neither given: TSDF-only
    H   ht given, lt missing: TSDF-only by the same rule

Every frame carries ht / lt images of its own (the synthetic field shifted by the frame number), so a frame that
read another frame's images -- or a TSDF-only frame that read stale bytes -- changes the map.

A stream only tests what it can tell apart: `distinguishes()` runs the frame-by-frame oracle with the stream's
pattern and with the plausible wrong ones (every frame TSDF-only, every frame with its predecessor's setting, every
frame semantic) and returns how far each wrong map lies from the right one in probability.
"""
import numpy as np

from ratsdf import synthetic

# the single-batch patterns: every kind of neighbour pair at every position
PATTERNS = ["SNSNSN", "NNNSSN", "SSSNNN", "NSSN", "SHSNHS"]
# three 4-frame batches back to back on one engine: every position changes its kind between batches
GRAPH_REPLAY = ["NNSN", "SNNS", "NSSN"]


def staging_pattern(n):
    """host frames: frame i of a fresh engine takes staging slot i % 16; every slot alternates between S and a
    TSDF-only kind from one lap of the ring to the next, so TSDF-only frames land where an earlier frame's ht / lt
    bytes still lie"""
    return "".join("S" if (i % 16 + i // 16) % 2 == 0 else "NH"[i // 16 % 2] for i in range(n))


def pinned_pattern(n):
    """side-by-side page-locked blocks: every third frame TSDF-only (breaks the runs that go up in one copy)"""
    return "".join("H" if i % 6 == 5 else "SSN"[i % 3] for i in range(n))


# group members (scene, pattern over 8 frames): all S; all N (segm_live stays 0 beside live members); alternating
GROUP = [("room", "S" * 8), ("sphere", "N" * 8), ("wall", "SN" * 4)]
# framecast chunks of 3: every chunk mixes S and N
FRAMECAST = "SNSNSSNSN" + "SN"


def semantic_frames(scene, n, scale=0.25, **kw):
    """n synthetic frames, each with ht / lt of its own (lt = 1 - ht, both within [0.01, 0.99])"""
    frames = synthetic.stream(scene, n, scale=scale, noise=True, holes=True, **kw)
    for i, f in enumerate(frames):
        ht = np.roll(f["ht"], (5 * i, 11 * i), axis=(0, 1))
        f["ht"] = np.ascontiguousarray(ht, dtype=np.float32)
        f["lt"] = (np.float32(1.0) - f["ht"]).astype(np.float32)
    return frames


def apply(frames, pattern):
    """the frames as the pattern gives them: ht / lt set to None where the pattern says so"""
    assert len(frames) == len(pattern) and set(pattern) <= set("SNH"), pattern
    out = []
    for f, k in zip(frames, pattern):
        out.append(dict(f, ht=f["ht"] if k in "SH" else None, lt=f["lt"] if k == "S" else None))
    return out


def wrong_patterns(pattern):
    """the patterns a plausible bug would integrate instead (those that differ from the right one)"""
    alts = {"N" * len(pattern), pattern[:1] + pattern[:-1], "S" * len(pattern)}
    tsdf_only = lambda p: p.replace("H", "N")
    return sorted(a for a in alts if tsdf_only(a) != tsdf_only(pattern))


def oracle_run(engine, frames, md):
    for f in frames:
        engine.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], md, f["intrinsics"], f["pose"])


def prob_gap(a, b):
    """largest probability difference of two maps with the same directory (the pattern never changes the TSDF part)"""
    ea, ba = a.dump_directory()
    eb, bb = b.dump_directory()
    assert np.array_equal(ea, eb) and np.array_equal(ba, bb)
    _, _, pa = a.dump_voxels(ba["idx"])
    _, _, pb = b.dump_voxels(bb["idx"])
    return float(np.max(np.abs(pa - pb))) if pa.size else 0.0


def distinguishes(make_oracle, frames, pattern, vs, md, **kw):
    """{wrong pattern: largest probability difference from the right map} over the frame-by-frame oracle"""
    right = make_oracle(vs, 6 * vs, **kw)
    oracle_run(right, apply(frames, pattern), md)
    gaps = {}
    for alt in wrong_patterns(pattern):
        wrong = make_oracle(vs, 6 * vs, **kw)
        oracle_run(wrong, apply(frames, alt), md)
        gaps[alt] = prob_gap(right, wrong)
        wrong.close()
    right.close()
    return gaps
