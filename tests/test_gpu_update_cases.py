"""The frame update of the HIP engine (k_integrate: integrate_block / finish_block) on the crafted prior voxels of
tests/update_cases.py: the same blocks go into a HIP engine and an oracle engine with import_blocks, the same frames
follow, and the maps are compared after every frame (after the batch, where the frames go as one batch).
tests/test_update_cases.py shows without a GPU that the cases hold what they are for and that the oracle follows the
reference's formula.

The bars: live block positions and the frame statistics equal; weight and colour exact; tsdf NaN in the same voxels,
+-inf in the same voxels with the same sign, bit for bit wherever the oracle's result is zero or normal, within
parity.TOL where it is subnormal; the probability NaN in the same voxels, else within parity.TOL, and exactly 0 or 1 in
the same voxels where the prior or the pixel's ht / lt is exactly 0 or 1; a voxel that a frame does not update keeps
all three words bit for bit.

Observed on an MI355X (printed by the tests): see DESIGN.md 4 "Frames onto imported voxels".
"""
import numpy as np
import pytest

import update_cases as uc
from fuse_ref import contributes, dump_set
from parity import TOL, assert_directory_equal, assert_heap_equal, assert_pool_consistent, assert_stats_equal
from update_cases import F

pytestmark = pytest.mark.gpu


def import_case(engines, cs):
    for e in engines:
        e.import_blocks(*cs.blocks)
        got = uc.by_position(dump_set(e))
        assert uc.words(got).tobytes() == uc.words(uc.by_position(cs.blocks)).tobytes(), "the imported map is not the crafted one"


def same_pools(gpu, cpu):
    """True when both engines name the same pool blocks (then every word can be compared, stale colours of fresh
    blocks included); otherwise the comparison goes by position"""
    try:
        assert_directory_equal(gpu, cpu)
        assert_heap_equal(gpu, cpu)
        return True
    except AssertionError:
        return False


def compare(gpu, cpu, what, alive, prior=None, fr=None, predict=uc.predict):
    """the HIP engine's map against the oracle's at the bars of the module docstring; alive: keys of the imported blocks
    that never left the map (every colour byte of theirs is known); prior (the oracle's map before the frame) and fr:
    the frame whose 0 / 1 probabilities are looked at; predict: the restatement of the case module the frame comes from
    (update_cases or proj_cases).  Returns the figures."""
    assert_pool_consistent(gpu)
    strict = same_pools(gpu, cpu)
    g, o = uc.by_position(dump_set(gpu)), uc.by_position(dump_set(cpu))
    assert len(g[0]) == len(o[0]) and np.array_equal(g[0], o[0]), f"{what}: live block positions differ"

    def show(bad):
        """the first few voxels of `bad`: what they held, what the frame brought, what both engines made of it"""
        if prior is None:
            return ""
        at, held = uc.align(prior, o)
        pr = predict(o[0], fr)
        out = []
        for b, v in np.argwhere(bad)[:6]:
            was = (f"held tsdf {prior[1][at[b], v]!r} rgbw {prior[2][at[b], v]} p {prior[3][at[b], v]!r}" if held[b]
                   else "fresh")
            k = pr.k[b, v]
            sem = "" if fr.ht is None else f" ht {fr.ht.reshape(-1)[k]!r} lt {fr.lt.reshape(-1)[k]!r}"
            out.append(f"block {o[0][b].tolist()} voxel {v}: {was}; updates {bool(pr.upd[b, v])} ts {pr.ts[b, v]!r} wn "
                       f"{pr.wn[b, v]!r} rgb {fr.rgb.reshape(-1, 3)[k].tolist()}{sem}; engine {g[1][b, v]!r} {g[2][b, v]} "
                       f"{g[3][b, v]!r}, oracle {o[1][b, v]!r} {o[2][b, v]} {o[3][b, v]!r}")
        return "\n  " + "\n  ".join(out)
    bad = g[2]["weight"] != o[2]["weight"]
    assert not bad.any(), f"{what}: weights differ in {int(bad.sum())} voxels{show(bad)}"
    # colours: every voxel, unless the pools are named differently -- then a fresh block's never-updated voxels hold
    # whatever colour its pool block had (AquireBlock leaves it), and only those are left out: every voxel of a block
    # that has been in the map since the import is compared, weight 0 or not
    known = np.ones(o[1].shape, bool) if strict else contributes(o[1], o[2]) | np.isin(uc.keys(o[0]), alive)[:, None]
    for ch in ("r", "g", "b"):
        bad = (g[2][ch] != o[2][ch]) & known
        assert not bad.any(), f"{what}: colour {ch} differs in {int(bad.sum())} voxels{show(bad)}"
    gt, ot = g[1], o[1]
    gn, on = np.isnan(gt), np.isnan(ot)
    assert np.array_equal(gn, on), f"{what}: tsdf NaN in {int(gn.sum())} voxels, the oracle's in {int(on.sum())}{show(gn != on)}"
    inf = np.isinf(ot)
    assert np.array_equal(np.isinf(gt), inf) and np.array_equal(gt[inf], ot[inf]), f"{what}: tsdf infinities differ"
    sub = (ot != 0) & (np.abs(ot) < F(uc.FLT_MIN))
    exact = ~on & ~sub
    bad = exact & (uc.bits(gt) != uc.bits(ot))
    assert not bad.any(), f"{what}: tsdf differs in {int(bad.sum())} voxels where the oracle's is zero or normal{show(bad)}"
    fin = ~on & ~inf
    dt = float(np.abs(gt[fin].astype(np.float64) - ot[fin].astype(np.float64)).max())
    assert not sub.any() or np.abs(gt[sub] - ot[sub]).max() <= TOL
    gp, op = g[3], o[3]
    gpn, opn = np.isnan(gp), np.isnan(op)
    assert np.array_equal(gpn, opn), (f"{what}: probability NaN in {int(gpn.sum())} voxels, the oracle's in "
                                      f"{int(opn.sum())}{show(gpn != opn)}")
    with np.errstate(invalid="ignore"):
        d = np.abs(np.where(opn, F(0), gp) - np.where(opn, F(0), op))
    dp = float(np.nanmax(d))  # (inf against inf: NaN, and equal)
    assert np.array_equal(np.isinf(gp), np.isinf(op)) and np.array_equal(gp[np.isinf(op)], op[np.isinf(op)])
    assert dp <= TOL, f"{what}: probability differs by {dp}{show(d > TOL)}"
    n01 = 0
    if prior is not None and fr.ht is not None:
        at, held = uc.align(prior, o)
        pr = predict(o[0][held], fr)
        p0 = prior[3][at[held]]
        h, l = fr.ht.reshape(-1)[pr.k], fr.lt.reshape(-1)[pr.k]
        sel = pr.upd & ((p0 == 0) | (p0 == 1) | (h == 0) | (h == 1) | (l == 0) | (l == 1))
        for v in (F(0), F(1)):
            assert np.array_equal((gp[held] == v)[sel], (op[held] == v)[sel]), f"{what}: probability exactly {v} in other voxels"
            n01 += int((op[held] == v)[sel].sum())
    figures = dict(tsdf=dt, prob=dp, subnormal=int(sub.sum()), exact01=n01, strict=strict)
    print(f"{what}: {len(o[0])} blocks; worst tsdf difference {dt:.3e}, worst probability difference {dp:.3e}, "
          f"{figures['subnormal']} subnormal tsdf results, {n01} probabilities exactly 0 or 1 looked at"
          f"{'' if strict else '; compared by position'}")
    return figures


STATS = ("visible_blocks", "updated_voxels", "allocated_blocks", "deleted_blocks", "active_blocks")


def still_alive(alive, cpu):
    """the keys of `alive` whose blocks the oracle's map still holds"""
    _, blocks = cpu.dump_directory()
    return alive[np.isin(alive, uc.keys(np.stack([blocks["x"], blocks["y"], blocks["z"]], axis=1)))]


def frame_by_frame(gpu, cpu, cs, send, what, mod=uc):
    """every frame of the case into both engines (`send` puts frame i into the HIP engine), compared after each.
    mod: the module the case comes from (update_cases, or proj_cases with its own restatement).  Returns the figures
    of every frame."""
    alive = uc.keys(cs.blocks[0])
    figures = []
    for i, fr in enumerate(cs.frames):
        before_g, before_o = dump_set(gpu), dump_set(cpu)
        send(i, fr)
        cpu.integrate(*fr.args())
        assert_stats_equal(gpu, cpu, STATS)
        if mod is uc and i == 1:
            assert gpu.last_frame_stats()["allocated_blocks"] > 0  # fresh and loaded blocks in one launch
        alive = still_alive(alive, cpu)
        assert len(alive) >= (16 if mod is uc else 1)
        figures.append(compare(gpu, cpu, f"{what} frame {i}", alive, before_o, fr, mod.predict))
        uc.untouched_unchanged(before_g, dump_set(gpu), fr, mod.predict)
    assert gpu.totals() == cpu.totals()
    return figures


def upload(cs):
    import torch
    dev = torch.device("cuda", 0)
    out = [{k: torch.from_numpy(np.array(getattr(fr, k))).to(dev) for k in ("rgb", "depth", "ht", "lt")
            if getattr(fr, k) is not None} for fr in cs.frames]
    torch.cuda.synchronize()
    return out


def pointers(d):
    return (d["rgb"].data_ptr(), d["depth"].data_ptr(), d["ht"].data_ptr() if "ht" in d else None,
            d["lt"].data_ptr() if "lt" in d else None)


@pytest.mark.parametrize("pool", uc.POOLS)
def test_frames_from_host_memory(pool, make_engine, make_oracle):
    cs = uc.case(pool)
    gpu, cpu = make_engine(uc.VS, uc.TRUNC, **uc.CFG), make_oracle(uc.VS, uc.TRUNC, threads=4, **uc.CFG)
    import_case((gpu, cpu), cs)
    frame_by_frame(gpu, cpu, cs, lambda i, fr: gpu.integrate(*fr.args()), f"{pool}[integrate]")


@pytest.mark.parametrize("pool", uc.POOLS)
def test_frames_from_device_memory(pool, make_engine, make_oracle):
    cs = uc.case(pool)
    gpu, cpu = make_engine(uc.VS, uc.TRUNC, **uc.CFG), make_oracle(uc.VS, uc.TRUNC, threads=4, **uc.CFG)
    import_case((gpu, cpu), cs)
    dev = upload(cs)
    frame_by_frame(gpu, cpu, cs, lambda i, fr: gpu.integrate_device(*pointers(dev[i]), uc.H, uc.W, uc.MD, uc.INTR, uc.POSE),
                   f"{pool}[integrate_device]")


def batch_of(engine_or_group, devs):
    """the three frames of every member's case as one batch (devs: one upload per member)"""
    one = not isinstance(devs[0], list)
    rows = [[pointers(d[i]) for d in ([devs] if one else devs)] for i in range(3)]
    col = lambda j: [(r[0][j] if one else [m[j] for m in r]) for r in rows]
    wrap = (lambda v: v) if one else (lambda v: [v] * len(devs))
    return engine_or_group.make_batch(col(0), col(1), col(2), col(3), uc.H, uc.W, uc.MD, [wrap(uc.INTR)] * 3,
                                      [wrap(uc.POSE)] * 3)


def after_the_batch(gpu, cpu, cs, what, mod=uc):
    """the oracle takes the case's frames one by one; then the maps are compared.  mod: as in frame_by_frame (the carve
    blocks' verdicts are looked at where the case has them: update_cases)"""
    before_g, before_o = dump_set(gpu), dump_set(cpu)
    alive = uc.keys(cs.blocks[0])
    for i, fr in enumerate(cs.frames):
        cpu.integrate(*fr.args())
        alive = still_alive(alive, cpu)
    assert_stats_equal(gpu, cpu, STATS)
    assert gpu.totals() == cpu.totals()  # (the first frame's carving among them)
    figures = compare(gpu, cpu, what, alive)
    after = dump_set(gpu)
    if mod is uc:
        _, cpos, _, _, verdict = uc.carve_blocks()
        assert np.array_equal(np.isin(uc.keys(cpos), uc.keys(after[0])), ~verdict), f"{what}: the carve blocks' verdicts"
    # what none of the three frames updates keeps its words
    at, held = uc.align(before_g, after)
    upd = np.zeros(after[1][held].shape, bool)
    for fr in cs.frames:
        upd |= mod.predict(after[0][held], fr).upd
    same = (uc.words(before_g, at[held]) == uc.words(after, held)).all(axis=-1)
    assert same[~upd].all() and (~upd).sum() >= 1000, f"{what}: {int((~same & ~upd).sum())} untouched voxels changed"
    return figures


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("pool", uc.POOLS)
def test_a_batch_of_three_frames(pool, graph, monkeypatch, make_engine, make_oracle):
    """the second and third frames update the first's results (its NaN and inf voxels among them); graph "1": one
    replay of a captured graph, "0": every frame launched by itself.  (prob: the middle frame is TSDF-only)"""
    cs = uc.case(pool)
    monkeypatch.setenv("RATSDF_GRAPH", graph)
    gpu, cpu = make_engine(uc.VS, uc.TRUNC, **uc.CFG), make_oracle(uc.VS, uc.TRUNC, threads=4, **uc.CFG)
    monkeypatch.delenv("RATSDF_GRAPH")
    import_case((gpu, cpu), cs)
    dev = upload(cs)
    gpu.integrate_device_batch(batch_of(gpu, dev))
    after_the_batch(gpu, cpu, cs, f"{pool}[batch, RATSDF_GRAPH={graph}]")


def test_a_group_of_two_engines_with_different_maps(make_engine, make_oracle):
    import ratsdf
    cases = [uc.case("tsdf"), uc.case("prob")]
    engines = [make_engine(uc.VS, uc.TRUNC, **uc.CFG) for _ in cases]
    oracles = [make_oracle(uc.VS, uc.TRUNC, threads=4, **uc.CFG) for _ in cases]
    for e, o, cs in zip(engines, oracles, cases):
        import_case((e, o), cs)
    devs = [upload(cs) for cs in cases]
    group = ratsdf.Group(engines)
    try:
        group.integrate_device_batch(batch_of(group, devs))
        group.synchronize()
        for e, o, cs in zip(engines, oracles, cases):
            after_the_batch(e, o, cs, f"{cs.pool}[group of two]")
    finally:
        group.close()


def one_voxel_per_lane(make_engine, make_oracle, pools=("weights", "tsdf")):
    """the weight, tsdf and carve pools frame by frame (tests/diagnostic_build_cases.py: RATSDF_VPL=1, the scalar loop
    the packed path is written against; the carve blocks are part of every case)"""
    for pool in pools:
        cs = uc.case(pool)
        gpu, cpu = make_engine(uc.VS, uc.TRUNC, **uc.CFG), make_oracle(uc.VS, uc.TRUNC, threads=4, **uc.CFG)
        import_case((gpu, cpu), cs)
        frame_by_frame(gpu, cpu, cs, lambda i, fr: gpu.integrate(*fr.args()), f"{pool}[one voxel per lane]")
