"""tests/proj_cases.py without a GPU: every family reaches what it is named for (counted on the numpy restatement of
the oracle's projection and visibility test), and the restatement is pinned to the oracle case by case -- the blocks go
into an oracle engine, frame 0 follows, and the frame statistics, the colour bytes of the weight-0 voxels and the
untouched blocks must be what the restatement says.  The HIP engine meets the same cases in
tests/test_gpu_proj_cases.py."""
import numpy as np
import pytest

import proj_cases as pc
from fuse_ref import dump_set
from proj_cases import F


def _halves(pr, H, W):
    return int(pc.exact_halves(pr.proj.qu).sum()), int(pc.exact_halves(pr.proj.qv).sum())


# ---------------------------------------------------------------------------------------------------------------------
# the premises, on the restatement
def test_pixel_colours_name_the_pixel():
    for W, H in ((160, 120), (161, 121)):
        c = pc.pixel_colours(W, H, 1).astype(np.int64)
        word = c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16)
        assert (word[:, 1:] != word[:, :-1]).all() and (word[1:] != word[:-1]).all()    # adjacent pixels
        for cx2, cy2 in ((159, 119), (160, 120), (180, 128)):                            # 2 cx, 2 cy of the cases
            v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            mu, mv = cx2 - u, cy2 - v
            ok = (mu >= 0) & (mu < W) & (mv >= 0) & (mv < H) & ((mu != u) | (mv != v))
            assert (word[v[ok], u[ok]] != word[mv[ok], mu[ok]]).all()                    # point-mirrored pixels


@pytest.mark.parametrize("rot", list(pc.HALVES_ROT))
def test_halves_reach_exact_halves_and_every_border_class(rot):
    cs = pc.halves(rot)
    fr = cs.frames[0]
    H, W = fr.shape
    pr = pc.predict(cs.blocks[0][:cs.n_crafted], fr)
    hu, hv = _halves(pr, H, W)
    cls = pc.border_classes(pr.proj, W, H)
    print(f"{cs.name}: {len(cs.blocks[0])} blocks ({cs.n_crafted} crafted), exact halves {hu} in u, {hv} in v; {cls}")
    assert hu >= 1000 and hv >= 1000
    assert all(n >= 32 for n in cls.values()), cls
    # exact halves that UPDATE, on both sides of zero and at the far borders: the pick's rounding decides a colour there
    upd_half = pr.upd & (pc.exact_halves(pr.proj.qu) | pc.exact_halves(pr.proj.qv))
    assert upd_half.sum() >= 1000
    # -0.5 rounds away from the image, W - 0.5 too: the voxels of those four classes do not update
    with np.errstate(invalid="ignore"):
        out = (pr.proj.qu == F(-0.5)) | (pr.proj.qu == F(W - 0.5)) | (pr.proj.qv == F(-0.5)) | (pr.proj.qv == F(H - 0.5))
        inside = ((pr.proj.qu > F(-0.5)) & (pr.proj.qu < 0)) & (pr.proj.qv > 0) & (pr.proj.qv < H - 1)
    assert not (pr.upd & out).any() and (pr.upd & inside).sum() >= 32
    # the rotation is exact: the camera-space picture is the identity pose's
    if rot != "identity":
        base = pc.halves("identity")
        p0 = pc.project(base.blocks[0][:base.n_crafted], base.frames[0])
        assert sorted(zip(pr.proj.qu.ravel().tolist(), pr.proj.qv.ravel().tolist())) == \
            sorted(zip(p0.qu.ravel().tolist(), p0.qv.ravel().tolist()))
        q = np.array(fr.pose[:4])
        assert (q[:3] != 0).any()


@pytest.mark.parametrize("side", list(pc.BORDER_SIDES))
def test_border_corners_on_and_just_outside_a_bound(side):
    axis, bound = pc.BORDER_BOUND[side]
    on, moved = pc.borders(side, False), pc.borders(side, True)
    edge = on.blocks[0][:2]
    assert np.array_equal(edge, moved.blocks[0][:2]) and np.array_equal(edge, np.array(pc.BORDER_SIDES[side][4]))
    c_on, c_off = pc.corners(edge, on.frames[0]), pc.corners(edge, moved.frames[0])
    H, W = on.frames[0].shape
    assert bound == (W - 1 if side == "uW" else H - 1 if side == "vH" else 0)
    for b in range(2):
        at = np.flatnonzero(c_on.inview[b])
        assert len(at) == 1, f"{side}: block {edge[b].tolist()} has {len(at)} corners in view"
        q_on, q_off = getattr(c_on, axis)[b, at[0]], getattr(c_off, axis)[b, at[0]]
        assert q_on == F(bound)
        assert not c_off.inview[b].any()
        miss = float(q_off) - bound
        assert 0 < abs(miss) < 2.0 ** -10 and (miss < 0) == (bound == 0), miss
        other = "v" if axis == "u" else "u"
        lim = (H if axis == "u" else W) - 1
        assert 0 < getattr(c_off, other)[b, at[0]] < lim and c_off.z[b, at[0]] > 0   # nothing else keeps it out
        print(f"{side}: block {edge[b].tolist()} corner {at[0]} at {axis} = {q_on!r}, moved: {q_off!r}")
    assert pc.visible(edge, on.frames[0]).all() and not pc.visible(edge, moved.frames[0]).any()
    # the second frame of either case is the other's first pose
    assert on.frames[1].pose == moved.frames[0].pose and moved.frames[1].pose == on.frames[0].pose


def test_corners_in_the_camera_plane():
    cs = pc.borders_camera_plane()
    fr = cs.frames[0]
    c = pc.corners(cs.blocks[0][:4], fr)
    assert ((c.z == 0).sum(axis=1) == 4).all() and (c.z <= 0).all() and not c.inview.any()
    assert np.isnan(c.u[0]).any() and np.isinf(c.u).any()      # 0 / 0 on the axis, x / 0 beside it
    assert not pc.visible(cs.blocks[0][:4], fr).any() and pc.visible(cs.blocks[0][4:cs.n_crafted], fr).all()
    assert pc.visible(cs.blocks[0][:4], cs.frames[2]).sum() == 0  # (behind the camera without the move, too)


def test_a_block_that_fills_the_image_is_not_visible():
    cs = pc.borders_fill()
    for fr in cs.frames:
        c = pc.corners([pc.FILL_BLOCK], fr)
        pr = pc.predict([pc.FILL_BLOCK], fr)
        H, W = fr.shape
        print(f"{cs.name}: corners at v = {sorted(set(c.v[0].tolist()))}; {int(pr.proj.inb.sum())} voxels project into the image")
        assert not c.inview.any() and (c.z > 0).all()
        far = c.z[0] == c.z[0].max()
        assert ((c.u[0] > 0) & (c.u[0] < W - 1))[far].all()        # the far corners: in the columns, just outside the rows
        assert (np.minimum(np.abs(c.v[0]), np.abs(c.v[0] - (H - 1)))[far] < 1.5).all()
        assert pr.proj.inb.sum() >= 100 and not pr.vis[0] and not pr.upd.any()
    assert pc.visible(cs.blocks[0][1:], cs.frames[0]).all()


def test_plane_b_has_mixed_pairs_and_the_voxel_at_the_camera_centre():
    cs = pc.plane("b")
    for i, fr in enumerate(cs.frames):
        pr = pc.predict(cs.blocks[0], fr)
        n = pc.mixed_pairs(pr.proj)
        z0 = pr.proj.pcz == 0
        odd = np.broadcast_to((pc.VI & 1).astype(bool)[None, :], z0.shape)
        centre = z0 & np.isnan(pr.proj.qu) & np.isnan(pr.proj.qv)
        print(f"{cs.name} frame {i}: {n} lane pairs with one voxel at pc.z == 0 (the pair's {'second' if odd[z0].all() else 'first'}"
              f" voxel); {int(centre.sum())} voxel at 0 / 0")
        assert n >= 32
        # frame 0: the voxel at 0 is the pair's second, its first is a safe divisor; frame 1 the other way round
        assert odd[z0].all() if i == 0 else not odd[z0].any()
        assert centre.sum() == 1 and (pr.k[centre] == 0).all() and pr.proj.inb[centre].all() and pr.upd[centre].all()
        assert 0 < fr.depth[0, 0] <= fr.md
        # every other voxel of the camera plane has an infinite quotient and picks nothing
        assert not pr.proj.inb[z0 & ~centre].any()


@pytest.mark.parametrize("sub", "abc")
def test_plane_poses(sub):
    cs = pc.plane(sub)
    q, t = cs.frames[0].pose[:4], cs.frames[0].pose[4:]
    pr = pc.project(cs.blocks[0][:cs.n_crafted], cs.frames[0])
    assert (pr.pcz < 0).any() and (pr.pcz > 0).any()
    if sub == "a":
        assert q == pc.IDENTITY and t[2] == -float(F(28) * F(cs.vs))
    if sub == "c":
        assert abs(2 * np.degrees(np.arccos(q[3])) - 10) < 1e-6
        assert all(float(F(x) * F(2 ** 20)) != round(float(F(x) * F(2 ** 20))) for x in t)


@pytest.mark.parametrize("name", list(pc.OBLIQUE))
def test_oblique_cases_have_voxels_inside_the_image_by_rounding_alone(name):
    cs = pc.oblique(name)
    K, q, _ = pc.OBLIQUE[name]
    for i, fr in enumerate(cs.frames):
        H, W = fr.shape
        n = pc.near_borders(pc.project(cs.blocks[0], fr), W, H)
        print(f"{cs.name} frame {i}: {len(cs.blocks[0])} blocks, {n} voxels in (-0.5, 0) or [W - 1, W - 0.5) on some axis")
        assert n >= 100
    assert K[0] != K[1]
    if name == "norm1.001":
        assert abs(np.linalg.norm(q) - 1.001) < 1e-5
    if name == "outside-y37":
        assert K[2] < 0
    if name.startswith("grid-end"):
        bx = cs.blocks[0][:cs.n_crafted, 0]
        assert ((bx == 4095).sum() >= 8 and (bx > 4000).all()) if name.endswith("+") else ((bx == -4096).sum() >= 8 and (bx < -4000).all())
        g = pc.block_voxels(cs.blocks[0][:cs.n_crafted])[:, 0]
        assert (g.max() == 32767) if name.endswith("+") else (g.min() == -32768)


@pytest.mark.parametrize("which", list(pc.FAR_TZ))
def test_far_cases_stand_on_their_side_of_the_guard(which):
    cs = pc.far(which)
    lim = F(1e18)
    for fr, w in zip(cs.frames, pc.FAR_ORDER[which]):
        pr = pc.predict(cs.blocks[0], fr)
        assert ((np.abs(pr.proj.pcz) < lim).all() if w == "below" else (np.abs(pr.proj.pcz) >= lim).all())
        assert pr.vis.all() and not pr.upd.any()
        assert (pr.proj.iu == 80).all() and (pr.proj.iv == 60).all()
        d = fr.depth.reshape(-1)[pr.k]
        assert ((d > 0) & (d <= fr.md)).all()   # the depth is valid: it is the distance that keeps the voxels out


def test_sizes():
    for _, fn, a in pc.ALL:
        cs = fn(*a)
        assert 2 <= len(cs.frames) <= 3 and len(cs.blocks[0]) <= 200, (cs.name, len(cs.blocks[0]))
        assert all(fr.shape in ((120, 160), (121, 161)) for fr in cs.frames)
        assert len(np.unique(pc.keys(cs.blocks[0]))) == len(cs.blocks[0])
        w = cs.blocks[2]["weight"]
        assert 0.5 < (w == 0).mean() < 0.8 or cs.family == "far"


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against the oracle
@pytest.mark.parametrize("fam,fn,a", pc.ALL, ids=pc.IDS)
def test_the_oracle_does_what_the_restatement_says(fam, fn, a, make_oracle):
    cs = fn(*a)
    fr = cs.frames[0]
    cpu = make_oracle(cs.vs, cs.trunc, threads=4, **pc.CFG)
    cpu.import_blocks(*cs.blocks)
    before = pc.by_position(dump_set(cpu))
    assert pc.words(before).tobytes() == pc.words(pc.by_position(cs.blocks)).tobytes()
    cpu.integrate(*fr.args())
    st = cpu.last_frame_stats()
    pr = pc.predict(before[0], fr)
    print(f"{cs.name}: visible {st['visible_blocks']} of {len(before[0])} blocks, {st['updated_voxels']} voxels updated, "
          f"{st['deleted_blocks']} blocks carved")
    assert st["allocated_blocks"] == 0, "frame 0 allocates: the guard blocks do not cover its candidates"
    assert st["visible_blocks"] == int(pr.vis.sum())
    assert st["updated_voxels"] == int(pr.upd.sum())
    after = pc.by_position(dump_set(cpu))
    at, held = pc.align(after, before)          # rows of `after` for the blocks of `before`; carved blocks are gone
    assert held.sum() == len(after[0]) == len(before[0]) - st["deleted_blocks"] and pr.vis[~held].all()
    # a weight-0 voxel that updates holds exactly the restated pixel's colour
    zero = pr.upd & (before[2]["weight"] == 0) & held[:, None]
    rgb = fr.rgb.reshape(-1, 3)[pr.k]
    got = after[2][at]
    for j, ch in enumerate("rgb"):
        bad = zero & (got[ch] != rgb[..., j])
        assert not bad.any(), f"{cs.name}: {int(bad.sum())} voxels hold another pixel's {ch}"
    assert zero.sum() >= (0 if fam == "far" else 500 if cs.name != "borders/fill" else 0)
    # what the restatement says does not update is unchanged bit for bit: whole invisible blocks among it
    wb, wa = pc.words(before), pc.words(after, at)
    changed = (wb != wa).any(axis=-1) & held[:, None]
    assert not (changed & ~pr.upd).any()
    assert (changed | ~pr.upd | ~held[:, None]).all() or fam == "far"  # (an update changes at least the weight or a colour)
    if fam == "far":
        verdict = np.isin(pc.keys(cs.blocks[0][:4]), pc.keys(after[0]))
        assert verdict.tolist() == [False, True, False, True], "the carve verdicts fall on the priors alone"
        assert st["deleted_blocks"] == 2
    if cs.name == "borders/fill":
        i = int(np.flatnonzero(pc.keys(before[0]) == pc.keys([pc.FILL_BLOCK])[0])[0])
        assert not pr.vis[i] and wb[i].tobytes() == wa[i].tobytes()


def test_the_oracle_updates_voxels_behind_the_camera_through_the_mirrored_pixel(make_oracle):
    """the reference's behaviour, kept: a voxel with pc.z < 0 in a visible block picks the pixel its point mirror
    projects to.  Per sub-case, counted on the oracle's own map"""
    total, astride = 0, 0
    for sub in "abc":
        cs = pc.plane(sub)
        fr = cs.frames[0]
        cpu = make_oracle(cs.vs, cs.trunc, threads=4, **pc.CFG)
        cpu.import_blocks(*cs.blocks)
        before = pc.by_position(dump_set(cpu))
        cpu.integrate(*fr.args())
        after = pc.by_position(dump_set(cpu))
        at, held = pc.align(after, before)
        pr = pc.predict(before[0], fr)
        mir = pc.mirrored_pixel(pr.proj, fr)
        word = lambda c: c["r"].astype(np.int64) | (c["g"].astype(np.int64) << 8) | (c["b"].astype(np.int64) << 16)
        pixel = lambda k: (fr.rgb.reshape(-1, 3)[k].astype(np.int64) * (1, 256, 65536)).sum(axis=-1)
        got = word(after[2][at])
        changed = (pc.words(before) != pc.words(after, at)).any(axis=-1) & held[:, None]
        behind = changed & (pr.proj.pcz < 0) & (before[2]["weight"] == 0)
        assert (got[behind] == pixel(pr.k)[behind]).all()
        differs = behind & ((mir < 0) | (got != pixel(np.maximum(mir, 0))))
        both = (pr.proj.pcz < 0).any(axis=1) & (pr.proj.pcz > 0).any(axis=1) & pr.vis & changed.any(axis=1)
        print(f"{cs.name}: the oracle updated {int((changed & (pr.proj.pcz < 0)).sum())} voxels behind the camera; "
              f"{int(differs.sum())} of weight 0 hold the mirrored pixel's colour and not the unmirrored one's; "
              f"{int(both.sum())} visible blocks astride the camera plane")
        assert differs.sum() >= 100 and both.sum() >= 2
        total, astride = total + int(differs.sum()), astride + int(both.sum())
    assert total >= 200 and astride >= 8
