"""The host-result entry points of ONE engine share one staging pair (device memory and its page-locked twin): every
one of them run back to back on the same engine, in one order, in the reverse order and a gather once more, each
result checked byte for byte.  A call's bytes must not depend on which calls came before it -- what an earlier call
left in the pair, how large either side has grown, where it laid out its parts.

The map is tiny_table of tests/readout_cases.py: a small directory, chained blocks, and the map of a sample set, an
ESDF box and a surface box alike.  Samples, ESDF, surface points, the welded surface mesh, gathers and the query are
checked against the restatements of the per-feature tests, which never ask an engine.  The ray cast and the mesh have
no restatement for this map: they are compared with the same call made first on a second engine that holds the same
map and has made no other call.

Marching cubes reads only voxels of weight above 10 and the ray cast only those of 10 or more, and tiny_table's
weights are 0 .. 3: on that map the mesh is empty (its three downloads are never made) and no ray hits.  The test
therefore runs twice: on tiny_table as it is, and on tiny_table_heavy, the same blocks with every observed voxel's
weight raised by 10 (an unobserved voxel stays unobserved), where the mesh has triangles and the view hits (on the CPU
oracle: 30 248 triangles, 39 % of the pixels).  The ESDF looks only at "weight 0 or not": its expectation is the same for
both.  The others are restated from the heavier BlockSet by the functions readout_cases.expected_* are made of.

The welded mesh (ratsdf_surface_mesh, whose host form sizes the same pair for vertices and triangles side by side) is
taken over the surface box and compared with tests/surface_mesh_ref.py.  tiny_table's weights leave no cell of eight
observed corners, in either map: the restatement's mesh is empty, so the call runs its count pass and reads its two
totals between the other calls and must hand back two empty lists whatever they left in the pair.  A welded mesh WITH
triangles comes at the end: a small sphere is imported far from everything the other calls read, and its mesh is taken
between samples, ESDF and surface points, each still checked against its restatement."""
import functools

import numpy as np
import pytest

import query_cases as qc
import raycast_cases
import readout_cases as rc
import sample_ref
import surface_mesh_ref
import surface_ref
from ratsdf._abi import SAMPLE_ALLOCATED

pytestmark = pytest.mark.gpu

POINTS = "tiny_table_jitter"
ESDF_BOX = "tiny_table_obs"
SURFACE_BOX = next(s for s in rc.SURFACE_BOXES if s[0] == "tiny_table")
ONE_BLOCK = qc.Case("one_block", qc.voxel_box((-8, -1), (0, 7), (-16, -9)), (-8, -1, 0, 7, -16, -9), 1)   # (-1, 0, -2)
# 50 x 77 pixels, from 60 voxels in front of the blocks (they span voxels -24 .. 23), looking along +z
# a sphere in the blocks 20 .. 21 (tiny_table spans blocks -3 .. 2), every voxel observed, and the box around it
BALL = dict(centre=(167.6, 168.3, 167.2), radius=4.7, lo=(20, 20, 20), hi=(21, 21, 21))
BALL_BOX = ((159, 158, 159), (18, 19, 18))
VIEW = (raycast_cases.centred(60, 50, 77), 50, 77, raycast_cases.look((0.0, 0.0, -84.0)), 4.0)


@functools.lru_cache(maxsize=None)
def _map(name):
    m = rc.tiny_table()
    if name == "tiny_table":
        return m
    b = m.blocks
    rgbw = b.rgbw.copy()
    rgbw["weight"] = np.where(b.rgbw["weight"] > 0, b.rgbw["weight"] + 10, 0)
    return rc.Map(name, raycast_cases.BlockSet(b.pos, b.tsdf, rgbw, b.prob), m.engine)


@functools.lru_cache(maxsize=None)
def _expected(name):
    """(samples, surface points, welded mesh) of the map: computed once, shared, never changed"""
    m, ps = _map(name), rc.point_set(POINTS)
    _, _, origin, dims, _ = SURFACE_BOX
    if name == "tiny_table":
        samples = rc.expected_samples(POINTS)
    else:
        samples = sample_ref.sample(ps.points, rc.VS, rc.blockset_lookup(m.blocks))
    surface = surface_ref.surface_points(surface_ref.blocks_of(*m.blocks), origin, dims, rc.VS, 1, 0.0)
    mesh = surface_mesh_ref.surface_mesh(surface_ref.blocks_of(*m.blocks), origin, dims, rc.VS, 1)
    for a in (samples, surface) + mesh:
        a.setflags(write=False)
    return samples, surface, mesh


def _same(got, want, what):
    for g, w in zip(got, want):
        assert qc.same_bytes(g, w), f"{what}: differs from the call on the engine that made no other"


@pytest.mark.parametrize("name", ["tiny_table", "tiny_table_heavy"])
def test_every_host_result_through_one_staging_pair(name, make_engine, tmp_path):
    m, ps, box = _map(name), rc.point_set(POINTS), rc.box(ESDF_BOX)
    assert ps.map.name == box.map == SURFACE_BOX[1] == "tiny_table"
    want_samples, want_surface, want_surface_mesh = _expected(name)
    _, _, s_origin, s_dims, least = SURFACE_BOX
    # the map is not trivial for any of the read-outs
    assert ((want_samples["flags"] & SAMPLE_ALLOCATED) != 0).sum() > len(want_samples) // 4
    assert len(want_surface) >= least

    fresh, e = (make_engine(rc.VS, rc.TRUNC, **m.engine) for _ in range(2))
    for eng in (fresh, e):
        rc.load(eng, m)
    d = qc.directory_of(e, m)
    want20 = qc.expected(m.blocks, d[0], d[1], True, None, rc.VS)
    # the ray cast and the mesh of an engine that makes no other host-result call
    want_images = fresh.raycast(*VIEW)
    want_mesh = fresh.gather_valid_mesh()
    heavy = name == "tiny_table_heavy"
    assert (len(want_mesh[1]) > 0) == heavy, "triangles: with weights above 10, and only then"
    # (the blocks fill 48 x 48 of the 76 x 50 voxels the view spans at their front face)
    assert (raycast_cases.hit_share(want_images[0]) > 0.2) == heavy, "hits: with weights of 10 or more, and only then"

    def gather_semantic(tag):
        qc.assert_same(e.gather_valid_semantic(), want20, f"{tag}: gather_valid_semantic")

    def raycast(tag):
        _same(e.raycast(*VIEW), want_images, f"{tag}: raycast")

    def sample_set(tag):
        rc.assert_samples(e.sample_points(ps.points), want_samples, f"{tag}: sample_points", ps.nan_allowed)

    def esdf(tag):
        got, st = e.esdf(box.origin, box.dims, box.occupied_below, box.unknown_occupied, with_state=True)
        assert qc.same_bytes(st, rc.expected_state(box.name)), f"{tag}: esdf state"
        assert qc.same_bytes(got, rc.expected_field(box.name)), f"{tag}: esdf"

    def surface(tag):
        got = e.surface_points(s_origin, s_dims, 1, 0.0)
        assert surface_ref.same_bytes(got, want_surface), (tag, len(got), len(want_surface))

    def surface_mesh(tag):
        v, tri = e.surface_mesh(s_origin, s_dims, 1)
        assert tri.dtype == np.int32 and tri.shape == want_surface_mesh[1].shape, (tag, tri.shape)
        assert np.array_equal(tri, want_surface_mesh[1]), tag
        assert surface_ref.same_bytes(v, want_surface_mesh[0]), (tag, len(v), len(want_surface_mesh[0]))

    def mesh(tag):
        _same(e.gather_valid_mesh(), want_mesh, f"{tag}: gather_valid_mesh")

    def query(tag):
        assert qc.check_query(e, m.blocks, ONE_BLOCK, d, tag) == 512

    def sample_one(tag):
        at = len(ps.points) // 2
        rc.assert_samples(e.sample_points(ps.points[at:at + 1]), want_samples[at:at + 1], f"{tag}: one point",
                          ps.nan_allowed)

    calls = (gather_semantic, raycast, sample_set, esdf, surface, surface_mesh, mesh, query, sample_one)
    for k, call in enumerate(calls):
        call(f"{name}, forward {k + 1}")
    for k, call in reversed(list(enumerate(calls))):
        call(f"{name}, backward {k + 1}")
    qc.check_gathers(e, m.blocks, d, tmp_path / "all.bin", f"{name}, at the end")

    # once more around a welded mesh that has triangles
    ball = surface_mesh_ref.sphere_blocks(BALL["centre"], BALL["radius"], BALL["lo"], BALL["hi"])
    want_ball = surface_mesh_ref.surface_mesh(surface_ref.blocks_of(*ball), *BALL_BOX, rc.VS, 1)
    assert len(want_ball[0]) > 200 and len(want_ball[1]) > 400
    surface_mesh_ref.assert_closed(want_ball[1], len(want_ball[0]))
    e.import_blocks(*ball)

    def ball_mesh(tag):
        v, tri = e.surface_mesh(*BALL_BOX, 1)
        assert tri.dtype == np.int32 and tri.shape == want_ball[1].shape and np.array_equal(tri, want_ball[1]), tag
        assert surface_ref.same_bytes(v, want_ball[0]), (tag, len(v), len(want_ball[0]))

    for k, call in enumerate((ball_mesh, sample_set, ball_mesh, esdf, surface, ball_mesh, surface_mesh, sample_one,
                              ball_mesh)):
        call(f"{name}, with the sphere {k + 1}")
