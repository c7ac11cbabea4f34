"""The crafted value cases of tests/surface_cases.py on the HIP engine: every set through ratsdf_surface_points,
ratsdf_surface_points_device, ratsdf_surface_mesh and ratsdf_surface_mesh_device, against the numpy restatements fed
from the BlockSet (tests/surface_ref.py, tests/surface_mesh_ref.py).  Records compare byte for byte; the one exception
is pos[a] of a record whose f is NaN, where both sides must be NaN (surface_cases.exempt: capped and counted in
tests/test_surface_cases.py).  One small engine per set."""
import numpy as np
import pytest

import surface_cases as sc
import surface_mesh_ref as mref
import surface_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A


def _snapshot(e):
    ei, blocks = e.dump_directory()
    nf, heap = e.dump_heap()
    t, c, p = e.dump_voxels(blocks["idx"])
    return ei, blocks, nf, heap[:nf].copy(), t, c, p


def _same(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y


def _records(words):
    """int32 [n, 8] from a device buffer as surface points"""
    return np.ascontiguousarray(words).view(ref.POINT).reshape(-1)


class _Report:
    def __init__(self, name):
        self.name, self.failed = name, []

    def records(self, got, want, allowed, edges, what):
        n = sc.differing(got, want, allowed)
        print(f"{self.name}, {what}: {len(got)} records, restatement {len(want)}: "
              f"{n if n >= 0 else 'the counts'} records differ")
        if n != 0:
            self.failed.append(what)
            if n > 0:                         # the first one, with what it was made of
                g = np.ascontiguousarray(got).view(ref.POINT).reshape(-1)
                bad = [i for i in range(len(g)) if sc.differing(g[i:i + 1], want[i:i + 1], allowed[i:i + 1])]
                classes = {}
                for i in bad:
                    key = tuple(np.flatnonzero(g[i:i + 1].view(np.uint32).reshape(-1)
                                               != np.ascontiguousarray(want[i:i + 1]).view(np.uint32).reshape(-1)))
                    classes[key] = classes.get(key, 0) + 1
                print(f"  differing words (0-2 pos, 3-5 normal, 6 prob, 7 rgbw) -> records: {classes}")
                for i in bad[:4]:
                    print(f"  record {i}: owner {edges.owner[i]} axis {edges.axis[i]} t0 {edges.t0[i]!r} "
                          f"t1 {edges.t1[i]!r} f {edges.f[i]!r} g {edges.g[i]} len2 {edges.len2[i]!r} "
                          f"len {edges.len[i]!r}"
                          f"\n    got  {g[i]} {g[i:i + 1].view(np.uint32).reshape(-1)}"
                          f"\n    want {want[i]} {np.ascontiguousarray(want[i:i + 1]).view(np.uint32).reshape(-1)}")

    def check(self, ok, what):
        if not ok:
            print(f"{self.name}, {what}: FAILED")
            self.failed.append(what)


@pytest.mark.parametrize("name", sc.CASES)
def test_every_entry_point(name, make_engine):
    from ratsdf import devmem
    c = sc.case(name)
    e = make_engine(sc.VS, sc.TRUNC, **sc.ENGINE)
    e.import_blocks(*c.blocks)
    before = _snapshot(e)
    rep = _Report(name)
    cnt = devmem.DeviceArray(np.full(2, -1, dtype=np.int64))

    # ---- surface points, host and device form
    for mp in c.min_probs:
        want, edges = sc.expected_points(name, mp), sc.expected_edges(name, mp)
        allowed, total = sc.exempt(want, edges), len(want)
        rep.records(e.surface_points(c.origin, c.dims, 1, mp), want, allowed, edges, f"surface_points(min_prob {mp!r})")
        assert e.surface_points_device(c.origin, c.dims, 0, 0, cnt, 1, mp) == total          # a pure count
        for cap in (total, sc.cut_inside_specials(edges)):
            buf = devmem.DeviceArray(np.full((cap + 4, 8), GUARD, dtype=np.int32))
            assert e.surface_points_device(c.origin, c.dims, buf, cap, cnt, 1, mp) == total
            got = buf.numpy()
            rep.records(_records(got[:cap]), want[:cap], allowed[:cap], edges,
                        f"surface_points_device(min_prob {mp!r}, capacity {cap} of {total})")
            rep.check(np.all(got[cap:] == GUARD), f"surface_points_device: nothing beyond capacity {cap}")

    # ---- the welded mesh, host and device form
    want_v, want_t = sc.expected_mesh(name)
    _, sign_t = sc.expected_mesh(name, signs_only=True)
    edges = sc.expected_edges(name, over_mesh=True)
    allowed = sc.exempt(want_v, edges)
    nv, nt = len(want_v), len(want_t)
    v, tri = e.surface_mesh(c.origin, c.dims, 1)
    rep.records(v, want_v, allowed, edges, "surface_mesh vertices")
    rep.check(tri.dtype == np.int32 and tri.shape == want_t.shape and np.array_equal(tri, want_t),
              "surface_mesh triangles")
    rep.check(tri.shape == sign_t.shape and np.array_equal(tri, sign_t), "surface_mesh triangles are the +-1 map's")
    # on the engine's own output: the vertices are a subsequence of its surface points over [origin, origin + dims + 1)
    # (at min_prob -inf, which drops nothing: the mesh has no min_prob and `probabilities` has negative words)
    mref.assert_subsequence(v, e.surface_points(c.origin, [d + 1 for d in c.dims], 1, float("-inf")))
    counts = devmem.DeviceArray(np.full(3, -1, dtype=np.int64))
    assert e.surface_mesh_device(c.origin, c.dims, 0, 0, 0, 0, counts) == (nv, nt)           # a pure count
    assert counts.numpy().tolist() == [nv, nt, -1]
    for vcap, tcap in ((nv, nt), (sc.cut_inside_specials(edges), 2 * nt // 3)):
        d_v = devmem.DeviceArray(np.full((vcap + 4, 8), GUARD, dtype=np.int32))
        d_t = devmem.DeviceArray(np.full((tcap + 4, 3), GUARD, dtype=np.int32))
        assert e.surface_mesh_device(c.origin, c.dims, d_v, vcap, d_t, tcap, counts) == (nv, nt)
        gv, gt = d_v.numpy(), d_t.numpy()
        rep.records(_records(gv[:vcap]), want_v[:vcap], allowed[:vcap], edges,
                    f"surface_mesh_device vertices (capacities {vcap} of {nv}, {tcap} of {nt})")
        rep.check(np.array_equal(gt[:tcap], want_t[:tcap]), f"surface_mesh_device triangles (capacity {tcap} of {nt})")
        rep.check(np.all(gv[vcap:] == GUARD) and np.all(gt[tcap:] == GUARD),
                  f"surface_mesh_device: nothing beyond capacities {vcap}, {tcap}")
        if vcap < nv:                                                                        # true indices are kept
            rep.check(gt[:tcap].max() >= vcap, f"surface_mesh_device: indices beyond the vertex capacity {vcap}")

    _same(before, _snapshot(e))                                                              # the map is only read
    assert not rep.failed, f"{name}: {rep.failed}"
