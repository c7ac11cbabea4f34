"""The crafted surface cases (tests/surface_cases.py) without a GPU: each set holds the classes of records it was
written for, the float32 contract stays within a derived distance of the same formulas in float64 where every
intermediate is an ordinary number, the "is NaN" exemption of the comparison rule is capped at a count that follows
from the planted voxels, and single mistakes planted in the per-edge restatement change records of the set named for
them -- so a kernel that makes one of them fails tests/test_gpu_surface_cases.py."""
import numpy as np
import pytest

import surface_cases as sc
import surface_ref as sr
from surface_cases import F, TINY, UNIT, VS, Variant

FLOOR = 30          # records per class


def _sub(x):
    return (x != 0) & (np.abs(x) < TINY)


def _columns(e):
    return np.concatenate([e.t0[:, None], e.t1[:, None], e.den[:, None], e.f[:, None], e.u[:, None], e.d0, e.d1, e.p0,
                           e.p1, e.g, e.sq, e.len2[:, None], e.len[:, None], e.normal, e.pos], axis=1)


def classes(e):
    """name -> [n] bool over the records of `e`"""
    x = _columns(e)
    # a product that is 0 without a factor being 0 has underflowed
    under = ((e.p0 == 0) & (e.d0 != 0) & (e.u[:, None] != 0)) | ((e.p1 == 0) & (e.d1 != 0) & (e.f[:, None] != 0)) | \
            ((e.sq == 0) & (e.g != 0))
    finite_t = np.isfinite(e.t0) & np.isfinite(e.t1)
    return {
        "all_normal": np.isfinite(x).all(axis=1) & ~_sub(x).any(axis=1) & ~under.any(axis=1) & (e.len2 != 0),
        "len2_subnormal": _sub(e.len2),
        "flat_by_underflow": (e.len2 == 0) & (e.g != 0).any(axis=1),
        "tsdf_subnormal": _sub(e.t0) & _sub(e.t1) & _sub(e.den) & (_sub(e.d0) | _sub(e.d1)).any(axis=1),
        "flat_by_overflow": np.isinf(e.len2) & np.isfinite(e.g).all(axis=1),
        "difference_overflows": np.isinf(e.den) & finite_t,
        "normal_subnormal": _sub(e.normal).any(axis=1),        # g_b / len with a subnormal quotient
    }


# ---- the sets are what they say -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.CASES)
def test_the_per_edge_restatement_is_surface_ref(name):
    c = sc.case(name)
    assert len(c.blocks) <= 27 and max(c.dims) <= 26 and all(o % 8 for o in c.origin)
    assert len(np.unique(c.blocks.prob.view(np.uint32))) > 1000 or name == "probabilities"
    assert len(np.unique(np.ascontiguousarray(c.blocks.rgbw).view(np.uint32))) == c.blocks.rgbw.size
    for mp in c.min_probs:
        want, e = sc.expected_points(name, mp), sc.expected_edges(name, mp)
        bad = sc.differing(e.rec, want, sc.exempt(want, e))
        print(f"{name}, min_prob {mp!r}: {len(want)} records, {bad} differ between the two restatements")
        assert bad == 0 and len(want) >= 200
        assert np.bincount(e.axis, minlength=3).min() >= 20                      # crossings on all three axes
        assert ((e.owner[np.arange(len(e.axis)), e.axis] & 7) == 7).sum() >= 20  # ... across seams
    if c.mesh:                                                                   # and of the mesh's vertices
        v, tri = sc.expected_mesh(name)
        e = sc.expected_edges(name, over_mesh=True)
        assert sc.differing(e.rec, v, sc.exempt(v, e)) == 0 and len(tri) >= 300


def test_ladder_classes():
    small, large = (classes(sc.expected_edges(n)) for n in ("ladder_small", "ladder_large"))
    want = {"ladder_small": ("all_normal", "len2_subnormal", "flat_by_underflow", "tsdf_subnormal", "normal_subnormal"),
            "ladder_large": ("all_normal", "flat_by_overflow", "difference_overflows")}
    for name, cl in (("ladder_small", small), ("ladder_large", large)):
        counts = {k: int(v.sum()) for k, v in cl.items()}
        print(f"{name}: records per class {counts}")
        for k in want[name]:
            assert counts[k] >= FLOOR, (name, k)
    e = sc.expected_edges("ladder_small")
    m = small["len2_subnormal"]                   # the normal is legitimately not unit: sqrtf of a subnormal is coarse
    n2 = (e.rec["normal"][m].astype(np.float64) ** 2).sum(axis=1)
    print(f"ladder_small: |normal|^2 over the subnormal len^2 records spans {n2.min():.6f} .. {n2.max():.6f}")
    assert (np.abs(n2 - 1) > 1e-4).sum() >= FLOOR
    assert (e.rec["normal"][small["flat_by_underflow"]] == 0).all()
    # three distinct gradient components
    g = np.abs(e.g[small["all_normal"]])
    assert ((g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])).all()
    e = sc.expected_edges("ladder_large")
    assert (e.rec["normal"][large["flat_by_overflow"]] == 0).all()
    m = large["difference_overflows"]             # f is 0 (t0 and t0 - t1 share their sign: +0): pos is the owner's
    assert (e.f[m].view(np.uint32) == 0).all() and (e.t0[m] < 0).sum() >= FLOOR
    assert np.array_equal(e.rec["pos"][m], e.owner[m].astype(F) * F(VS)) and not e.up[m].any()
    assert np.array_equal(e.rec["rgbw"]["r"][m], (e.owner[m, 0] & 255).astype(np.uint8))


def _planted_map(name):
    return {p.voxel: p.word for p in sc.nonfinite_planted()} if name == "nonfinite" else {}


def _tsdf_at(c):
    """voxel -> tsdf, and "in the map" """
    b = sc.blocks_of(c)

    def at(v):
        key = tuple(int(x) >> 3 for x in v)
        if key not in b:
            return None
        return b[key][0][(int(v[0]) & 7) + 8 * (int(v[1]) & 7) + 64 * (int(v[2]) & 7)]
    return at


def nan_f_count(name):
    """how many records of the set have a NaN f, counted from the planted voxels alone: a planted voxel's edge to a
    neighbour of the other sign class has a NaN f when the voxel is the owner (inf / inf, or NaN in) and when it is a
    NaN upper endpoint; an infinite upper endpoint gives x / inf = 0.  (NaN is not negative.)"""
    c, at, n = sc.case(name), _tsdf_at(sc.case(name)), 0
    o, d = np.array(c.origin), np.array(c.dims)
    for v, word in _planted_map(name).items():
        t = sc.bits(word)
        for a in range(3):
            up, dn = at(np.add(v, UNIT[a])), at(np.subtract(v, UNIT[a]))
            if up is not None and bool(t < 0) != bool(up < 0) and np.all((np.array(v) >= o) & (np.array(v) < o + d)):
                n += 1                                                   # the planted voxel owns the edge
            if dn is not None and np.isnan(t) and bool(dn < 0) and np.all((np.subtract(v, UNIT[a]) >= o)):
                n += 1                                                   # a NaN upper endpoint below a negative owner
    return n


# the records whose pos[a] is compared as "is NaN" only, per set: exact, not "at most"
NAN_EXEMPT = {"ladder_small": 0, "ladder_large": 0, "nonfinite": 269, "quotients": 0, "probabilities": 0}


@pytest.mark.parametrize("name", sc.CASES)
def test_the_nan_exemption_is_capped(name):
    c = sc.case(name)
    for mp in c.min_probs:
        want, e = sc.expected_points(name, mp), sc.expected_edges(name, mp)
        allowed = sc.exempt(want, e)              # asserts: only pos[a] where f is NaN, never a normal
        assert allowed.sum(axis=1).max(initial=0) <= 1
        print(f"{name}, min_prob {mp!r}: {int(allowed.sum())} records are compared as 'is NaN' in pos[a]")
        assert int(allowed.sum()) == NAN_EXEMPT[name] == nan_f_count(name)
    if c.mesh:
        v, _ = sc.expected_mesh(name)
        allowed = sc.exempt(v, sc.expected_edges(name, over_mesh=True))
        print(f"{name}, mesh: {int(allowed.sum())} vertices are compared as 'is NaN' in pos[a]")
        assert int(allowed.sum()) == NAN_EXEMPT[name]                   # every voxel observed: every crossing a vertex


def test_nonfinite_roles_and_what_the_contract_gives():
    c, e = sc.case("nonfinite"), sc.expected_edges("nonfinite")
    planted = _planted_map("nonfinite")
    vox = np.array(list(planted))
    assert all(np.abs(vox - p).max(axis=1)[np.any(vox != p, axis=1)].min() >= 4 for p in vox)
    roles = {}                                    # (word, role) -> the local indices the planted voxel has
    seen_flat_nan, seen_flat_inf = 0, 0
    for i in range(len(e.rec)):
        v, a = e.owner[i], int(e.axis[i])
        w = v + UNIT[a]
        stencil = [tuple(x + s * UNIT[b]) for x in (v, w) for b in range(3) for s in (-1, 1)]
        if tuple(v) in planted:
            role, p = "owner", tuple(v)
        elif tuple(w) in planted:
            role, p = "upper", tuple(w)
        else:
            hit = [s for s in stencil if s in planted]
            if not hit:
                continue
            assert len(hit) == 1                  # no record's stencil holds two of them
            role, p = "gradient", hit[0]
            assert np.isfinite(e.rec["pos"][i]).all() and (e.rec["normal"][i] == 0).all()
            assert not np.isfinite(e.len[i])
            seen_flat_nan += int(np.isnan(e.len[i]))
            seen_flat_inf += int(np.isinf(e.len[i]))
        roles.setdefault((planted[p], role), set()).update(int(x) & 7 for x in p)
    for word in sc.NONFINITE_WORDS:
        for role in ("owner", "upper", "gradient"):
            assert (word, role) in roles, (hex(word), role)
    for role in ("owner", "upper", "gradient"):
        local = set().union(*(roles[(w, role)] for w in sc.NONFINITE_WORDS))
        assert {0, 7} <= local and local - {0, 7}, role
    print(f"nonfinite: {seen_flat_nan} records flat through a NaN len and {seen_flat_inf} through an infinite one, "
          f"from a gradient neighbour alone")
    assert seen_flat_nan >= FLOOR
    # by construction: NaN is not negative; inf / inf is a NaN f, the lower endpoint and a NaN pos[a]; x / inf is 0
    at = _tsdf_at(c)
    edges = {(tuple(v), int(a)): i for i, (v, a) in enumerate(zip(e.owner, e.axis))}
    n_nan = n_inf_owner = n_inf_upper = 0
    for p, word in planted.items():
        t = sc.bits(word)
        for a in range(3):
            up, dn = at(np.add(p, UNIT[a])), at(np.subtract(p, UNIT[a]))
            i = edges.get((p, a))
            if up is not None and np.isnan(t):
                assert (i is not None) == bool(up < 0)
                n_nan += 1
            if up is not None and np.isinf(t) and i is not None:
                assert np.isnan(e.f[i]) and np.isnan(e.rec["pos"][i, a]) and not e.up[i]
                assert e.rec["rgbw"]["r"][i] == p[0] & 255 and e.rec["rgbw"]["g"][i] == p[1] & 255
                n_inf_owner += 1
            j = edges.get((tuple(np.subtract(p, UNIT[a])), a))
            if dn is not None and np.isinf(t) and j is not None:
                assert e.f[j] == 0 and not e.up[j] and e.rec["pos"][j, a] == F(p[a] - 1) * F(VS)
                n_inf_upper += 1
    print(f"nonfinite: {n_nan} upward edges of NaN voxels, {n_inf_owner} crossings owned by an infinity, "
          f"{n_inf_upper} with an infinite upper endpoint")
    assert min(n_nan, n_inf_owner, n_inf_upper) >= FLOOR


def test_quotients_are_what_they_are_named():
    e = sc.expected_edges("quotients")
    edges = {(tuple(v), int(a)): i for i, (v, a) in enumerate(zip(e.owner, e.axis))}
    seen = set()
    for p in sc.quotient_pairs():
        i = edges[(p.owner, p.axis)]
        assert e.f[i].view(np.uint32) == p.f_bits, p
        assert ((p.owner[p.axis] & 7) == 7) == p.seam
        up = p.kind in ("half", "half_above", "one")
        assert bool(e.up[i]) == up, p
        chosen = np.add(p.owner, UNIT[p.axis]) if up else np.array(p.owner)
        assert [int(e.rec["rgbw"][k][i]) for k in "rgb"] == [int(x) & 255 for x in chosen], p
        if p.kind == "one":                       # pos[a] is the next voxel's
            assert e.rec["pos"][i, p.axis] == F(p.owner[p.axis] + 1) * F(VS)
        seen.add((p.kind, p.axis, p.seam))
    assert len(seen) == len(sc.QUOTIENT_KINDS) * 3 * 2
    sub = e.f[(e.f != 0) & (np.abs(e.f) < TINY)]
    assert len(sub) == 6


def test_probabilities_hold_the_awkward_words():
    c = sc.case("probabilities")
    full = sc.expected_edges("probabilities", 0.0)
    word = full.rec["prob"].view(np.uint32)
    for w in sc.PROB_WORDS:
        if w is not None and w != 0x80000002:     # (a negative subnormal is below every min_prob here)
            assert (word == w).sum() >= 10, hex(w)
    nan = np.isnan(full.rec["prob"]).sum()
    for mp in c.min_probs:
        e = sc.expected_edges("probabilities", mp)
        kept = e.rec["prob"]
        print(f"probabilities, min_prob {mp!r}: {len(kept)} of {len(full.rec)} records kept, "
              f"{int(np.isnan(kept).sum())} with a NaN probability")
        assert np.isnan(kept).sum() == nan >= 2 * FLOOR                  # a NaN probability is never dropped
        assert not (kept[~np.isnan(kept)] < F(mp)).any()
    zero, minus_zero = (sc.expected_points("probabilities", mp) for mp in (0.0, -0.0))
    assert sr.same_bytes(zero, minus_zero)
    assert (zero["prob"].view(np.uint32) == 0x80000000).sum() >= 10                # -0.0 < 0.0 is false: kept
    between = sc.expected_edges("probabilities", sc.MIN_PROB_BETWEEN).rec["prob"].view(np.uint32)
    assert (between == 5).sum() >= 10 and (between == 3).sum() == 0 and (between == 0).sum() == 0
    top = sc.expected_edges("probabilities", float("inf")).rec["prob"]
    assert (np.isnan(top) | (top == np.inf)).all() and (top == np.inf).sum() >= 10


def test_the_mesh_has_no_min_prob():
    """a vertex of negative probability stays, where surface points at min_prob 0.0 drop it: every crossing of the
    all-observed map is a vertex"""
    v, tri = sc.expected_mesh("probabilities")
    e = sc.expected_edges("probabilities", over_mesh=True)
    negative = int((v["prob"].view(np.uint32) == 0x80000002).sum())
    print(f"probabilities, mesh: {len(v)} vertices, {negative} of them with a negative subnormal probability")
    assert sc.differing(e.rec, v, sc.exempt(v, e)) == 0 and negative >= 10
    assert len(v) == len(sc.expected_edges("probabilities", 0.0).rec) + negative
    assert np.isnan(v["prob"]).sum() >= FLOOR and len(np.unique(tri)) == len(v)


@pytest.mark.parametrize("name", sc.MESH_CASES)
def test_mesh_topology_follows_from_the_signs_alone(name):
    """NaN, +-0 and infinite corners: the same triangles as the map with every word replaced by +-1 of equal
    "negative" bit; only the vertex records differ"""
    v, tri = sc.expected_mesh(name)
    sv, stri = sc.expected_mesh(name, signs_only=True)
    print(f"mesh_values, {name}: {len(v)} vertices, {len(tri)} triangles; {sc.changed(v, sv)} vertex records differ "
          f"from the +-1 map's")
    assert np.array_equal(tri, stri) and len(v) == len(sv) and len(tri) >= 300
    assert np.array_equal(v["rgbw"]["weight"], sv["rgbw"]["weight"]) and sc.changed(v, sv) > 0
    assert tri.min() == 0 and tri.max() == len(v) - 1 and len(np.unique(tri)) == len(v)


# ---- the distance of the float32 contract from the same formulas in float64 ----------------------------------------
def test_distance_from_float64():
    """On the records whose intermediates are all ordinary numbers.  u = 2^-24, first order, every operation of the
    contract correctly rounded (relative error at most u each):
      pos[a] = ((float)v + f) * vs with f = t0 / (t0 - t1): four rounded operations, none of which lets an earlier error
        grow (0 <= f <= 1, v is an integer, |v + f| <= |v| + 1), so |pos[a] - pos64[a]| <= 4 u (|v[a]| + 1) vs.
      normal: f carries 2 u (subtraction, division), 1 - f then 3 u absolute (2 u of f and its own rounding);
        d_b carries u; d0 (1 - f) is off by at most |d0| (3 u + 2 u), d1 f by |d1| (u + 2 u + u), their sum by
        u |g_b| <= 2 u D_b more, D_b = max(|d0_b|, |d1_b|): |g_b - g_b64| <= 11 u D_b.  Where the two terms cancel
        that is large against g_b itself: the bound is in D, not in g.  len^2 adds three roundings to the squares and
        sqrtf halves them and adds one: |len - len64| <= 11 u |D| + 2.5 u len.  The quotient adds one more:
        |normal_b - normal_b64| <= u (11 D_b / len + 11 |D| / len + 3.5), using |normal_b| <= 1.
    Second-order terms are covered by a factor of 1.01 (|D| / len stays below 2^10 on these records, asserted)."""
    u = 2.0 ** -24
    worst = {"pos": 0.0, "normal": 0.0}
    total = 0
    for name in ("ladder_small", "ladder_large", "nonfinite", "quotients"):
        e, e64 = sc.expected_edges(name), sc.expected_edges(name, 0.0, Variant(f64=True))
        assert np.array_equal(e.owner, e64.owner) and np.array_equal(e.axis, e64.axis)
        m = classes(e)["all_normal"] & np.isfinite(_columns(e64)).all(axis=1)
        total += int(m.sum())
        va = np.abs(e.owner[m]).astype(np.float64)                     # (per component; the two other axes have
        err = np.abs(e.pos[m].astype(np.float64) - e64.pos[m])         # one rounding each and take the same bound)
        bound = 1.01 * 4 * u * (va + 1) * float(F(VS))
        assert (err <= bound).all(), name
        worst["pos"] = max(worst["pos"], float((err / bound).max()))
        D = np.maximum(np.abs(e64.d0[m]), np.abs(e64.d1[m]))
        ratio = np.sqrt((D * D).sum(axis=1)) / e64.len[m]
        assert ratio.max() < 2 ** 10
        err = np.abs(e.normal[m].astype(np.float64) - e64.normal[m])
        bound = 1.01 * u * (11 * D / e64.len[m][:, None] + 11 * ratio[:, None] + 3.5)
        assert (err <= bound).all(), name
        worst["normal"] = max(worst["normal"], float((err / bound).max()))
        print(f"{name}: {int(m.sum())} all-normal records, worst normal error {err.max() / u:.2f} u, "
              f"worst |D| / len {ratio.max():.1f}")
    print(f"float64 distance over {total} records: worst error / bound {worst['pos']:.3f} for pos, "
          f"{worst['normal']:.3f} for the normal")
    assert total >= 400 and 0 < worst["pos"] <= 1 and 0 < worst["normal"] <= 1


# ---- wrong variants -------------------------------------------------------------------------------------------------
WRONG = [
    ("subnormal inputs flushed to zero", Variant(flush_in=True), "ladder_small", 0.0),
    ("subnormal results flushed", Variant(flush_out=True), "ladder_small", 0.0),
    ("fused multiply-add in g_b and len^2", Variant(fma=True), "ladder_small", 0.0),
    ("fused multiply-add in g_b and len^2", Variant(fma=True), "ladder_large", 0.0),
    ("tie as f > 0.5f", Variant(tie_gt=True), "quotients", 0.0),
    ("negative as signbit", Variant(negative="signbit"), "quotients", 0.0),
    ("negative as signbit", Variant(negative="signbit"), "nonfinite", 0.0),
    ("negative as !(t >= 0)", Variant(negative="not_ge"), "nonfinite", 0.0),
    ("flat rule as len == 0 only", Variant(flat="zero_only"), "ladder_large", 0.0),
    ("flat rule as len == 0 only", Variant(flat="zero_only"), "nonfinite", 0.0),
    ("flat rule missing", Variant(flat="none"), "ladder_small", 0.0),
    ("flat rule missing", Variant(flat="none"), "nonfinite", 0.0),
    ("central difference as tu * 0.5f - td * 0.5f", Variant(split_half=True), "ladder_small", 0.0),
    ("prob < min_prob on flushed operands", Variant(prob_flushed=True), "probabilities", sc.MIN_PROB_BETWEEN),
    ("prob < min_prob on flushed operands", Variant(prob_flushed=True), "probabilities", 0.0),
    ("upper endpoint from the owner's block at a seam", Variant(seam_own_block=True), "quotients", 0.0),
    ("upper endpoint from the owner's block at a seam", Variant(seam_own_block=True), "probabilities", float("inf")),
]


@pytest.mark.parametrize("what,variant,name,min_prob", WRONG, ids=[f"{w[0]} on {w[2]}" for w in WRONG])
def test_wrong_variant_changes_records_of_its_set(what, variant, name, min_prob):
    want = sc.expected_edges(name, min_prob).rec         # (asserted above to be surface_ref's records)
    wrong = sc.expected_edges(name, min_prob, variant).rec
    n = sc.changed(want, wrong)
    print(f"{what}: changes {n} records of {name} ({len(want)} by the contract, {len(wrong)} by the variant)"
          + (f" at min_prob {min_prob!r}" if min_prob else ""))
    assert n > 0
    if name in sc.MESH_CASES and variant.negative == "lt":     # the mesh's vertices are the same crossings
        v, _ = sc.expected_mesh(name)
        assert sc.changed(v, sc.expected_edges(name, 0.0, variant, True).rec) > 0
