"""The directory rule of map files (include/ratsdf_map.h: D1 walks end, D2 a block is where lookups find it, D3 no
block behind a dead node, H the header names a configuration an engine can have) without a GPU.  The load kernels
check nothing on the device, so ratsdf_map_file_info -- the host validation ratsdf_load_map shares -- must refuse
every file whose directory is no hash table, however right its sizes, indices and checksum are.  Good files come from
the CPU oracle through mapfile_ref.from_dumps, in directories small enough to chain; the defects are
tests/mapfile_cases.py; the rule is restated in mapfile_ref.check_directory, and the two must agree on every file
written here."""
import numpy as np
import pytest

import mapfile_cases as mc
import mapfile_ref as ref
from kat_cases import chain_positions, ref_hash
from ratsdf import synthetic

BUCKET_BITS = 9   # the smallest directory the engine accepts: 512 buckets, 1024 entries
BLOCK_BITS = 8
LAST = (1 << BUCKET_BITS) - 1
# bucket -> blocks in it.  "wrap": the last bucket's chain continues at the table's start, as kat_cases.case_collision
# shows for the default table; "long": a chain of 7 nodes, its neighbour bucket's blocks among them, and bucket 0
LAYOUT = {"wrap": {LAST: 8, 5: 5, 300: 1}, "long": {100: 9, 101: 4, 0: 3, 301: 2}}
WRITTEN = {}  # name -> bytes of every file this module handed to map_file_info or check_directory


def _positions(layout):
    return [p for bucket, count in layout.items() for p in chain_positions(bucket, count, bucket_bits=BUCKET_BITS)]


def _allocated(oracle_lib, layout):
    from ratsdf._abi import Engine
    e = Engine(oracle_lib, 0.02, 0.12, block_bits=BLOCK_BITS, bucket_bits=BUCKET_BITS)
    pos = _positions(layout)
    for _ in range(max(layout.values())):  # one insertion per bucket per pass (voxel_hash.cu:67-104)
        e.test_allocate(pos)
    assert e.num_active_blocks() == len(pos)
    return e


@pytest.fixture(scope="module")
def good(oracle_lib):
    """name -> bytes: the two crafted directories, and a sphere scan in a directory of 1024 buckets"""
    from ratsdf._abi import Engine
    out = {}
    for name, layout in LAYOUT.items():
        e = _allocated(oracle_lib, layout)
        out[name] = ref.from_dumps(e)
        e.close()
    e = Engine(oracle_lib, 0.02, 0.12, block_bits=14, bucket_bits=10, threads=8)
    for f in synthetic.stream("sphere", 3, scale=0.25):
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
    out["sphere"] = ref.from_dumps(e)
    e.close()
    return out


@pytest.fixture(scope="module")
def bad(good):
    """(good file, defect) -> (bytes, violation) for the two crafted directories"""
    return {(g, name): case for g in LAYOUT for name, case in mc.defects(good[g]).items()}


def _status(tmp_path, name, data):
    """map_file_info's status for the file (0: accepted)"""
    import ratsdf
    WRITTEN[name] = data
    p = tmp_path / "m.map"
    p.write_bytes(data)
    try:
        ratsdf.map_file_info(p)
    except ratsdf.RatsdfError as err:
        return err.status
    return 0


def test_the_good_files_chain_wrap_and_pass_the_rule(good):
    for name in LAYOUT:
        m = ref.parse(good[name])
        assert len(mc.chained(m)) >= 8, name
        assert ref.check_directory(m) is None, name
    m = ref.parse(good["wrap"])
    n = mc.n_entry(m)
    assert mc.wrap_links(m) == [n - 1], "the last bucket's list head leads across the table's end"
    chain = mc.chains(m)[0]
    assert chain[0] == n - 1 and chain[1] < chain[0] and len(chain) == 7  # head + 6 nodes, at the table's start
    assert all(ref_hash(mc.position(m, e), BUCKET_BITS) == LAST for e in chain)
    assert len(mc.chains(ref.parse(good["long"]))[0]) >= 1 + 3
    m = ref.parse(good["sphere"])
    assert len(m["entry_index"]) > 100 and mc.chained(m) and ref.check_directory(m) is None


@pytest.mark.parametrize("which", list(LAYOUT))
@pytest.mark.parametrize("defect", [f.__name__ for f in mc.D2_DEFECTS + mc.D1_DEFECTS + mc.D3_DEFECTS]
                         + mc.HEADER_DEFECTS)
def test_defective_file_is_refused(tmp_path, bad, which, defect):
    assert mc.self_cycle_exists({"bucket_bits": BUCKET_BITS}), "1024 entries: an offset of 1024 is an int16"
    data, violation = bad[which, defect]
    assert ref.check_directory(ref.parse(data)) == violation
    assert _status(tmp_path, f"{which}: {defect}", data) == 1


def test_every_defect_is_a_case(bad):
    names = {name for _, name in bad}
    assert names == {f.__name__ for f in mc.D2_DEFECTS + mc.D1_DEFECTS + mc.D3_DEFECTS} | set(mc.HEADER_DEFECTS)
    assert len(set(data for data, _ in bad.values())) == len(bad)  # no two cases are the same file


def test_the_defects_are_what_they_say(good):
    """the cases' own construction, checked on the parsed files: which entries moved, which ring the offsets form"""
    g = ref.parse(good["wrap"])
    n = mc.n_entry(g)

    def ring(m, start):
        seen, e = [], start
        while e not in seen:
            seen.append(e)
            e = (e + int(m["blocks"]["offset"][mc.record(m, e)])) & (n - 1)
        return seen[seen.index(e):]

    chain = mc.chains(g)[0]
    for f, length in ((mc.two_entry_cycle, 2), (mc.self_cycle, 1), (mc.long_cycle, len(chain) - 1),
                      (mc.cycle_through_the_end, len(chain))):
        m = ref.parse(mc.rewrite(good["wrap"], f))
        r = ring(m, chain[-1])
        assert len(r) == length, f.__name__
        if f is mc.cycle_through_the_end:
            assert n - 1 in r and min(r) < 16  # both sides of the table's end
    m = ref.parse(mc.rewrite(good["wrap"], mc.dead_cycle))
    extra = np.setdiff1d(m["entry_index"], g["entry_index"])
    assert len(extra) == 2 and all(not mc.live(m, int(e)) for e in extra) and len(ring(m, int(extra[0]))) == 2
    # a moved entry keeps its place and no longer hashes there; a duplicate names a position twice
    for f in (mc.moved_home_entry, mc.moved_chain_node):
        m = ref.parse(mc.rewrite(good["wrap"], f))
        changed = [int(e) for e, a, b in zip(g["entry_index"], g["blocks"], m["blocks"]) if a != b]
        assert len(changed) == 1 and np.array_equal(m["entry_index"], g["entry_index"])
        assert (changed[0] in mc.chained(g)) == (f is mc.moved_chain_node)
    for f in (mc.duplicate_in_home_entries, mc.duplicate_in_chain):
        m = ref.parse(mc.rewrite(good["wrap"], f))
        pos = [mc.position(m, int(e)) for e in m["entry_index"]]
        assert len(set(pos)) == len(pos) - 1
    m = ref.parse(mc.rewrite(good["wrap"], mc.cut_link))
    assert len(mc.chains(m)[0]) == len(chain) - 1 and mc.live(m, chain[-1])


def test_good_files_are_accepted(tmp_path, good):
    for name, data in good.items():
        assert ref.check_directory(ref.parse(data)) is None, name
        assert _status(tmp_path, f"{name}: good", data) == 0, name
        orphan = mc.with_orphan_dead_node(data)
        m = ref.parse(orphan)
        assert np.count_nonzero((m["blocks"]["idx"] == -1) & (m["blocks"]["offset"] != 0)) == 1
        assert ref.check_directory(m) is None, name
        assert _status(tmp_path, f"{name}: orphan dead node", orphan) == 0, name


@pytest.mark.parametrize("which", list(LAYOUT))
def test_files_after_deletions_are_accepted(tmp_path, oracle_lib, good, which):
    """the oracle's Delete unlinks a node (voxel_hash.cu:135-187): after the tail, a middle node and the list head of
    the longest chain have gone, the rest of the chain is still found"""
    g = ref.parse(good[which])
    chain = mc.chains(g)[0]
    e = _allocated(oracle_lib, LAYOUT[which])
    left = len(g["entry_index"])
    for what, entry in (("tail", chain[-1]), ("middle", chain[len(chain) // 2]), ("head", chain[0])):
        e.test_delete([mc.position(g, entry)])
        left -= 1
        assert e.num_active_blocks() == left
        data = ref.from_dumps(e)
        m = ref.parse(data)
        assert len(mc.chained(m)) >= len(chain) - 4  # the chain is shorter, not gone
        assert ref.check_directory(m) is None, what
        assert _status(tmp_path, f"{which}: {what} deleted", data) == 0, what
    e.close()


def test_create_refuses_what_a_file_may_not_hold(make_oracle):
    """rule H is the range of ratsdf_create_ex: an engine cannot save a header that a load would refuse"""
    import ratsdf
    for kw in (dict(voxel_size=float("inf")), dict(truncation=float("inf")), dict(voxel_size=float("nan")),
               dict(shard_slab_bits=ref.MAX_SHARD_SLAB_BITS + 1), dict(shard_rank=3, shard_count=3)):
        with pytest.raises(ratsdf.RatsdfError) as ei:
            make_oracle(**{"voxel_size": 0.02, "truncation": 0.12, **kw})
        assert ei.value.status == 1, kw
    make_oracle(0.02, 0.12, shard_slab_bits=ref.MAX_SHARD_SLAB_BITS, shard_rank=2, shard_count=3)


@pytest.mark.parametrize("which", list(LAYOUT))
def test_randomly_changed_directories(tmp_path, good, which):
    """one to three entries get another offset (small, back to an entry of the file, the table's size) or another
    entry's position: the engine's check, organised per bucket, and the rule's plain lookups give the same answer"""
    rng = np.random.default_rng(2024)
    g = ref.parse(good[which])
    n, table = len(g["entry_index"]), mc.n_entry(g)
    verdicts = []
    for k in range(120):
        def change(m):
            for _ in range(int(rng.integers(1, 4))):
                e = int(m["entry_index"][rng.integers(n)])
                kind = int(rng.integers(4))
                if kind == 0:
                    mc.set_offset(m, e, int(rng.integers(-6, 7)))
                elif kind == 1:
                    mc.set_offset(m, e, int(rng.choice([0, table, -table])))
                elif kind == 2:
                    to = int(m["entry_index"][rng.integers(n)])
                    if to != e:
                        mc.link(m, e, to)
                else:
                    mc.set_position(m, e, mc.position(m, int(m["entry_index"][rng.integers(n)])))
        data = mc.rewrite(good[which], change)
        verdict = ref.check_directory(ref.parse(data))
        assert (_status(tmp_path, f"{which}: random {k}", data) == 0) == (verdict is None), (k, verdict)
        verdicts.append(verdict)
    assert {None, "D1", "D2"} <= set(verdicts), "the changes reach every outcome"


def test_zz_the_rule_and_the_engine_agree_on_every_file(tmp_path, good, bad):
    """over everything this module wrote (run alone: over the cases, written here)"""
    for (which, name), (data, _) in bad.items():
        WRITTEN.setdefault(f"{which}: {name}", data)
    for name, data in good.items():
        WRITTEN.setdefault(f"{name}: good", data)
    assert len(WRITTEN) >= len(bad) + len(good)
    for name, data in sorted(WRITTEN.items()):
        ok = ref.check_directory(ref.parse(data)) is None
        assert (_status(tmp_path, name, data) == 0) == ok, name
