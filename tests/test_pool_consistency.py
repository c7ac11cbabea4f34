"""parity.assert_pool_consistent on the CPU: it passes on real oracle maps of two pool sizes and fails, naming the rule,
on dumps doctored to break each rule once -- a pool index named twice, a free-list entry repeated, a block that is
neither free nor named, a block both free and named, and an active count that disagrees with the directory."""
import numpy as np
import pytest

from fuzz_cases import SMALL, passes
from parity import assert_pool_consistent
from ratsdf import synthetic

VS = 0.02


class Doctored:
    """the dumps of a real engine, changed by `edit(entries, blocks, num_free, heap)` before the check reads them"""

    def __init__(self, e, edit, active_delta=0):
        self.e, self.edit, self.active_delta = e, edit, active_delta
        self.block_bits = e.block_bits
        ei, bl = e.dump_directory()
        nf, heap = e.dump_heap()
        ei, bl, heap = ei.copy(), bl.copy(), heap.copy()
        self.dumps = edit(ei, bl, nf, heap)

    def dump_directory(self):
        return self.dumps[0], self.dumps[1]

    def dump_heap(self):
        return self.dumps[2], self.dumps[3]

    def num_active_blocks(self):
        return len(self.dumps[1]) + self.active_delta


@pytest.fixture(scope="module")
def grown(oracle_lib):
    """an oracle map with deletes behind it: freed blocks sit on the free list out of allocation order"""
    from ratsdf._abi import Engine
    e = Engine(oracle_lib, VS, 6 * VS)
    for f in synthetic.stream("room", 4, scale=0.25, noise=True, holes=True):
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], 4.0, f["intrinsics"], f["pose"])
    yield e
    e.close()


def test_real_maps_pass(grown, make_oracle):
    assert grown.totals()["deleted_blocks"] > 0 and len(grown.dump_directory()[1]) > 40
    assert_pool_consistent(grown)
    small = make_oracle(0.01, 0.06, **SMALL)  # 4096 pool blocks: the pool size comes from the engine
    for op, pos in passes(3, n_pass=30):
        (small.test_allocate if op == "alloc" else small.test_delete)(pos)
    assert 0 < small.num_active_blocks() < 4096 and small.dump_heap()[1].shape == (4096,)
    assert_pool_consistent(small)


def _named_twice(ei, bl, nf, heap):
    bl["idx"][5] = bl["idx"][2]  # entry 5's own block is now lost as well: the duplicate must be reported first
    return ei, bl, nf, heap


def _free_twice(ei, bl, nf, heap):
    heap[nf - 1] = heap[0]
    return ei, bl, nf, heap


def _lost(ei, bl, nf, heap):
    keep = np.ones(len(bl), dtype=bool)
    keep[3] = False  # an entry vanishes and its block goes nowhere
    return ei[keep], bl[keep], nf, heap


def _free_and_named(ei, bl, nf, heap):
    heap[0] = bl["idx"][7]
    return ei, bl, nf, heap


def _short_free_list(ei, bl, nf, heap):
    return ei, bl, nf - 1, heap  # the top of the free list is dropped


@pytest.mark.parametrize("edit,active_delta,message", [
    (_named_twice, 0, "named by two live entries"),
    (_free_twice, 0, "on the free list twice"),
    (_lost, 0, "neither free nor named"),
    (_short_free_list, 0, "neither free nor named"),
    (_free_and_named, 0, "both free and named"),
    (lambda *d: d, 1, "num_active_blocks"),
])
def test_each_rule_fails_on_a_doctored_dump(grown, edit, active_delta, message):
    assert_pool_consistent(Doctored(grown, lambda *d: d))  # the stub itself changes nothing
    with pytest.raises(AssertionError, match=message):
        assert_pool_consistent(Doctored(grown, edit, active_delta))


def test_a_larger_pool_than_configured_is_not_assumed(grown):
    """the same dumps checked as if the pool were twice as large leave half of it unaccounted for"""
    d = Doctored(grown, lambda *x: x)
    d.block_bits = grown.block_bits + 1
    with pytest.raises(AssertionError, match="neither free nor named"):
        assert_pool_consistent(d)
