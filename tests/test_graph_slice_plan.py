"""nts_graph_plan_slices, the host planner of the sliced graph build (include/ntsynt_hip.h): contiguous bin ranges whose items fit
a byte budget, a bin that alone does not fit on its own."""
import ctypes

import numpy as np
import pytest

from ntsynt_amd import _lib

NTS_EINVAL = -22


def plan(hist, bytes_per_elem, budget):
    lib = _lib.load()
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    cuts = np.zeros(hist.size + 1, np.uint32)
    n = ctypes.c_uint32()
    rc = lib.nts_graph_plan_slices(hist.ctypes.data, hist.size, int(bytes_per_elem), int(budget), cuts.ctypes.data, ctypes.byref(n))
    return rc, cuts[:n.value + 1]


def check(hist, bpe, budget):
    rc, cuts = plan(hist, bpe, budget)
    assert rc == 0
    assert cuts[0] == 0 and cuts[-1] == len(hist)
    assert np.all(np.diff(cuts.astype(np.int64)) > 0)                  # increasing, every bin in exactly one slice
    for a, b in zip(cuts[:-1], cuts[1:]):
        items = int(np.sum(hist[a:b], dtype=np.uint64))
        # within budget, or a single bin that alone is over it
        assert items * bpe <= budget or (b - a == 1 and items * bpe > budget) or \
            (int(np.count_nonzero(hist[a:b])) == 1 and items * bpe > budget), (a, b, items)
    # greedy: no two neighbouring slices would fit as one
    for s in range(len(cuts) - 2):
        both = int(np.sum(hist[cuts[s]:cuts[s + 2]], dtype=np.uint64))
        assert both * bpe > budget
    return cuts


HISTS = {
    "uniform": np.full(65536, 40, np.uint64),
    "skewed": (np.random.default_rng(3).zipf(1.6, 65536) % 5000).astype(np.uint64),
    "hot_bin": np.concatenate([np.full(30000, 7, np.uint64), [3_000_000], np.full(35535, 7, np.uint64)]).astype(np.uint64),
    "sparse": np.where(np.arange(65536) % 97 == 0, 1000, 0).astype(np.uint64),
}


@pytest.mark.parametrize("name", sorted(HISTS))
@pytest.mark.parametrize("budget", [4096, 1 << 20, 50 << 20])
def test_cuts_cover_every_bin_and_slices_fit(name, budget):
    hist = HISTS[name]
    cuts = check(hist, 65, budget)
    if name == "uniform":
        per = budget // 65 // 40                                       # whole bins per slice
        assert len(cuts) - 1 == -(-65536 // max(per, 1))


def test_hot_bin_is_a_slice_of_its_own():
    hist = HISTS["hot_bin"]
    cuts = check(hist, 65, 1 << 20)
    assert 30000 in cuts.tolist() and 30001 in cuts.tolist()          # the bin over the budget stands alone
    s = cuts.tolist().index(30000)
    assert cuts[s + 1] == 30001


def test_budget_that_holds_everything_gives_one_slice():
    for hist in HISTS.values():
        total = int(np.sum(hist, dtype=np.uint64))
        rc, cuts = plan(hist, 65, total * 65)
        assert rc == 0 and cuts.tolist() == [0, hist.size]
        rc, cuts = plan(hist, 65, total * 65 + 12345)
        assert rc == 0 and cuts.tolist() == [0, hist.size]


def test_budget_zero_and_bad_arguments_are_rejected():
    """0 means "automatic" to nts_graph_budget; the build resolves it to bytes before it plans, so the planner refuses it"""
    hist = HISTS["uniform"]
    assert plan(hist, 65, 0)[0] == NTS_EINVAL
    assert plan(hist, 0, 1 << 20)[0] == NTS_EINVAL
    assert plan(np.zeros(0, np.uint64), 65, 1 << 20)[0] == NTS_EINVAL


def test_empty_histogram_is_one_slice():
    rc, cuts = plan(np.zeros(65536, np.uint64), 65, 1 << 20)
    assert rc == 0 and cuts.tolist() == [0, 65536]


def test_budget_setter_is_bound():
    lib = _lib.load()
    assert lib.nts_graph_budget(None, 1 << 30) == NTS_EINVAL        # (no context: refused, nothing touched)
    v = ctypes.c_uint32()
    assert lib.nts_graph_last_plan(None, ctypes.byref(v), None, None, None) == NTS_EINVAL
