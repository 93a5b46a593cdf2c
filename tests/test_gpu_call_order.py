"""Every device call gives its result after any other (docs/design/04_24_call_order.md).  The entries of tests/call_order_cases.py --
every entry point that takes named scratch buffers from the context (ws_get) or goes through its pinned staging area -- run in orders
the other GPU tests never take.  In a context of the test's own (`fresh`: but for what a sliced graph build drops, a context's scratch
only grows, so only a new one regrows):
small, large, small (every buffer regrows, is freed into the allocation cache and is met again); around a neighbour that requests the
same scratch names (the neighbour's large call is the regrowth); and small, large, small with the allocation cache emptied, or a freed
block taken and overwritten by somebody else, between the calls.  In ONE context that every earlier test has grown (`ctx`): a refused
call between good ones, and one long shuffled chain -- what a call inherits in buffers that stay.  Every result is compared byte for
byte with the brute force or the oracle (integer kernels: no tolerance).  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests import call_order_cases as C

pytestmark = pytest.mark.gpu
STEP_SECONDS = 120
NAMES = [e.name for e in C.ENTRIES]
FILLER_BYTES, FILLER_BYTE = 64 << 20, 0xA5


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ctx():
    from ntsynt_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture
def fresh():
    "a context nothing has run in: every scratch buffer and the staging area are still to be allocated"
    from ntsynt_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def call(ctx, name, size, before=()):
    "one entry at one size against its expectation; `before`: the calls that ran ahead of it, for the message.  Returns the bytes"
    want = C.expected_of(name, size)
    got = C.BY_NAME[name].run(ctx, C.case_of(name, size))
    assert isinstance(got, bytes)
    if got != want:
        n = min(len(got), len(want))
        at = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError(f"{name} at {size} differs from its expectation at byte {at} of {len(got)} / {len(want)}; before it ran {list(before)[-2:]}")
    return got


def play(ctx, steps, between=None):
    out = []
    for i, (name, size) in enumerate(steps):
        out.append(call(ctx, name, size, steps[:i]))
        if between is not None:
            between()
    return out


# ---- growth and return ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_small_large_small(fresh, name):
    first, _, third = play(fresh, [(name, "S"), (name, "L"), (name, "S")])
    assert first == third


@pytest.mark.parametrize("way", sorted(C.SKETCH_WAYS))
@pytest.mark.parametrize("size", C.SIZES)
def test_the_sketch_goes_the_way_its_entry_is_named_for(ctx, way, size):
    call(ctx, "sketch_" + way, size)
    went = C.SKETCH_WENT[(way, C.case_of("sketch_" + way, size)["og"].total_bp)]
    print(f"sketch {way} at {size}: {went}")
    assert C.SKETCH_CHECK[way](went), (way, size, went)


class Recording:
    "a context's library with the names of the functions taken from it written down"

    def __init__(self, lib):
        self._lib, self.seen = lib, set()

    def __getattr__(self, name):
        self.seen.add(name)
        return getattr(self._lib, name)


@pytest.mark.parametrize("name", sorted(C.CALLS))
def test_an_entry_calls_the_exported_functions_its_table_names(fresh, name):
    "C.CALLS is written by hand; that an entry's run() reaches the functions it names is read off the context's library here"
    lib = fresh.lib
    fresh.lib = Recording(lib)
    try:
        call(fresh, name, "S")
        seen = fresh.lib.seen
    finally:
        fresh.lib = lib
    assert set(C.CALLS[name]) <= seen, (name, sorted(set(C.CALLS[name]) - seen))


# ---- neighbours -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x,y", C.neighbours())
def test_around_a_neighbour(fresh, x, y):
    play(fresh, [(x, "S"), (y, "L"), (x, "S"), (y, "S"), (x, "L")])


@pytest.mark.parametrize("first,second", [("graph_build", "graph_build"), ("graph_build", "graph_build_sliced"), ("graph_build_sliced", "graph_build"),
                                          ("graph_build_sliced", "graph_build_sliced")])
def test_two_graph_builds_back_to_back(fresh, first, second):
    """the graph a build returns lives in the context's scratch until the next build: it is read back in full (inside nts_graph_build,
    which synchronises behind its copies) before the second build reuses, regrows or drops that scratch, and a second build of the same
    case behind it gives the bytes the first gave"""
    before = call(fresh, first, "S")
    call(fresh, second, "L", [(first, "S")])
    assert call(fresh, first, "S", [(first, "S"), (second, "L")]) == before
    assert call(fresh, second, "S", [(second, "L"), (first, "S")]) == before      # (one case, one graph, whatever the slices)


@pytest.mark.parametrize("size", C.SIZES)
def test_the_sliced_build_has_the_slices_its_entry_is_named_for(ctx, size):
    call(ctx, "graph_build_sliced", size)
    plan = C.case_of("graph_build_sliced", size)["sliced_plan"]
    print(f"graph_build_sliced at {size}: {plan}")
    assert plan["v_slices"] >= C.GRAPH_SLICES, (size, plan)
    assert fresh_budget_is_automatic(ctx)


def fresh_budget_is_automatic(ctx):
    "the budget a sliced entry set is gone: a one-pass build behind it plans one range per pass"
    call(ctx, "graph_build", "S")
    plan = ctx.graph_last_plan()
    return plan["v_slices"] == 1 and plan["e_slices"] == 1


# ---- the cache in between -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_cache_emptied_after_every_call(fresh, name):
    "what the large call's regrowth freed goes back to the driver before the next call: a pointer kept into it is no longer mapped memory of ours"
    first, _, third = play(fresh, [(name, "S"), (name, "L"), (name, "S")], between=fresh.mem_trim)
    assert first == third


@pytest.mark.parametrize("name", NAMES)
def test_a_filter_takes_the_freed_blocks_between_the_calls(fresh, name):
    """64 MiB of 0xA5 created before the first call and freed and created again after every call: what it gives back is what the next
    call's regrown scratch of 64 KiB and more is cut from, and a write through a pointer into such a block after the block went back
    lands in the next filter: its bytes are read back before it goes"""
    from ntsynt_amd.device import BloomFilter
    fill = np.full(FILLER_BYTES, FILLER_BYTE, dtype=np.uint8)
    held = []

    def swap():
        for bf in held:
            got = bf.to_numpy()
            try:
                assert got.size == FILLER_BYTES and (got == FILLER_BYTE).all(), (name, "the filler filter was written to", int((got != FILLER_BYTE).sum()))
            finally:
                bf.free()
        held.clear()
        bf = BloomFilter(fresh, FILLER_BYTES, 24)
        bf.from_numpy(fill)
        held.append(bf)
    try:
        swap()
        first, _, third = play(fresh, [(name, "S"), (name, "L"), (name, "S")], between=swap)
        assert first == third
    finally:
        for bf in held:
            bf.free()


# ---- a refused call in the middle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [e.name for e in C.ENTRIES if e.refuse])
def test_a_refused_call_in_the_middle(ctx, name):
    from ntsynt_amd.device import NtsError
    e = C.BY_NAME[name]
    first = call(ctx, name, "S")
    with pytest.raises(NtsError):
        e.refuse(ctx, C.case_of(name, "S"))
    call(ctx, name, "L", [(name, "S"), (name, "refused")])
    assert call(ctx, name, "S", [(name, "refused"), (name, "L")]) == first


# ---- one long chain, and a fresh context --------------------------------------------------------------------------------------------
_chain = {}


def run_chain(ctx):
    "the chain's results per (entry, size), once; every expectation is computed before its first GPU call"
    if not _chain:
        order = C.chain_order()
        for name, size in order:
            C.expected_of(name, size)
        ran = {}
        for i, (name, size) in enumerate(order):
            got = call(ctx, name, size, order[:i])
            assert ran.setdefault((name, size), got) == got, (name, size, "two results in one chain", order[max(i - 2, 0):i])
        _chain.update(order=order, ran=ran)
    return _chain["order"], _chain["ran"]


def test_one_long_chain(ctx):
    order, ran = run_chain(ctx)
    assert set(ran) == {(n, s) for n in NAMES for s in C.SIZES}, "an entry or a size was left out"
    assert len(order) == C.CHAIN_PASSES * len(NAMES)


def test_a_fresh_context_agrees_with_the_chain(ctx):
    from ntsynt_amd.device import Context
    _, ran = run_chain(ctx)
    for name in NAMES:
        other = Context(0)
        try:
            assert C.BY_NAME[name].run(other, C.case_of(name, "S")) == ran[(name, "S")], name
        finally:
            other.close()
