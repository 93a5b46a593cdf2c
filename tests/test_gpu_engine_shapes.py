"""The device graph engine (nts_engine_*, csrc/nts_dgraph.inc) on hand-made graph shapes against the oracle, call by call.

The synthetic genome families of the other engine tests make long simple chains with rising positions and little else.  Here the
minimizer lists are written by hand (tests/engine_shapes.py over tests/engine_brute.py's builders: rings, forks, a hub of degree 300,
lone vertices, chains at the lengths where the pointer jumping gains a round, start-end ties, contig changes, 2 000 tiny paths with
boundaries at lanes 63/64 and 255/256, orientation counts at and next to the threshold, indel gaps at the threshold and one over, the
weight filter's boundary, erosion walks of every kind, bubbles that share a vertex, a second add at the edges of a block's interior) and
300 random families of perturbed lists.  After every engine call the state read back -- live vertices, live edges and weights, oriented
paths, block table, terminal / internal marks, counters -- must equal the oracle's, exactly.  tests/test_engine_shapes_host.py proves on
the CPU that every case has the feature it is named for.  Every test runs under a time limit of its own."""
import faulthandler

import pytest

from tests import engine_shapes as ES

pytestmark = pytest.mark.gpu
STEP_SECONDS = 120


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


def device_equals_oracle(ctx, case, what, more=None):
    want, br = ES.oracle_trace(case)
    dev = ES.Dev(ctx, case["G"], **case["par"])
    try:
        got = ES.play(dev, case["script"])
        ES.same(want, got, what)
        lists = more(br) if more is not None else None
        if lists is not None:                                 # one refinement round on top, from the oracle's blocks
            script = [("add", lists)] + ES.REFINE
            d = ES.OracleDriver.__new__(ES.OracleDriver)
            d.br = br
            ES.same(ES.play(d, script), ES.play(dev, script), what + ": refinement")
    finally:
        dev.free()
    return lists is not None


@pytest.mark.parametrize("name", sorted(ES.CASES))
def test_device_engine_equals_the_oracle_after_every_call(ctx, name):
    device_equals_oracle(ctx, ES.CASES[name](), name)


def test_long_erosion_walk_on_the_host_path(ctx_x, monkeypatch):
    "the chain of 120 too-close vertices with every flagged pair walked by nts_engine_erode's host path (experiments build)"
    monkeypatch.setenv("NTS_ERODE_HOST", "1")
    for name in ("erosion_long", "erosion_cross", "erosion_10_9", "erosion_20_19"):
        device_equals_oracle(ctx_x, ES.CASES[name](), name + " on the host path")


def test_start_end_tie_is_settled_differently(ctx):
    """OPEN (docs/design/04_4_graph_stage.md, tests/test_engine_shapes_host.py): with the two ends of a path at the same position of two
    reference contigs and the end the oracle lists last carrying the larger vertex id, k_e_classify starts at the other end -- the
    oracle's path backwards, like the host engine.  Kept until ntJoin's rule is pinned; the "tie" case above is the agreeing half."""
    lay, hs = ES._tie(True)
    dev = ES.Dev(ctx, 3, bp=ES.BIG, n=2)
    try:
        got = ES.play(dev, ES.FIRST(lay.lists))
    finally:
        dev.free()
    want = ES.play(ES.OracleDriver(3, bp=ES.BIG, n=2), ES.FIRST(lay.lists))
    assert got[1][2] == want[1][2]
    assert want[-1][1]["paths"] == [tuple(hs[::-1])] and got[-1][1]["paths"] == [tuple(hs)]


@pytest.mark.parametrize("part", range(6))
def test_random_families(ctx, part):
    "300 seeded families (50 per part): the whole first-round sequence, every fifth with a refinement add on top"
    from tests import engine_brute as EB
    n_refined = 0
    for seed in range(50 * part, 50 * part + 50):
        case = ES.random_script(seed)
        more = None
        if case["refine"]:
            def more(br, seed=seed):
                return EB.refinement_lists(br, seed) if br.blocks_ else None
        n_refined += device_equals_oracle(ctx, case, f"family {seed}", more)
    assert n_refined >= 5
